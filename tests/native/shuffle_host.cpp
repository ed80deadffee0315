// shuffle_host.cpp -- TEST ONLY.  The plan of nxz_batch_shuffle / nxz_batch_unshuffle (power-gzip_amd/csrc/nxz_shuffle.h), the code the
// engine's host side and the kernel run, compiled for the host.  One request per line on stdin (all numbers decimal), answers on stdout:
//   tile elem                                  -> T: the elements of a tile
//   slots T                                    -> the 16-byte slots a plane's run of a tile touches at most
//   tiles n_elems elem                         -> the tiles of a job
//   overlap a b len                            -> 1 when [a, a + len) and [b, b + len) share a byte
//   refuse src dst len elem reserved           -> the status
//   job src dst len elem reserved              -> "status n_elems elem tail": what the kernel gets
//   batch src dst len elem reserved ...        -> "total | first[0..n] | status[0..n-1]" of nxz_shuffle_plan_batch (total -1: too many tiles)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "nxz_shuffle.h"

static nxz_shuffle_job_t job_of(const uint64_t *v)
{
	nxz_shuffle_job_t j;
	j.src = (const uint8_t *)(uintptr_t)v[0]; j.dst = (uint8_t *)(uintptr_t)v[1]; j.len = v[2]; j.elem = (uint32_t)v[3]; j.reserved = (uint32_t)v[4];
	return j;
}

int main()
{
	static char line[1 << 20];
	while (fgets(line, sizeof line, stdin)) {
		char *cmd = strtok(line, " \n");
		if (!cmd) continue;
		std::vector<uint64_t> v;
		for (char *p = strtok(nullptr, " \n"); p; p = strtok(nullptr, " \n")) v.push_back(strtoull(p, nullptr, 10));
		if (!strcmp(cmd, "tile") && v.size() == 1) printf("%u\n", nxz_shuffle_tile_elems_of((uint32_t)v[0]));
		else if (!strcmp(cmd, "slots") && v.size() == 1) printf("%u\n", nxz_shuffle_plane_slots((uint32_t)v[0]));
		else if (!strcmp(cmd, "tiles") && v.size() == 2) printf("%" PRIu64 "\n", nxz_shuffle_tiles(v[0], (uint32_t)v[1]));
		else if (!strcmp(cmd, "overlap") && v.size() == 3) printf("%d\n", nxz_shuffle_overlap(v[0], v[1], v[2]) ? 1 : 0);
		else if (!strcmp(cmd, "refuse") && v.size() == 5) { const nxz_shuffle_job_t j = job_of(v.data()); printf("%u\n", nxz_shuffle_refusal(&j)); }
		else if (!strcmp(cmd, "job") && v.size() == 5) {
			const nxz_shuffle_job_t j = job_of(v.data());
			nxz_shuffle_plan_t p;
			const uint32_t st = nxz_shuffle_plan_job(&j, &p);
			if (p.src != j.src || p.dst != j.dst) return 4;
			printf("%u %" PRIu64 " %u %u\n", st, p.n_elems, p.elem, p.tail);
		} else if (!strcmp(cmd, "batch") && v.size() % 5 == 0) {
			const size_t n = v.size() / 5;
			std::vector<nxz_shuffle_job_t> jobs;
			for (size_t i = 0; i < n; i++) jobs.push_back(job_of(&v[5 * i]));
			// (exact sizes: the sanitizer sees a write past first[n] or status[n - 1])
			std::vector<nxz_shuffle_plan_t> plan(n);
			std::vector<uint32_t> first(n + 1), status(n);
			const int64_t total = nxz_shuffle_plan_batch(jobs.data(), n, plan.data(), first.data(), status.data());
			printf("%" PRId64 " |", total);
			if (total >= 0) for (uint32_t f : first) printf(" %u", f);
			printf(" |");
			if (total >= 0) for (uint32_t s : status) printf(" %u", s);
			printf("\n");
		} else return 3;
	}
	return 0;
}
