// streams_dict_host.cpp -- TEST ONLY.  The rules of nxz_batch_deflate_streams_dict (power-gzip_amd/csrc/nxz_streams_dict.h), the code the
// device runs, compiled for the host.  One request per line on stdin (all numbers decimal), answers on stdout:
//   win dict_len hist_max                       -> "h0 at start": block 0's window, where it begins in the dictionary's 32 KiB device
//                                                  image and where in the dictionary's own bytes
//   bwin k hist_max dict_len                    -> the window of block k
//   fmt fmt                                     -> 1 if the call takes the format, else 0
//   hdr fmt level dictid                        -> "len hex": the header's length and its bytes ("-" for none)
//   bound src_len hist_max fmt                  -> "bound plain_bound": this call's and nxz_batch_deflate_streams'
//   refuse src dst src_len dst_cap hist_max fmt -> the completion code
//   order C blocks_0 blocks_1 ...               -> the launch order of every chunk of C blocks of a batch whose stream i has blocks_i
//                                                  blocks, found as the host finds it (the engine's own plan, nxz_streams_plan.h, run here)
//                                                  and the expand kernel: a line "nf pos_0 pos_1 ..." per chunk
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "nxz_streams_plan.h"

static uint32_t owner_of(const std::vector<uint32_t> &first, uint32_t g)       // (nxz_streams_dev.h)
{
	uint32_t lo = 0, hi = (uint32_t)first.size() - 2;
	while (lo < hi) {
		const uint32_t mid = lo + (hi - lo) / 2;
		if (first[mid + 1] > g) hi = mid; else lo = mid + 1;
	}
	return lo;
}

static void order(char *args)
{
	std::vector<uint32_t> v;
	for (char *p = strtok(args, " \n"); p; p = strtok(nullptr, " \n")) v.push_back((uint32_t)strtoul(p, nullptr, 10));
	const uint32_t C = v[0], n = (uint32_t)v.size() - 1;
	std::vector<uint32_t> first(n + 1), nz(n + 1);
	const int64_t total = nxz_plan_prefix(n, first.data(), nz.data(), [&](size_t i, bool *) { return v[1 + i]; });
	if (total < 0) exit(5);
	for (nxz_plan_chunk c = {0, 0, 0, 0}; nxz_plan_next_chunk(first.data(), (uint32_t)total, C, &c);) {
		const nxz_plan_count f = nxz_plan_dict_firsts(first.data(), nz.data(), c);
		printf("%u", f.inside);
		for (uint32_t t = 0; t < c.m; t++) {
			const uint32_t g = c.b0 + t, i = owner_of(first, g);
			const uint64_t k = g - first[i];
			printf(" %u", nxz_streams_dict_launch_pos(t, k, nxz_streams_dict_firsts_before(nz[i], k) - f.before, f.inside));
		}
		printf("\n");
	}
}

int main()
{
	char line[65536];
	while (fgets(line, sizeof line, stdin)) {
		uint64_t a[6] = {0};
		char what[16] = "";
		const int k = sscanf(line, "%15s %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, what, &a[0], &a[1], &a[2], &a[3], &a[4], &a[5]);
		if (k < 1) continue;
		if (!strcmp(what, "win") && k == 3) {
			const uint32_t h0 = nxz_streams_dict_window((size_t)a[0], (uint32_t)a[1]);
			printf("%u %u %zu\n", h0, nxz_streams_dict_window_at(h0), nxz_streams_dict_window_start((size_t)a[0], (uint32_t)a[1]));
		} else if (!strcmp(what, "bwin") && k == 4) {
			const uint32_t hm = (uint32_t)a[1];
			printf("%u\n", nxz_streams_dict_block_window(a[0], nxz_streams_block_bytes(hm), nxz_streams_window(hm), nxz_streams_dict_window((size_t)a[2], hm)));
		} else if (!strcmp(what, "fmt") && k == 2) printf("%d\n", nxz_streams_dict_fmt_ok((int)a[0]) ? 1 : 0);
		else if (!strcmp(what, "hdr") && k == 4) {
			uint8_t h[6];
			const uint32_t n = nxz_streams_dict_header((int)a[0], (int)(int64_t)a[1], (uint32_t)a[2], h);
			printf("%u ", nxz_streams_dict_header_len((int)a[0]));
			if (!n) printf("-");
			for (uint32_t i = 0; i < n; i++) printf("%02x", h[i]);
			printf("\n");
		} else if (!strcmp(what, "bound") && k == 4)
			printf("%" PRIu64 " %" PRIu64 "\n", nxz_streams_dict_bound(a[0], (uint32_t)a[1], (int)a[2]), nxz_streams_bound(a[0], (uint32_t)a[1], (int)a[2]));
		else if (!strcmp(what, "refuse") && k == 7) {
			nxz_stream_job_t j;
			j.src = (const uint8_t *)(uintptr_t)a[0]; j.dst = (uint8_t *)(uintptr_t)a[1]; j.src_len = a[2]; j.dst_cap = a[3];
			printf("%u\n", nxz_streams_dict_refusal(&j, (uint32_t)a[4], (int)a[5]));
		} else if (!strcmp(what, "order") && k >= 2) order(line + 5);
		else return 2;
	}
	return 0;
}
