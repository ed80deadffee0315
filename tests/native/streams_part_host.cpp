// streams_part_host.cpp -- TEST ONLY.  The rules of nxz_batch_deflate_streams_part (power-gzip_amd/csrc/nxz_streams_part.h), the code the
// device runs, compiled for the host.  One request per line on stdin (all numbers decimal), answers on stdout:
//   win prev_len hist_max                            -> h0: block 0's window
//   bwin k hist_max prev_len                         -> the window of block k
//   bound src_len hist_max fmt flags                 -> "bound header_len trailer_len"
//   refuse src dst src_len dst_cap prev prev_len flags carry_status hist_max fmt -> the completion code
//   staged src src_len prev prev_len hist_max        -> "contiguous staged"
//   carry first crc adler total_in total_out parts status | crc adler src_len out_len flags
//                                                    -> the carry a part starts from (`first`: 1 with NXZ_PART_FIRST) and the one it
//                                                       leaves: "crc adler total_in total_out parts status" twice
//   frame fmt level flags crc adler total_len        -> "hex hex": the header and the trailer bytes this part writes ("-" for none)
//   plan C staged_0 blocks_0 staged_1 blocks_1 ...   -> per chunk of C blocks "sg_b0 nst q..." as the host finds them (the engine's own plan,
//                                                       nxz_streams_plan.h, run here) and the expand kernel: the staged first blocks in front of the chunk, inside
//                                                       it, and the slot of each staged block of the chunk in the batch's order
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "nxz_streams_part.h"
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

static void plan(char *args)
{
	std::vector<uint32_t> v;
	for (char *p = strtok(args, " \n"); p; p = strtok(nullptr, " \n")) v.push_back((uint32_t)strtoul(p, nullptr, 10));
	const uint32_t C = v[0], n = ((uint32_t)v.size() - 1) / 2;
	std::vector<uint32_t> first(n + 1), sg(n + 1);
	const int64_t total = nxz_plan_prefix(n, first.data(), sg.data(), [&](size_t i, bool *staged) { *staged = v[1 + 2 * i] != 0; return v[2 + 2 * i]; });
	if (total < 0) exit(5);
	for (nxz_plan_chunk k = {0, 0, 0, 0}; nxz_plan_next_chunk(first.data(), (uint32_t)total, C, &k);) {
		const nxz_plan_count c = nxz_plan_part_staged(first.data(), sg.data(), k);
		printf("%u %u", c.before, c.inside);
		for (uint32_t t = 0; t < k.m; t++) {
			const uint32_t g = k.b0 + t, i = owner_of(first, g);
			if (g == first[i] && sg[i + 1] != sg[i]) printf(" %u", sg[i] - c.before);
		}
		printf("\n");
	}
}

static void hex(const uint8_t *b, uint32_t n)
{
	if (!n) printf("-");
	for (uint32_t i = 0; i < n; i++) printf("%02x", b[i]);
}

static void print_carry(const nxz_stream_carry_t &c)
{
	printf("%u %u %" PRIu64 " %" PRIu64 " %u %u", c.crc, c.adler, c.total_in, c.total_out, c.parts, c.status);
}

int main()
{
	static char line[1 << 20];
	static_assert(sizeof(nxz_stream_part_job_t) == 48 && sizeof(nxz_stream_carry_t) == 32, "the records' sizes");
	while (fgets(line, sizeof line, stdin)) {
		uint64_t a[12] = {0};
		char what[16] = "";
		const int k = sscanf(line, "%15s %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64
				     " %" SCNu64 " %" SCNu64, what, &a[0], &a[1], &a[2], &a[3], &a[4], &a[5], &a[6], &a[7], &a[8], &a[9], &a[10], &a[11]);
		if (k < 1) continue;
		if (!strcmp(what, "win") && k == 3) printf("%u\n", nxz_streams_part_window((uint32_t)a[0], (uint32_t)a[1]));
		else if (!strcmp(what, "bwin") && k == 4) {
			const uint32_t hm = (uint32_t)a[1];
			printf("%u\n", nxz_streams_part_block_window(a[0], nxz_streams_block_bytes(hm), nxz_streams_window(hm), nxz_streams_part_window((uint32_t)a[2], hm)));
		} else if (!strcmp(what, "bound") && k == 5)
			printf("%" PRIu64 " %u %u\n", nxz_streams_part_bound(a[0], (uint32_t)a[1], (int)a[2], (uint32_t)a[3]),
			       nxz_streams_part_header_len((int)a[2], (uint32_t)a[3]), nxz_streams_part_trailer_len((int)a[2], (uint32_t)a[3]));
		else if (!strcmp(what, "refuse") && k == 11) {
			nxz_stream_part_job_t j;
			j.src = (const uint8_t *)(uintptr_t)a[0]; j.dst = (uint8_t *)(uintptr_t)a[1]; j.src_len = a[2]; j.dst_cap = a[3];
			j.prev = (const uint8_t *)(uintptr_t)a[4]; j.prev_len = (uint32_t)a[5]; j.flags = (uint32_t)a[6];
			printf("%u\n", nxz_streams_part_refusal(&j, (uint32_t)a[7], (uint32_t)a[8], (int)a[9]));
		} else if (!strcmp(what, "staged") && k == 6) {
			nxz_stream_part_job_t j;
			j.src = (const uint8_t *)(uintptr_t)a[0]; j.dst = nullptr; j.src_len = a[1]; j.dst_cap = 0;
			j.prev = (const uint8_t *)(uintptr_t)a[2]; j.prev_len = (uint32_t)a[3]; j.flags = 0;
			printf("%d %d\n", nxz_streams_part_contiguous(&j) ? 1 : 0, nxz_streams_part_staged(&j, (uint32_t)a[4]) ? 1 : 0);
		} else if (!strcmp(what, "carry") && k == 13) {
			nxz_stream_carry_t c;
			c.crc = (uint32_t)a[1]; c.adler = (uint32_t)a[2]; c.total_in = a[3]; c.total_out = a[4]; c.parts = (uint32_t)a[5]; c.status = (uint32_t)a[6];
			const uint32_t flags = (uint32_t)a[11];
			if (((flags & NXZ_PART_FIRST) != 0) != (a[0] != 0)) return 3;
			const nxz_stream_carry_t in = nxz_streams_part_carry_in(&c, flags);
			const nxz_stream_carry_t out = nxz_streams_part_carry_out(&in, (uint32_t)a[7], (uint32_t)a[8], a[9], a[10], flags);
			print_carry(in); printf(" "); print_carry(out); printf("\n");
		} else if (!strcmp(what, "frame") && k == 7) {
			const int fmt = (int)a[0];
			const uint32_t flags = (uint32_t)a[2];
			uint8_t h[10], t[8];
			const uint32_t hl = flags & NXZ_PART_FIRST ? nxz_streams_header(fmt, (int)(int64_t)a[1], h) : 0;
			const uint32_t tl = flags & NXZ_PART_LAST ? nxz_streams_trailer(fmt, (uint32_t)a[3], (uint32_t)a[4], a[5], t) : 0;
			if (hl != nxz_streams_part_header_len(fmt, flags) || tl != nxz_streams_part_trailer_len(fmt, flags)) return 4;
			hex(h, hl); printf(" "); hex(t, tl); printf("\n");
		} else if (!strcmp(what, "plan") && k >= 2) plan(line + 4);
		else return 2;
	}
	return 0;
}
