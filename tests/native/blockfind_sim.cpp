// blockfind_sim.cpp -- TEST INFRASTRUCTURE: the block search of the one-stream inflate (power-gzip_amd/csrc/nxz_blockfind.hip,
// the product source itself: find_blocks_kernel, check_headers_kernel, header_ok, header_ok_wave) run on the CPU through
// tests/native/hip_cpu_shim.h, an OS thread per lane, a workgroup per segment, one after the other.  It judges nothing: it
// runs the streams of a case file (tests/test_blockfind_sim.py: the hand-built headers of tests/blockfind_cases.py) and
// prints `first` -- the first header of every segment, then NXZ_BLOCKFIND_MORE further ones per segment -- as
// nxz_launch_find_blocks leaves it, for the caller to compare with tests/blockfind_model.py.
//   usage: blockfind_sim <case file>
//   case file: u32 n, then n times { u32 src_len, offset of src in its 16-byte granule, seg_bytes, mode; u64 first_bit; src_len bytes }
//     mode 0: two kernels, as the launcher runs them by default; 1: the first kernel alone (NXZ_BLOCKFIND_TWO=0), `more`
//     all ~0 as the launcher's memset leaves it; 2: the first kernel alone with diag = 5 (header_ok_wave: a wavefront per
//     candidate), which the launcher reaches through NXZ_BLOCKFIND_DIAG only
//     3: header_ok by a lane and header_ok_wave by a wavefront, alone, at bit first_bit of a stream of one segment (the code-length
//     code's Kraft sum included, which inside the search the first test has decided before either is called): "case <i> 1 1 <lane> <wave> 0 0"
//   output: a line per case: "case <i> <nseg> <intact>" and nseg * 4 numbers; the last line is "ran"
//   (intact: the bytes in front of and behind `first` and the scratch area are as they were)
// Built with -I tests/native/hip_sim, where hip/hip_runtime.h stands in for HIP's and includes the shim.
#define __HIPCC__ 1
#include "hip_cpu_shim.h"
#include "../../power-gzip_amd/csrc/nxz_blockfind.hip"
#include <stdio.h>
#include <vector>

int main(int argc, char **argv)
{
	if (argc < 2) { fprintf(stderr, "usage: %s <case file>\n", argv[0]); return 2; }
	FILE *f = fopen(argv[1], "rb");
	if (!f) { perror(argv[1]); return 2; }
	uint32_t n = 0;
	if (fread(&n, 4, 1, f) != 1 || n > 4096) { fprintf(stderr, "%s: no case file\n", argv[1]); return 2; }
	const size_t GUARD = 8;                             // (64-bit words around `first`, and as many 16-bit words around the scratch area)
	for (uint32_t i = 0; i < n; i++) {
		uint32_t h[4];
		uint64_t first_bit = 0;
		if (fread(h, 4, 4, f) != 4 || fread(&first_bit, 8, 1, f) != 1 || h[0] > (1u << 24) || h[1] > 15 || h[2] < 512 || h[2] > nxzb::SEG || h[3] > 3) {
			fprintf(stderr, "%s: case %u\n", argv[1], i);
			return 2;
		}
		const uint32_t srclen = h[0], seg_bytes = h[2], mode = h[3];
		std::vector<uint8_t> buf(srclen + 64 + 32, 0xa5);        // (what lies behind the stream is no zeros)
		uint8_t *src = (uint8_t *)(((uintptr_t)buf.data() + 15) & ~(uintptr_t)15) + h[1];
		if (srclen && fread(src, 1, srclen, f) != srclen) { fprintf(stderr, "%s: case %u is cut short\n", argv[1], i); return 2; }
		if (mode == 3) {
			// the two header checkers alone, at bit first_bit of a stream that is its own segment: a lane, and a wavefront
			if (srclen > nxzb::SEG + nxzb::LOOK) { fprintf(stderr, "%s: case %u is too long for one segment\n", argv[1], i); return 2; }
			static __attribute__((aligned(16))) uint8_t seg[nxzb::SEG + nxzb::LOOK + 16];
			memset(seg, 0, sizeof(seg));
			memcpy(seg, src, srclen);
			uint32_t lane_says = 0, wave_says = 0;
			hipsim_run_block(0, 1, 64, [&] {
				const bool a = threadIdx.x == 0 && nxzb::header_ok(seg, (uint32_t)first_bit, srclen * 8, 0xffffffffu);
				const bool b = nxzb::header_ok_wave((const uint32_t *)seg, sizeof(seg) / 4, (uint32_t)first_bit, srclen * 8, (int)threadIdx.x);
				if (threadIdx.x == 0) { lane_says = a; wave_says = b; }
			});
			printf("case %u 1 1 %u %u 0 0\n", i, lane_says, wave_says);
			continue;
		}
		const uint32_t nseg = (srclen + seg_bytes - 1) / seg_bytes;
		const size_t nfirst = (size_t)nseg * (1 + NXZ_BLOCKFIND_MORE), nleft = nxz_blockfind_scratch(nseg) / sizeof(uint16_t);
		std::vector<uint64_t> fb(nfirst + 2 * GUARD, 0x5a5a5a5a5a5a5a5aull);
		std::vector<uint16_t> lb(nleft + 2 * GUARD, 0x5a5a);
		uint64_t *first = fb.data() + GUARD;
		uint16_t *left = mode == 0 ? lb.data() + GUARD : nullptr;
		const uint32_t diag = mode == 2 ? 5 : 0;
		for (uint32_t g = 0; g < nseg; g++)
			hipsim_run_block(g, nseg, nxzb::NT, [&] { nxzb::find_blocks_kernel(src, srclen, first_bit, first, nseg, seg_bytes, diag, left); });
		if (left)
			for (uint32_t g = 0; g < nseg; g++)
				hipsim_run_block(g, nseg, 64, [&] { nxzb::check_headers_kernel(src, srclen, first, nseg, seg_bytes, left); });
		else
			memset(first + nseg, 0xff, (size_t)nseg * NXZ_BLOCKFIND_MORE * sizeof(uint64_t));
		int intact = 1;
		for (size_t k = 0; k < GUARD; k++) {
			if (fb[k] != 0x5a5a5a5a5a5a5a5aull || fb[GUARD + nfirst + k] != 0x5a5a5a5a5a5a5a5aull) intact = 0;
			if (lb[k] != 0x5a5a || lb[GUARD + nleft + k] != 0x5a5a) intact = 0;
		}
		printf("case %u %u %d", i, nseg, intact);
		for (size_t k = 0; k < nfirst; k++) printf(" %llu", (unsigned long long)first[k]);
		printf("\n");
		fflush(stdout);
	}
	fclose(f);
	printf("ran\n");
	return 0;
}
