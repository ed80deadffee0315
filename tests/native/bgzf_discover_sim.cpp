// bgzf_discover_sim.cpp -- TEST INFRASTRUCTURE: the BGZF member discovery (power-gzip_amd/csrc/nxz_frame.hip, the product source
// itself: bgzf_scan_kernel<false|true>, tile_scan_kernel, succ_kernel, jump_kernel, chain_kernel, member_kernel, layout_kernel,
// coff_kernel) run on the CPU through tests/native/hip_cpu_shim.h in the order nxz_launch_bgzf_discover / nxz_launch_bgzf_coff
// launch them, a workgroup at a time.  The kernels with barriers or lane exchanges (the scan, the two prefix sums) get an OS
// thread per lane; the others, whose lanes never meet, run their lanes one after the other.  It judges nothing: it runs the
// images of a case file (tests/test_bgzf_discover_sim.py: tests/bgzf_discover_cases.py) and writes what the launchers left for
// the caller to compare with tests/bgzf_model.py discover().
// The workspace is exactly nxz_bgzf_workspace(len, cap) bytes from malloc and the image's buffer ends 64 bytes behind the image:
// under -fsanitize=address a read or write past either shows.
//   usage: bgzf_discover_sim <case file> <result file>
//   case file: u32 n, then n records.  u32 mode;
//     mode 0: u32 len, head (the byte of its 16-byte granule packed[0] lies at); u64 cap, max_members; 64 bytes in front of the
//             image, len bytes, 64 bytes behind it
//     mode 1: u32 ntiles; ntiles x u32 counts -- tile_scan_kernel alone
//   result file, a record per case, every array as it lies in memory with 0xa5 where nothing was written:
//     mode 0: u64 ctl[4], packed, dst, intact; u64 pos[cap]; u32 size[cap]; u64 offsets[max_members + 1], coff[max_members + 1];
//             the jobs (cap x 48 bytes)
//     mode 1: u32 off[ntiles]; u64 ctl[0], intact
//   (intact: the words around offsets, coff, off are as they were)
// Built with -I tests/native/hip_sim, where hip/hip_runtime.h stands in for HIP's and includes the shim.
#define __HIPCC__ 1
#include "hip_cpu_shim.h"
#include "../../power-gzip_amd/csrc/nxz_frame.hip"
#include <stdio.h>
#include <vector>

static const size_t GUARD = 32, PAD = 64;
static const uint64_t S8 = 0xa5a5a5a5a5a5a5a5ull;

// a workgroup whose lanes never wait for each other: one lane after the other on this thread
template <typename F> static void run_serial(unsigned b, unsigned nblocks, unsigned threads, F kernel)
{
	blockDim = { threads, 1, 1 };
	gridDim = { nblocks, 1, 1 };
	for (unsigned t = 0; t < threads; t++) {
		threadIdx = { t, 0, 0 };
		blockIdx = { b, 0, 0 };
		kernel();
	}
}

static bool guards_ok(const std::vector<uint64_t> &v, size_t n)
{
	for (size_t k = 0; k < GUARD; k++)
		if (v[k] != S8 || v[GUARD + n + k] != S8) return false;
	return true;
}

static int put(FILE *o, const void *p, size_t n) { return !n || fwrite(p, 1, n, o) == n; }

int main(int argc, char **argv)
{
	if (argc < 3) { fprintf(stderr, "usage: %s <case file> <result file>\n", argv[0]); return 2; }
	FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
	if (!f || !o) { perror(f ? argv[2] : argv[1]); return 2; }
	uint32_t n = 0;
	if (fread(&n, 4, 1, f) != 1 || n > 65536) { fprintf(stderr, "%s: no case file\n", argv[1]); return 2; }
	for (uint32_t i = 0; i < n; i++) {
		uint32_t mode = 0;
		if (fread(&mode, 4, 1, f) != 1 || mode > 1) { fprintf(stderr, "%s: case %u\n", argv[1], i); return 2; }
		if (mode == 1) {
			uint32_t nt = 0;
			if (fread(&nt, 4, 1, f) != 1 || nt == 0 || nt > (1u << 20)) { fprintf(stderr, "%s: case %u\n", argv[1], i); return 2; }
			// (as the launcher lays them out: one word of room behind the last tile's)
			uint32_t *cnt = (uint32_t *)malloc(((size_t)nt + 1) * 4);
			std::vector<uint64_t> ob(((size_t)nt + 1) / 2 + 1 + 2 * GUARD, S8);
			uint32_t *off = (uint32_t *)(ob.data() + GUARD);
			uint64_t ctl[4] = { S8, S8, S8, S8 };
			if (fread(cnt, 4, nt, f) != nt) { fprintf(stderr, "%s: case %u is cut short\n", argv[1], i); return 2; }
			cnt[nt] = 0xa5a5a5a5u;
			hipsim_run_block(0, 1, 1024, [&] { nxzf::tile_scan_kernel(cnt, nt, off, ctl); });
			uint64_t intact = guards_ok(ob, ((size_t)nt + 1) / 2 + 1) && off[nt] == 0xa5a5a5a5u && ctl[1] == S8;
			if (!put(o, off, (size_t)nt * 4) || !put(o, ctl, 8) || !put(o, &intact, 8)) return 2;
			free(cnt);
			continue;
		}
		uint32_t h[2];
		uint64_t q[2];
		if (fread(h, 4, 2, f) != 2 || fread(q, 8, 2, f) != 2 || h[0] > (1u << 26) || h[1] > 15 || q[0] > (1u << 24) || q[1] > (1u << 24)) {
			fprintf(stderr, "%s: case %u\n", argv[1], i);
			return 2;
		}
		const uint64_t len = h[0], head = h[1], cap = q[0], mm = q[1];
		// the image's buffer: 16-byte aligned, PAD bytes + head in front of the image, PAD bytes behind it (and what rounds the size up to 16)
		uint8_t *raw = (uint8_t *)aligned_alloc(16, (PAD + head + len + PAD + 15) & ~(size_t)15);
		uint8_t *packed = raw + PAD + head;
		memset(raw, 0xee, PAD + head);
		if (fread(packed - PAD, 1, PAD + len + PAD, f) != PAD + len + PAD) { fprintf(stderr, "%s: case %u is cut short\n", argv[1], i); return 2; }
		const size_t wsn = nxz_bgzf_workspace(len, cap);
		uint8_t *ws = (uint8_t *)malloc(wsn);
		memset(ws, 0xa5, wsn);
		std::vector<uint64_t> ob(mm + 1 + 2 * GUARD, S8), cb(mm + 1 + 2 * GUARD, S8);
		uint64_t *offsets = ob.data() + GUARD, *coff = cb.data() + GUARD;
		uint8_t *dst = (uint8_t *)(uintptr_t)0x700000000000ull;             // (an address: the discovery never touches what the members decode to)
		nxz_batch_job_t *jobs = nullptr;
		if (nxz_launch_bgzf_discover(packed, len, dst, offsets, mm, ws, cap, &jobs, nullptr)) return 3;   // (here: its memset, and where the jobs lie)
		const BgzfWs w = bgzf_ws(ws, packed, len, cap);
		const unsigned tiles = (unsigned)w.tiles, g = (unsigned)((cap + 1 + 255) / 256);
		if ((uint8_t *)jobs != (uint8_t *)w.jobs || (uint8_t *)(w.jobs + cap) > ws + wsn) return 3;
		for (unsigned b = 0; b < tiles; b++)
			hipsim_run_block(b, tiles, 256, [&] { nxzf::bgzf_scan_kernel<false>(packed, len, w.tile_cnt, nullptr, cap, nullptr, nullptr); });
		hipsim_run_block(0, 1, 1024, [&] { nxzf::tile_scan_kernel(w.tile_cnt, tiles, w.tile_off, w.ctl); });
		for (unsigned b = 0; b < tiles; b++)
			hipsim_run_block(b, tiles, 256, [&] { nxzf::bgzf_scan_kernel<true>(packed, len, nullptr, w.tile_off, cap, w.pos, w.size); });
		for (unsigned b = 0; b < g; b++) run_serial(b, g, 256, [&] { nxzf::succ_kernel(w.pos, w.size, w.ctl, cap, w.J); });
		for (uint32_t r = 0; r + 1 < w.levels; r++)
			for (unsigned b = 0; b < g; b++)
				run_serial(b, g, 256, [&] { nxzf::jump_kernel(w.J + (size_t)r * (cap + 1), w.ctl, cap, w.J + (size_t)(r + 1) * (cap + 1)); });
		run_serial(0, 1, 1, [&] { nxzf::chain_kernel(w.pos, w.size, w.ctl, cap, w.J, w.levels); });
		for (unsigned b = 0; b < g; b++)
			run_serial(b, g, 256, [&] { nxzf::member_kernel(packed, w.pos, w.size, w.ctl, cap, w.J, w.levels, mm, w.memb, w.isz); });
		hipsim_run_block(0, 1, 1024, [&] { nxzf::layout_kernel(packed, w.pos, w.size, w.ctl, mm, w.memb, w.isz, dst, offsets, jobs); });
		if (nxz_launch_bgzf_coff(packed, len, ws, cap, mm, coff, nullptr)) return 3;
		const unsigned gc = (unsigned)(((mm < cap ? mm : cap) + 1 + 255) / 256);
		for (unsigned b = 0; b < gc; b++) run_serial(b, gc, 256, [&] { nxzf::coff_kernel(w.pos, w.ctl, mm, w.memb, coff); });
		const uint64_t pa = (uint64_t)(uintptr_t)packed, da = (uint64_t)(uintptr_t)dst, intact = guards_ok(ob, mm + 1) && guards_ok(cb, mm + 1);
		if (!put(o, w.ctl, 32) || !put(o, &pa, 8) || !put(o, &da, 8) || !put(o, &intact, 8) || !put(o, w.pos, cap * 8) || !put(o, w.size, cap * 4) ||
		    !put(o, offsets, (mm + 1) * 8) || !put(o, coff, (mm + 1) * 8) || !put(o, jobs, cap * sizeof(nxz_batch_job_t)))
			return 2;
		free(ws);
		free(raw);
	}
	fclose(f);
	if (fclose(o)) return 2;
	printf("ran %u\n", n);
	return 0;
}
