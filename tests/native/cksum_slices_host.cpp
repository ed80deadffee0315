// The entropy kernel's checksum arithmetic (power-gzip_amd/csrc/nxz_cksum_slices.h, the product code itself) run on
// the host "as 256 lanes would": every lane's part, the sums over the lanes of a wavefront and over the wavefronts in
// the 32-bit registers the kernel has, then finish().  tests/test_cksum_slices_host.py writes the cases and compares
// with zlib.
// usage: cksum_slices_host CASES    CASES: u32 count, then per case u32 h, n, in_crc, in_adler and h + n bytes
// prints "crc adler" (hex) per case.  Every case's bytes stand in an allocation of exactly h + n bytes, so that under
// AddressSanitizer a load outside [src, src + n) on the far side is caught.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "nxz_cksum_slices.h"

static bool rd32(FILE *f, uint32_t &v) { return fread(&v, 4, 1, f) == 1; }

int main(int argc, char **argv)
{
	if (argc != 2) return 2;
	FILE *f = fopen(argv[1], "rb");
	if (!f) return 2;
	uint32_t count;
	if (!rd32(f, count)) return 2;
	std::vector<uint32_t> T(1024);
	for (uint32_t lane = 0; lane < nxzck::LANES; lane++) nxzck::table_column(T.data(), lane);
	for (uint32_t c = 0; c < count; c++) {
		uint32_t h, n, in_crc, in_adler;
		if (!rd32(f, h) || !rd32(f, n) || !rd32(f, in_crc) || !rd32(f, in_adler)) return 2;
		uint8_t *buf = (uint8_t *)malloc(h + n ? h + n : 1);
		if (h + n && fread(buf, 1, h + n, f) != h + n) return 2;
		const nxzck::Shape sh = nxzck::shape_of(n);
		uint32_t crc = 0, tail = 0, s1 = 0, s2 = 0;
		uint64_t s1_wide = 0, s2_wide = 0;
		for (uint32_t wave = 0; wave < nxzck::LANES / 64; wave++) {
			uint32_t wc = 0, wt = 0, w1 = 0, w2 = 0;
			for (uint32_t l = 0; l < 64; l++) {
				const nxzck::Part p = nxzck::lane_part(buf + h, sh, in_crc ^ 0xffffffffu, wave * 64 + l, T.data());
				wc ^= p.crc; wt ^= p.tailcrc; w1 += p.s1; w2 += p.s2;
				s1_wide += p.s1; s2_wide += p.s2;
			}
			crc ^= wc; tail ^= wt; s1 += w1; s2 += w2;
		}
		if (s1 != s1_wide || s2 != s2_wide) { printf("a 32-bit sum wrapped in case %u\n", c); return 1; }
		uint32_t oc, oa;
		nxzck::finish(sh, in_crc, in_adler, crc, tail, s1, s2, oc, oa);
		printf("%08x %08x\n", oc, oa);
		free(buf);
	}
	fclose(f);
	return 0;
}
