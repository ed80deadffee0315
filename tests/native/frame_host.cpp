// frame_host.cpp -- TEST ONLY.  The engine's zlib / gzip header parser, trailer rule and BGZF member check
// (power-gzip_amd/csrc/nxz_frame.h, the code the device runs) compiled for the host.  Reads records from stdin:
//   u8 kind, u8 fmt, u32 len (little-endian), len bytes
// kind 0: parse the header (fmt = NXZ_FMT_*) -> "status format hdr_len extra_off extra_len name_off comment_off flg xfl os cinfo mtime dictid"
// kind 1: BGZF member size at the start -> "size"
// kind 2: CRC-32 of the bytes, by the 64 slices the device combines -> "crc"
// kind 3: the trailer rule (fmt = the frame's format, | 0x80: compare the checksum).  The bytes are eight little-endian words -- hdr_len
//         and the result's cc, sfbt, spbc, subc, tpbc, crc, adler -- and then the job's source -> "status end check isize"
// Every record's bytes sit in an allocation of exactly their length (run under AddressSanitizer).  The first line is the
// layout of nxz_batch_frame_t: its size and the offsets of its fields.
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>
#include "nxz_frame.h"

struct HostOps {
	uint32_t find_nul(const uint8_t *p, uint32_t from, uint32_t len)
	{
		for (uint32_t i = from; i < len; i++) if (!p[i]) return i;
		return len;
	}
	uint32_t crc32(const uint8_t *p, uint32_t n)
	{
		uint32_t v = 0;
		for (uint32_t k = 0; k < 64; k++) {
			uint32_t lo, hi;
			nxz_slice(n, 64, k, &lo, &hi);
			v ^= nxz_crc_part(p, lo, hi, n);
		}
		return nxz_crc_finish(v, n);
	}
};

int main()
{
	printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(nxz_batch_frame_t),
	       offsetof(nxz_batch_frame_t, status), offsetof(nxz_batch_frame_t, format), offsetof(nxz_batch_frame_t, hdr_len),
	       offsetof(nxz_batch_frame_t, end), offsetof(nxz_batch_frame_t, check), offsetof(nxz_batch_frame_t, isize),
	       offsetof(nxz_batch_frame_t, mtime), offsetof(nxz_batch_frame_t, dictid), offsetof(nxz_batch_frame_t, extra_off),
	       offsetof(nxz_batch_frame_t, extra_len), offsetof(nxz_batch_frame_t, name_off), offsetof(nxz_batch_frame_t, comment_off),
	       offsetof(nxz_batch_frame_t, flg), offsetof(nxz_batch_frame_t, xfl), offsetof(nxz_batch_frame_t, os),
	       offsetof(nxz_batch_frame_t, cinfo));
	HostOps ops;
	for (;;) {
		uint8_t h[6];
		if (fread(h, 1, 6, stdin) != 6) break;
		const uint32_t len = (uint32_t)h[2] | (uint32_t)h[3] << 8 | (uint32_t)h[4] << 16 | (uint32_t)h[5] << 24;
		std::vector<uint8_t> buf(len);
		if (len && fread(buf.data(), 1, len, stdin) != len) return 2;
		const uint8_t *p = buf.data();
		if (h[0] == 0) {
			nxz_batch_frame_t f;
			nxz_frame_parse(p, len, h[1], &f, ops);
			printf("%u %u %u %u %u %u %u %u %u %u %u %u %u\n", f.status, f.format, f.hdr_len, f.extra_off, f.extra_len, f.name_off,
			       f.comment_off, f.flg, f.xfl, f.os, f.cinfo, f.mtime, f.dictid);
		} else if (h[0] == 1) {
			printf("%u\n", nxz_bgzf_member_size(p, len));
		} else if (h[0] == 3) {
			if (len < 32) return 2;
			uint32_t w[8];
			for (int k = 0; k < 8; k++) w[k] = nxz_rd32le(p + 4 * k);
			nxz_batch_result_t r = {};
			r.cc = w[1]; r.sfbt = w[2]; r.spbc = w[3]; r.subc = w[4]; r.tpbc = w[5]; r.crc = w[6]; r.adler = w[7];
			const std::vector<uint8_t> src(buf.begin() + 32, buf.end());   // (an allocation of the source's own length)
			uint32_t end, check, isize;
			const uint32_t st = nxz_frame_trailer(h[1] & 0x7f, w[0], &r, src.data(), len - 32, (h[1] & 0x80) != 0, &end, &check, &isize);
			printf("%u %u %u %u\n", st, end, check, isize);
		} else {
			printf("%u\n", ops.crc32(p, len));
		}
	}
	return 0;
}
