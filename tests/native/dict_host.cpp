// dict_host.cpp -- TEST ONLY.  The rules of a preset dictionary (power-gzip_amd/csrc/nxz_dict.h) and the FDICT branch of the
// header parser (nxz_frame.h: nxz_frame_parse_dict), the code the device runs, compiled for the host.  Records on stdin:
//   u8 kind, u8 arg, u32 len (little-endian), len bytes
// kind 0: the windows of a dictionary of these bytes -> "inflate_window inflate_start deflate_window deflate_start max_source dictid"
// kind 1: the zlib header for level arg - 1 (0 = level -1) and the DICTID of these bytes -> twelve hex digits
// kind 2: does a compress job fit?  bytes = u32 W, u32 src_len, u32 hist_len -> "0" / "1"
// kind 3: parse a header with a dictionary: arg = fmt | have_dict << 4; bytes = u32 dictid, then the stream
//         -> "status format hdr_len flg cinfo dictid use_dict"
// Every record's bytes sit in an allocation of exactly their length (run under AddressSanitizer).
#include <cstdio>
#include <cstring>
#include <vector>
#include "nxz_dict.h"
#include "nxz_frame.h"

struct HostOps {
	uint32_t find_nul(const uint8_t *p, uint32_t from, uint32_t len)
	{
		for (uint32_t i = from; i < len; i++) if (!p[i]) return i;
		return len;
	}
	uint32_t crc32(const uint8_t *p, uint32_t n) { return nxz_crc_finish(nxz_crc_part(p, 0, n, n), n); }
};

int main()
{
	HostOps ops;
	for (;;) {
		uint8_t h[6];
		if (fread(h, 1, 6, stdin) != 6) break;
		const uint32_t len = nxz_rd32le(h + 2);
		std::vector<uint8_t> buf(len);
		if (len && fread(buf.data(), 1, len, stdin) != len) return 2;
		const uint8_t *p = buf.data();
		if (h[0] == 0) {
			printf("%u %zu %u %zu %u %u\n", nxz_dict_inflate_window(len), nxz_dict_inflate_start(len), nxz_dict_deflate_window(len),
			       nxz_dict_deflate_start(len), nxz_dict_max_source(len), nxz_dict_adler32(p, len));
		} else if (h[0] == 1) {
			uint8_t o[6];
			nxz_zlib_dict_header((int)h[1] - 1, nxz_dict_adler32(p, len), o);
			printf("%02x%02x%02x%02x%02x%02x\n", o[0], o[1], o[2], o[3], o[4], o[5]);
		} else if (h[0] == 2) {
			if (len != 12) return 2;
			printf("%d\n", nxz_dict_job_fits(nxz_rd32le(p), nxz_rd32le(p + 4), nxz_rd32le(p + 8)) ? 1 : 0);
		} else {
			if (len < 4) return 2;
			// (the stream in an allocation of its own, so that a read past its end is caught)
			std::vector<uint8_t> s(buf.begin() + 4, buf.end());
			nxz_batch_frame_t f;
			bool use = false;
			nxz_frame_parse_dict(s.data(), (uint32_t)s.size(), h[1] & 15, &f, ops, (h[1] >> 4) != 0, nxz_rd32le(p), &use);
			printf("%u %u %u %u %u %u %d\n", f.status, f.format, f.hdr_len, f.flg, f.cinfo, f.dictid, use ? 1 : 0);
		}
	}
	return 0;
}
