// nxz_dict.h -- the rules of a shared preset dictionary (nxz_dict_t, include/nxz_engine.h) as plain code that compiles
// for the device (the kernels of the nxz_batch_*_dict calls) and for the host (nxz_batch.cpp, tests/native/dict_host.cpp).
//
// A dictionary is `len` bytes that every job of a batch may refer to as if they stood in front of its data:
//   inflate window   the last min(len, 32768) bytes -- what zlib's inflateSetDictionary keeps;
//   deflate window   the last W = min(len, 32768) & ~15 bytes.  The compress kernels take a history that is a multiple of 16
//                    bytes; up to 15 leading bytes are dropped, which is legal: the encoder merely never refers to them.
//                    (Padding instead would not be: a match into padding decodes differently.)  A job carries at most
//                    65536 - W bytes of source;
//   DICTID           Adler-32 of all len bytes from 1 (RFC 1950 2.2), 1 for an empty dictionary;
//   zlib header      CMF 0x78, FLG with FLEVEL from the level as zlib's deflate.c sets it, FDICT set, FCHECK so that
//                    CMF * 256 + FLG is a multiple of 31; then DICTID, most significant byte first.
#ifndef NXZ_DICT_H
#define NXZ_DICT_H
#include <stdint.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define NXZ_DICT_HD __host__ __device__
#else
#define NXZ_DICT_HD
#endif

#define NXZ_DICT_WINDOW 32768u
#define NXZ_DICT_BLOCK  65536u       /* window + source of one compress job: the LZ77 kernel's LDS image */

NXZ_DICT_HD inline uint32_t nxz_dict_inflate_window(size_t len) { return len < NXZ_DICT_WINDOW ? (uint32_t)len : NXZ_DICT_WINDOW; }
NXZ_DICT_HD inline uint32_t nxz_dict_deflate_window(size_t len) { return nxz_dict_inflate_window(len) & ~15u; }
/* where the windows begin in the dictionary's bytes */
NXZ_DICT_HD inline size_t nxz_dict_inflate_start(size_t len) { return len - nxz_dict_inflate_window(len); }
NXZ_DICT_HD inline size_t nxz_dict_deflate_start(size_t len) { return len - nxz_dict_deflate_window(len); }
NXZ_DICT_HD inline uint32_t nxz_dict_max_source(size_t len) { return NXZ_DICT_BLOCK - nxz_dict_deflate_window(len); }
/* a compress job the dictionary calls take: no history of its own, window + source within the block */
NXZ_DICT_HD inline bool nxz_dict_job_fits(uint32_t W, uint32_t src_len, uint32_t hist_len)
{
	return hist_len == 0 && src_len <= NXZ_DICT_BLOCK - W;
}

/* nxz_batch_decompress_dict's route, decided on the device job by job: a stream of fewer than src_min source bytes goes a wavefront
 * each, not a workgroup each.  A source that is not 16-byte aligned (framed streams behind their headers) costs the wavefront kernel
 * more, the workgroup kernel nothing: a quarter of the bound for those (profiles/r08_dict.txt). */
NXZ_DICT_HD inline bool nxz_dict_small_stream(const void *src, uint32_t src_len, uint32_t src_min)
{
	return src_len < (((uintptr_t)src & 15) ? src_min / 4 : src_min);
}

NXZ_DICT_HD inline uint32_t nxz_dict_adler32(const uint8_t *p, size_t len)
{
	uint32_t a = 1, b = 0;
	while (len) {
		size_t k = len < 5552 ? len : 5552;          /* (the sums stay below 2^32 for so many bytes) */
		len -= k;
		while (k--) { a += *p++; b += a; }
		a %= 65521u; b %= 65521u;
	}
	return b << 16 | a;
}

/* CMF << 8 | FLG of a zlib stream of `level` (-1, 0..9); fdict: the FDICT bit */
NXZ_DICT_HD inline uint32_t nxz_zlib_cmf_flg(int level, int fdict)
{
	const uint32_t flevel = level < 0 || level == 6 ? 2 : level < 2 ? 0 : level < 6 ? 1 : 3;
	uint32_t hdr = 0x78u << 8 | flevel << 6 | (fdict ? 0x20u : 0u);
	hdr += 31 - hdr % 31;
	return hdr;
}
/* the six header bytes of a stream that names a dictionary */
NXZ_DICT_HD inline void nxz_zlib_dict_header(int level, uint32_t dictid, uint8_t out[6])
{
	const uint32_t h = nxz_zlib_cmf_flg(level, 1);
	out[0] = (uint8_t)(h >> 8); out[1] = (uint8_t)h;
	out[2] = (uint8_t)(dictid >> 24); out[3] = (uint8_t)(dictid >> 16); out[4] = (uint8_t)(dictid >> 8); out[5] = (uint8_t)dictid;
}
#endif
