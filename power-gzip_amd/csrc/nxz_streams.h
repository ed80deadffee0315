// nxz_streams.h -- the rules of nxz_batch_deflate_streams (include/nxz_engine.h: a device buffer of any length -> one raw, zlib or
// gzip stream) as plain code that compiles for the device (nxz_streams.hip), for the engine's host side (nxz_batch_streams.cpp) and for a
// host test program (tests/native/streams_host.cpp).
//
//   the block plan   a buffer is cut as nxz_deflate_host_hist cuts it: with a window of H = min(hist_max & ~15, 32768) bytes a
//                    block carries B = 65536 - H source bytes, block k starts at k * B and sees the min(H, k * B) bytes of the same
//                    buffer in front of it (a multiple of 16: H and B are).  A buffer of length 0 has no block;
//   the bound        nxz_deflate_host_bound_hist (src_len + 10 a block + 16) and the framing;
//   the framing      the header in front of the deflate data and the trailer behind it, per format;
//   the two joins    CRC-32 and Adler-32 of a buffer from those of its parts (the host forms are gf2_mul32 / crc_shift_op / adler_join
//                    in nxz_deflate_host.cpp; zlib's crc32_combine / adler32_combine do the same).
#ifndef NXZ_STREAMS_H
#define NXZ_STREAMS_H
#include <stdint.h>
#include <stddef.h>
#include "../../include/nxz_engine.h"

#if defined(__HIPCC__)
#define NXZ_STREAMS_HD __host__ __device__
#else
#define NXZ_STREAMS_HD
#endif

#define NXZ_STREAMS_SPAN 65536u          /* window + source of one compress job */
#define NXZ_STREAMS_SLOT 73856u          /* room for one block's output between the compress and the pack step (nxz_compress_bound(65536) rounded) */
#define NXZ_STREAMS_CHUNK_DEFAULT 4096u  /* blocks per chunk when NXZ_STREAMS_CHUNK is not set (profiles/r11_streams.txt: 94.6 GiB/s; 1024: 75.0, 16384: 99.5) */

/* ---- the block plan ---- */
NXZ_STREAMS_HD inline uint32_t nxz_streams_window(uint32_t hist_max) { return hist_max > 32768u ? 32768u : hist_max & ~15u; }
NXZ_STREAMS_HD inline uint32_t nxz_streams_block_bytes(uint32_t hist_max) { return NXZ_STREAMS_SPAN - nxz_streams_window(hist_max); }
NXZ_STREAMS_HD inline uint64_t nxz_streams_blocks(uint64_t src_len, uint32_t B) { return src_len / B + (src_len % B ? 1 : 0); }
NXZ_STREAMS_HD inline uint64_t nxz_streams_block_start(uint64_t k, uint32_t B) { return k * B; }
NXZ_STREAMS_HD inline uint32_t nxz_streams_block_len(uint64_t src_len, uint64_t k, uint32_t B)
{
	const uint64_t rest = src_len - k * B;
	return rest < B ? (uint32_t)rest : B;
}
NXZ_STREAMS_HD inline uint32_t nxz_streams_block_window(uint64_t k, uint32_t B, uint32_t H)
{
	const uint64_t front = k * B;
	return front < H ? (uint32_t)front : H;
}

/* ---- the framing ---- */
NXZ_STREAMS_HD inline bool nxz_streams_fmt_ok(int fmt) { return fmt == NXZ_FMT_RAW || fmt == NXZ_FMT_ZLIB || fmt == NXZ_FMT_GZIP; }
NXZ_STREAMS_HD inline uint32_t nxz_streams_header_len(int fmt) { return fmt == NXZ_FMT_ZLIB ? 2 : fmt == NXZ_FMT_GZIP ? 10 : 0; }
NXZ_STREAMS_HD inline uint32_t nxz_streams_trailer_len(int fmt) { return fmt == NXZ_FMT_ZLIB ? 4 : fmt == NXZ_FMT_GZIP ? 8 : 0; }
/* FLEVEL as zlib's deflate.c writes it (nxz_batch_pack_zlib): 0 for levels 0-1, 1 for 2-5, 2 for 6 and -1, 3 for 7-9 */
NXZ_STREAMS_HD inline uint32_t nxz_streams_zlib_flg(int level)
{
	const uint32_t flevel = level < 0 || level == 6 ? 2 : level < 2 ? 0 : level < 6 ? 1 : 3;
	uint32_t hdr = 0x78u << 8 | flevel << 6;
	hdr += 31 - hdr % 31;
	return hdr & 0xff;
}
/* the header bytes (at most 10); returns their number */
NXZ_STREAMS_HD inline uint32_t nxz_streams_header(int fmt, int level, uint8_t out[10])
{
	if (fmt == NXZ_FMT_ZLIB) {
		out[0] = 0x78; out[1] = (uint8_t)nxz_streams_zlib_flg(level);
		return 2;
	}
	if (fmt == NXZ_FMT_GZIP) {                     /* ID1 ID2 CM FLG=0 MTIME=0 XFL=4 OS=3, as the stream layer writes it */
		out[0] = 0x1f; out[1] = 0x8b; out[2] = 8; out[3] = 0; out[4] = 0; out[5] = 0; out[6] = 0; out[7] = 0; out[8] = 4; out[9] = 3;
		return 10;
	}
	return 0;
}
/* the trailer bytes (at most 8); returns their number.  zlib: Adler-32 big-endian; gzip: CRC-32, ISIZE = src_len mod 2^32, little-endian */
NXZ_STREAMS_HD inline uint32_t nxz_streams_trailer(int fmt, uint32_t crc, uint32_t adler, uint64_t src_len, uint8_t out[8])
{
	if (fmt == NXZ_FMT_ZLIB) {
		for (int k = 0; k < 4; k++) out[k] = (uint8_t)(adler >> (8 * (3 - k)));
		return 4;
	}
	if (fmt == NXZ_FMT_GZIP) {
		const uint32_t isize = (uint32_t)src_len;
		for (int k = 0; k < 4; k++) { out[k] = (uint8_t)(crc >> (8 * k)); out[4 + k] = (uint8_t)(isize >> (8 * k)); }
		return 8;
	}
	return 0;
}
/* the deflate data of a buffer of length 0: one empty stored block with BFINAL */
#define NXZ_STREAMS_EMPTY_LEN 5u
NXZ_STREAMS_HD inline void nxz_streams_empty(uint8_t out[5]) { out[0] = 1; out[1] = 0; out[2] = 0; out[3] = 0xff; out[4] = 0xff; }

/* ---- the bound ---- */
NXZ_STREAMS_HD inline uint64_t nxz_streams_deflate_bound(uint64_t src_len, uint32_t hist_max)
{
	return src_len + nxz_streams_blocks(src_len, nxz_streams_block_bytes(hist_max)) * 10 + 16;
}
NXZ_STREAMS_HD inline uint64_t nxz_streams_bound(uint64_t src_len, uint32_t hist_max, int fmt)
{
	return nxz_streams_deflate_bound(src_len, hist_max) + nxz_streams_header_len(fmt) + nxz_streams_trailer_len(fmt);
}

/* ---- refusals: 0, or the completion code of a stream that is not taken (its dst stays untouched, it gets no blocks) ---- */
/* ... against a bound the caller has worked out (nxz_streams_dict.h has another) */
NXZ_STREAMS_HD inline uint32_t nxz_streams_refusal_at(const nxz_stream_job_t *j, uint64_t bound)
{
	if ((!j->src && j->src_len) || ((uintptr_t)j->src & 15) || !j->dst) return NXZ_CC_INVALID_OP;
	if (j->dst_cap < bound) return NXZ_CC_TARGET_SPACE;
	return 0;
}
NXZ_STREAMS_HD inline uint32_t nxz_streams_refusal(const nxz_stream_job_t *j, uint32_t hist_max, int fmt)
{
	return nxz_streams_refusal_at(j, nxz_streams_bound(j->src_len, hist_max, fmt));
}

/* ---- CRC-32 of [a][b] from those of a and b ---- */
/* a * b mod P in GF(2)[x], reflected (bit 31 = x^0), P = the CRC-32 polynomial */
NXZ_STREAMS_HD inline uint32_t nxz_gf2_mul32(uint32_t a, uint32_t b)
{
	uint32_t p = 0;
	for (uint32_t m = 0x80000000u; m; m >>= 1) {
		if (a & m) p ^= b;
		b = (b >> 1) ^ ((b & 1) ? 0xedb88320u : 0);
	}
	return p;
}
/* base^e by square-and-multiply (1 is 0x80000000) */
NXZ_STREAMS_HD inline uint32_t nxz_gf2_pow32(uint32_t base, uint64_t e)
{
	uint32_t r = 0x80000000u;
	for (; e; e >>= 1) { if (e & 1) r = nxz_gf2_mul32(r, base); base = nxz_gf2_mul32(base, base); }
	return r;
}
/* the operator of `nbytes` bytes: x^(8 nbytes) mod P (x^8 is 0x00800000) */
NXZ_STREAMS_HD inline uint32_t nxz_crc_shift_op(uint64_t nbytes) { return nxz_gf2_pow32(0x00800000u, nbytes); }
/* crc of [a][b]: crc_a moved over b's bytes (op = nxz_crc_shift_op(len_b), or a product of such), then crc_b */
NXZ_STREAMS_HD inline uint32_t nxz_crc_join(uint32_t crc_a, uint32_t crc_b, uint32_t op) { return nxz_gf2_mul32(crc_a, op) ^ crc_b; }
/* the operator of `full` blocks of B bytes each (op_block = nxz_crc_shift_op(B), made once) and `tail` bytes more
 * (always inlined: left as a call it costs the layout kernels, its one user on the device, the eighth wavefront a SIMD) */
NXZ_STREAMS_HD inline __attribute__((always_inline)) uint32_t nxz_crc_blocks_op(uint32_t op_block, uint64_t full, uint32_t tail)
{
	const uint32_t f = nxz_gf2_pow32(op_block, full);
	return tail ? nxz_gf2_mul32(f, nxz_crc_shift_op(tail)) : f;
}

/* ---- Adler-32 of [a][b] from those of a and b (both from 1) and b's length ---- */
#define NXZ_ADLER_BASE 65521u
NXZ_STREAMS_HD inline uint32_t nxz_adler_join(uint32_t a1, uint32_t a2, uint64_t len2)
{
	const uint64_t M = NXZ_ADLER_BASE, rem = len2 % M, s1 = a1 & 0xffff;
	const uint64_t sum1 = (s1 + (a2 & 0xffff) + M - 1) % M;
	const uint64_t sum2 = (rem * s1 + (a1 >> 16) + (a2 >> 16) + M - rem) % M;
	return (uint32_t)((sum2 << 16) | sum1);
}
#endif
