// nxz_frame.h -- zlib (RFC 1950) and gzip (RFC 1952) headers and trailers, and the BGZF member check, as plain code that
// compiles for the device (nxz_frame.hip: a wavefront per header) and for the host (tests/native/frame_host.cpp).
//
// The parser reads the header one field at a time and stops at the first fault, in zlib's order of checks
// (inflate.c: FCHECK, method, window size, then FDICT; gzip: magic, method, reserved flags, the optional
// fields, FHCRC).  A field that reaches past the source is NXZ_FRAME_TRUNCATED.  Two steps depend on who
// runs it and are passed in as `Ops`:
//   find_nul(p, from, len) -> index of the first 0 byte in [from, len), or len      (FNAME / FCOMMENT)
//   crc32(p, n)            -> CRC-32 of n bytes                                    (FHCRC)
// The device version looks at 64 bytes a step by ballot and computes the CRC in 64 slices combined by
// multiplication with x^(8k) (nxz_crc_part below); the host version runs the same 64 slices one after the other.
#ifndef NXZ_FRAME_H
#define NXZ_FRAME_H
#include <stdint.h>
#include "../../include/nxz_engine.h"

#if defined(__HIPCC__)
#define NXZ_HD __host__ __device__
#else
#define NXZ_HD
#endif

NXZ_HD inline uint32_t nxz_rd16le(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
NXZ_HD inline uint32_t nxz_rd32le(const uint8_t *p) { return nxz_rd16le(p) | nxz_rd16le(p + 2) << 16; }
NXZ_HD inline uint32_t nxz_rd32be(const uint8_t *p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

// ---- CRC-32 (reflected, polynomial 0xedb88320) in pieces --------------------------------------------------------
// the register over n bytes from 0, without the initial and final inversion
// ... one byte more
NXZ_HD inline uint32_t nxz_crc_step(uint32_t c, uint32_t byte)
{
	c ^= byte;
	for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((c & 1) ? 0xedb88320u : 0);
	return c;
}
NXZ_HD inline uint32_t nxz_crc_raw(const uint8_t *p, uint32_t n)
{
	uint32_t c = 0;
	for (uint32_t i = 0; i < n; i++) c = nxz_crc_step(c, p[i]);
	return c;
}
// a * b mod P in the reflected representation (0x80000000 = 1)
NXZ_HD inline uint32_t nxz_gf_mul(uint32_t a, uint32_t b)
{
	uint32_t r = 0;
	for (int i = 0; i < 32; i++) {
		r ^= (b & 0x80000000u) ? a : 0;
		a = (a >> 1) ^ ((a & 1) ? 0xedb88320u : 0);
		b <<= 1;
	}
	return r;
}
// x^(8 n) mod P
NXZ_HD inline uint32_t nxz_x8n(uint32_t n)
{
	uint32_t r = 0x80000000u, sq = 0x00800000u;
	while (n) { if (n & 1) r = nxz_gf_mul(r, sq); sq = nxz_gf_mul(sq, sq); n >>= 1; }
	return r;
}
// slice k of NS over n bytes: [lo, hi)
NXZ_HD inline void nxz_slice(uint32_t n, uint32_t ns, uint32_t k, uint32_t *lo, uint32_t *hi)
{
	const uint32_t per = (n + ns - 1) / ns;
	const uint64_t a = (uint64_t)k * per, b = a + per;
	*lo = a < n ? (uint32_t)a : n;
	*hi = b < n ? (uint32_t)b : n;
}
// what slice [lo, hi) of n bytes adds to the register of all n (XOR the slices' parts, then nxz_crc_finish)
NXZ_HD inline uint32_t nxz_crc_part(const uint8_t *p, uint32_t lo, uint32_t hi, uint32_t n)
{
	return lo < hi ? nxz_gf_mul(nxz_crc_raw(p + lo, hi - lo), nxz_x8n(n - hi)) : 0;
}
NXZ_HD inline uint32_t nxz_crc_finish(uint32_t parts, uint32_t n) { return ~(parts ^ nxz_gf_mul(0xffffffffu, nxz_x8n(n))); }

// ---- the header --------------------------------------------------------------------------------------------------
// The field rules, one copy for the parser below and for the byte-wise state machine of a stream read in parts (nxz_inflate_part.h).
// zlib's two bytes, in zlib's order of checks: NXZ_FRAME_OK, _BAD_HEADER (FCHECK, CINFO > 7), _BAD_METHOD or _NEED_DICT (FDICT)
NXZ_HD inline uint32_t nxz_zlib_header_status(uint32_t cmf, uint32_t flg)
{
	if ((cmf * 256 + flg) % 31) return NXZ_FRAME_BAD_HEADER;
	if ((cmf & 15) != 8) return NXZ_FRAME_BAD_METHOD;
	if ((cmf >> 4) > 7) return NXZ_FRAME_BAD_HEADER;
	return flg & 0x20 ? NXZ_FRAME_NEED_DICT : NXZ_FRAME_OK;
}
// byte i (0 .. 3) of a gzip header: ID1, ID2, CM, FLG
NXZ_HD inline uint32_t nxz_gzip_fixed_status(uint32_t i, uint32_t byte)
{
	return i == 0 ? (byte != 0x1f ? NXZ_FRAME_BAD_HEADER : NXZ_FRAME_OK) : i == 1 ? (byte != 0x8b ? NXZ_FRAME_BAD_HEADER : NXZ_FRAME_OK)
	     : i == 2 ? (byte != 8 ? NXZ_FRAME_BAD_METHOD : NXZ_FRAME_OK) : ((byte & 0xe0) ? NXZ_FRAME_BAD_HEADER : NXZ_FRAME_OK);
}
// is this the gzip magic? (NXZ_FMT_AUTO)
NXZ_HD inline bool nxz_gzip_magic(uint32_t b0, uint32_t b1) { return b0 == 0x1f && b1 == 0x8b; }

// Fills f (status, format, hdr_len and the header's fields; end / check / isize are the trailer's, left 0) and
// returns the status.  fmt: NXZ_FMT_ZLIB / _GZIP / _AUTO.
template <class Ops>
NXZ_HD inline uint32_t nxz_frame_parse(const uint8_t *p, uint32_t len, int fmt, nxz_batch_frame_t *f, Ops &ops)
{
	*f = nxz_batch_frame_t();
	const bool gz = fmt == NXZ_FMT_GZIP || (fmt == NXZ_FMT_AUTO && len >= 2 && nxz_gzip_magic(p[0], p[1]));
	f->format = gz ? NXZ_FMT_GZIP : NXZ_FMT_ZLIB;
	uint32_t st = NXZ_FRAME_OK;
	if (!gz) {
		if (len < 2) st = NXZ_FRAME_TRUNCATED;
		else {
			const uint32_t cmf = p[0], flg = p[1];
			f->flg = (uint8_t)flg; f->cinfo = (uint8_t)(cmf >> 4);
			st = nxz_zlib_header_status(cmf, flg);
			if (st == NXZ_FRAME_NEED_DICT) {
				if (len < 6) st = NXZ_FRAME_TRUNCATED;
				else { f->dictid = nxz_rd32be(p + 2); f->hdr_len = 6; }
			} else if (st == NXZ_FRAME_OK) f->hdr_len = 2;
		}
		f->status = st;
		return st;
	}
	uint32_t q = 10;
	if (len < 1) st = NXZ_FRAME_TRUNCATED;
	else if ((st = nxz_gzip_fixed_status(0, p[0])) != NXZ_FRAME_OK) ;
	else if (len < 2) st = NXZ_FRAME_TRUNCATED;
	else if ((st = nxz_gzip_fixed_status(1, p[1])) != NXZ_FRAME_OK) ;
	else if (len < 3) st = NXZ_FRAME_TRUNCATED;
	else if ((st = nxz_gzip_fixed_status(2, p[2])) != NXZ_FRAME_OK) ;
	else if (len < 4) st = NXZ_FRAME_TRUNCATED;
	else if ((st = nxz_gzip_fixed_status(3, f->flg = p[3])) != NXZ_FRAME_OK) ;
	else if (len < 10) st = NXZ_FRAME_TRUNCATED;
	else {
		const uint32_t flg = p[3];
		f->mtime = nxz_rd32le(p + 4); f->xfl = p[8]; f->os = p[9];
		if (flg & 4) {
			if (len < q + 2) st = NXZ_FRAME_TRUNCATED;
			else {
				f->extra_len = nxz_rd16le(p + q);
				f->extra_off = q + 2;
				q += 2 + f->extra_len;
				if (q > len) st = NXZ_FRAME_TRUNCATED;
			}
		}
		if (st == NXZ_FRAME_OK && (flg & 8)) {
			f->name_off = q;
			const uint32_t z = q < len ? ops.find_nul(p, q, len) : len;
			if (z >= len) st = NXZ_FRAME_TRUNCATED; else q = z + 1;
		}
		if (st == NXZ_FRAME_OK && (flg & 16)) {
			f->comment_off = q;
			const uint32_t z = q < len ? ops.find_nul(p, q, len) : len;
			if (z >= len) st = NXZ_FRAME_TRUNCATED; else q = z + 1;
		}
		if (st == NXZ_FRAME_OK && (flg & 2)) {
			if (len < q + 2) st = NXZ_FRAME_TRUNCATED;
			else {
				if ((ops.crc32(p, q) & 0xffff) != nxz_rd16le(p + q)) st = NXZ_FRAME_BAD_HCRC;
				q += 2;
			}
		}
		if (st == NXZ_FRAME_OK) f->hdr_len = q;
	}
	f->status = st;
	return st;
}

// The same for a caller that holds a preset dictionary (nxz_batch_decompress_framed_dict): a zlib header with FDICT whose
// DICTID is the dictionary's is no fault -- the deflate data starts behind the six bytes and may refer to the dictionary
// (*use_dict = true).  Any other DICTID, or no dictionary (have_dict false), stays NXZ_FRAME_NEED_DICT; a zlib stream
// without FDICT and every gzip stream is decoded without the dictionary, as zlib does.
template <class Ops>
NXZ_HD inline uint32_t nxz_frame_parse_dict(const uint8_t *p, uint32_t len, int fmt, nxz_batch_frame_t *f, Ops &ops,
					    bool have_dict, uint32_t dictid, bool *use_dict)
{
	uint32_t st = nxz_frame_parse(p, len, fmt, f, ops);
	*use_dict = false;
	if (st == NXZ_FRAME_NEED_DICT && have_dict && f->dictid == dictid) {
		st = NXZ_FRAME_OK;
		f->status = st;
		*use_dict = true;
	}
	return st;
}

// ---- the trailer -------------------------------------------------------------------------------------------------
NXZ_HD inline uint32_t nxz_frame_trailer_bytes(uint32_t format) { return format == NXZ_FMT_GZIP ? 8u : 4u; }

// What stands behind the deflate data of a job whose header parsed (format, hdr_len) and whose deflate data gave r -- a decode's
// result, or the size walk's.  The first byte behind the final block is hdr_len + spbc - subc / 8 on every route
// (oracle/nxz_inflate.c: spbc = the source bytes taken, subc = the bits left behind the final end-of-block); the trailer is read
// from there a byte at a time.  Returns the status; *end, *check and *isize are the frame's fields, 0 unless the trailer was read.
// compare_check: hold Adler-32 / CRC-32 against r's (the walk has none to compare: without it nothing is NXZ_FRAME_BAD_CHECK).
// gzip's ISIZE is held against r->tpbc either way.
// the trailer's bytes t against the output's checksums and length: *check and *isize as read, the verdict
NXZ_HD inline uint32_t nxz_frame_trailer_status(uint32_t format, const uint8_t *t, uint32_t crc, uint32_t adler, uint32_t out_len, bool compare_check,
						uint32_t *check, uint32_t *isize)
{
	if (format != NXZ_FMT_GZIP) {
		*check = nxz_rd32be(t); *isize = 0;
		return compare_check && *check != adler ? NXZ_FRAME_BAD_CHECK : NXZ_FRAME_OK;
	}
	*check = nxz_rd32le(t); *isize = nxz_rd32le(t + 4);
	return compare_check && *check != crc ? NXZ_FRAME_BAD_CHECK : *isize != out_len ? NXZ_FRAME_BAD_LENGTH : NXZ_FRAME_OK;
}
NXZ_HD inline uint32_t nxz_frame_trailer(uint32_t format, uint32_t hdr_len, const nxz_batch_result_t *r, const uint8_t *src, uint32_t src_len,
					 bool compare_check, uint32_t *end, uint32_t *check, uint32_t *isize)
{
	*end = *check = *isize = 0;
	if (!(r->sfbt & 0x100) || (r->cc != NXZ_CC_OK && r->cc != NXZ_CC_DATA_LENGTH))
		return r->cc == NXZ_CC_DATA_LENGTH ? NXZ_FRAME_TRUNCATED : NXZ_FRAME_DEFLATE;   // (the source ran out before the final block ended)
	const uint32_t tl = nxz_frame_trailer_bytes(format);
	const uint64_t dend = (uint64_t)hdr_len + r->spbc - (r->subc >> 3);
	if (dend + tl > src_len) return NXZ_FRAME_TRUNCATED;
	*end = (uint32_t)dend + tl;
	return nxz_frame_trailer_status(format, src + dend, r->crc, r->adler, r->tpbc, compare_check, check, isize);
}

// ---- BGZF: one member with the "BC" subfield at p (left bytes from there on) -------------------------------------
// Its total size (BSIZE + 1), or 0.  The checks of the host's scanner (nxz_blocked.cpp member_size): FLG = FEXTRA
// alone, XLEN >= 6, the subfield anywhere among the others, the size covers header and trailer and lies inside `left`.
NXZ_HD inline uint32_t nxz_bgzf_member_size(const uint8_t *p, uint64_t left)
{
	if (left < 12 + 6 + 8 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || p[3] != 4) return 0;
	const uint32_t xlen = nxz_rd16le(p + 10);
	if (xlen < 6 || 12 + (uint64_t)xlen + 8 > left) return 0;
	for (uint32_t q = 0; q + 4 <= xlen;) {
		const uint8_t *s = p + 12 + q;
		const uint32_t slen = nxz_rd16le(s + 2);
		if (s[0] == 'B' && s[1] == 'C' && slen == 2 && q + 6 <= xlen) {
			const uint32_t size = nxz_rd16le(s + 4) + 1;
			return size >= 12 + xlen + 8 && size <= left ? size : 0;
		}
		q += 4 + slen;
	}
	return 0;
}

#endif
