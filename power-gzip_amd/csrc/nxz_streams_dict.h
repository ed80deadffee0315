// nxz_streams_dict.h -- the rules of nxz_batch_deflate_streams_dict (include/nxz_engine.h: a device buffer of any length -> one raw or
// zlib stream whose first block sees a shared preset dictionary) as plain code that compiles for the device (nxz_streams_dict.hip),
// for the engine's host side (nxz_batch_streams.cpp) and for a host test program (tests/native/streams_dict_host.cpp).  What is
// not here is nxz_streams.h's: the block plan, the trailer, the checksum joins.
//
//   the first window   block 0 sees the last h0 = min(H, len) & ~15 bytes of the dictionary, H = nxz_streams_window(hist_max): the
//                      `prev` rule of nxz_deflate_host_hist (nxz_deflate_host.cpp), NOT nxz_dict_deflate_window -- hist_max bounds
//                      it as it bounds every other block's window.  Block k >= 1 sees H bytes of its own buffer (B >= H: always full);
//   where it lies      a dictionary's device image is 32 KiB with the dictionary's end at its end (nxz_dict_create), so the window
//                      begins h0 bytes before the image's end, 16-byte aligned as h0 is;
//   the framing        raw: nothing.  zlib: the six bytes of nxz_zlib_dict_header (FDICT, DICTID of the whole dictionary) in front,
//                      the Adler-32 of the source alone behind.  gzip has no dictionary field: not taken;
//   the bound          the plain call's, and 4 more for zlib (the DICTID);
//   the launch order   where a block of a chunk stands among the chunk's compress jobs (nxz_streams_dict.hip says why).
#ifndef NXZ_STREAMS_DICT_H
#define NXZ_STREAMS_DICT_H
#include "nxz_streams.h"
#include "nxz_dict.h"

/* ---- the windows ---- */
NXZ_STREAMS_HD inline uint32_t nxz_streams_dict_window(size_t dict_len, uint32_t hist_max)
{
	const uint32_t H = nxz_streams_window(hist_max);
	return (dict_len < H ? (uint32_t)dict_len : H) & ~15u;
}
/* offset of block 0's window in the dictionary's right-aligned device image of NXZ_DICT_WINDOW bytes */
NXZ_STREAMS_HD inline uint32_t nxz_streams_dict_window_at(uint32_t h0) { return NXZ_DICT_WINDOW - h0; }
/* ... and in the dictionary's own bytes */
NXZ_STREAMS_HD inline size_t nxz_streams_dict_window_start(size_t dict_len, uint32_t hist_max) { return dict_len - nxz_streams_dict_window(dict_len, hist_max); }
/* the window of block k: the dictionary's for the first, H bytes of the buffer for every other (nxz_streams_block_window: k * B >= H) */
NXZ_STREAMS_HD inline uint32_t nxz_streams_dict_block_window(uint64_t k, uint32_t B, uint32_t H, uint32_t h0)
{
	return k ? nxz_streams_block_window(k, B, H) : h0;
}

/* ---- the launch order of a chunk: its first blocks (dictionary jobs) in front, the rest behind, each kind in the batch's order ---- */
/* the first blocks of the batch in front of block k of a stream that has nz_i streams with blocks in front of it */
NXZ_STREAMS_HD inline uint32_t nxz_streams_dict_firsts_before(uint32_t nz_i, uint64_t k) { return nz_i + (k ? 1 : 0); }
/* the place of block t of a chunk (block k of its stream) that has `before` first blocks of the chunk in front of it and nf in all */
NXZ_STREAMS_HD inline uint32_t nxz_streams_dict_launch_pos(uint32_t t, uint64_t k, uint32_t before, uint32_t nf)
{
	return k ? nf + (t - before) : before;
}

/* ---- the framing ---- */
NXZ_STREAMS_HD inline bool nxz_streams_dict_fmt_ok(int fmt) { return fmt == NXZ_FMT_RAW || fmt == NXZ_FMT_ZLIB; }
NXZ_STREAMS_HD inline uint32_t nxz_streams_dict_header_len(int fmt) { return fmt == NXZ_FMT_ZLIB ? 6 : 0; }
/* the header bytes (at most 6); returns their number */
NXZ_STREAMS_HD inline uint32_t nxz_streams_dict_header(int fmt, int level, uint32_t dictid, uint8_t out[6])
{
	if (fmt != NXZ_FMT_ZLIB) return 0;
	nxz_zlib_dict_header(level, dictid, out);
	return 6;
}

/* ---- the bound and the refusals ---- */
NXZ_STREAMS_HD inline uint64_t nxz_streams_dict_bound(uint64_t src_len, uint32_t hist_max, int fmt)
{
	return nxz_streams_bound(src_len, hist_max, fmt) + nxz_streams_dict_header_len(fmt) - nxz_streams_header_len(fmt);
}
NXZ_STREAMS_HD inline uint32_t nxz_streams_dict_refusal(const nxz_stream_job_t *j, uint32_t hist_max, int fmt)
{
	return nxz_streams_refusal_at(j, nxz_streams_dict_bound(j->src_len, hist_max, fmt));
}
#endif
