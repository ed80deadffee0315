// nxz_streams_part.h -- the rules of nxz_batch_deflate_streams_part (include/nxz_engine.h: a stream written in parts, a device buffer a
// part) as plain code that compiles for the device (nxz_streams_part.hip), for the engine's host side (nxz_batch_streams.cpp) and for a
// host test program (tests/native/streams_part_host.cpp).  What is not here is nxz_streams.h's: the block plan, the header and
// trailer bytes, the checksum joins.
//
//   the first window   block 0 of a part sees the last h0 = min(H, prev_len) & ~15 bytes of `prev`, H = nxz_streams_window(hist_max): the
//                      `prev` rule of nxz_deflate_host_hist (nxz_deflate_host.cpp), as nxz_streams_dict_window restates it.  Block
//                      k >= 1 sees H bytes of its own part (B >= H: always full);
//   where it lies      in front of the source in memory when prev + prev_len == src (the job begins h0 bytes below src; src and h0
//                      are multiples of 16), else the block is STAGED: [window][the block's source bytes] in a 64 KiB slot of scratch;
//   the framing        the plain call's header with NXZ_PART_FIRST only, its trailer with NXZ_PART_LAST only;
//   the bound          nxz_streams_deflate_bound and the framing this part carries;
//   the refusals       the plain call's against this bound, and the part's own;
//   the carry          what a stream takes from call to call.
#ifndef NXZ_STREAMS_PART_H
#define NXZ_STREAMS_PART_H
#include "nxz_streams.h"

#define NXZ_PART_FLAGS (NXZ_PART_FIRST | NXZ_PART_LAST)
#define NXZ_STREAMS_STAGE_SLOT NXZ_STREAMS_SPAN   /* a staged block: window + source <= H + B */

/* ---- the first window ---- */
NXZ_STREAMS_HD inline uint32_t nxz_streams_part_window(uint32_t prev_len, uint32_t hist_max)
{
	const uint32_t H = nxz_streams_window(hist_max);
	return (prev_len < H ? prev_len : H) & ~15u;
}
/* the window of block k of a part */
NXZ_STREAMS_HD inline uint32_t nxz_streams_part_block_window(uint64_t k, uint32_t B, uint32_t H, uint32_t h0)
{
	return k ? nxz_streams_block_window(k, B, H) : h0;
}
/* is the window already in front of the source in memory? */
NXZ_STREAMS_HD inline bool nxz_streams_part_contiguous(const nxz_stream_part_job_t *j) { return (uintptr_t)j->prev + j->prev_len == (uintptr_t)j->src; }
/* does block 0 of this (accepted) part go through a staging slot? */
NXZ_STREAMS_HD inline bool nxz_streams_part_staged(const nxz_stream_part_job_t *j, uint32_t hist_max)
{
	return j->src_len != 0 && nxz_streams_part_window(j->prev_len, hist_max) != 0 && !nxz_streams_part_contiguous(j);
}

/* ---- the framing and the bound ---- */
NXZ_STREAMS_HD inline uint32_t nxz_streams_part_header_len(int fmt, uint32_t flags) { return flags & NXZ_PART_FIRST ? nxz_streams_header_len(fmt) : 0; }
NXZ_STREAMS_HD inline uint32_t nxz_streams_part_trailer_len(int fmt, uint32_t flags) { return flags & NXZ_PART_LAST ? nxz_streams_trailer_len(fmt) : 0; }
NXZ_STREAMS_HD inline uint64_t nxz_streams_part_bound(uint64_t src_len, uint32_t hist_max, int fmt, uint32_t flags)
{
	return nxz_streams_deflate_bound(src_len, hist_max) + nxz_streams_part_header_len(fmt, flags) + nxz_streams_part_trailer_len(fmt, flags);
}

/* ---- the refusals: 0, or the completion code of a part that is not taken.  carry_status: the incoming carry's (looked at without
 * FIRST only; the host, which cannot see it, passes 0 and plans the part's blocks -- the device then leaves them unused) ---- */
NXZ_STREAMS_HD inline uint32_t nxz_streams_part_refusal(const nxz_stream_part_job_t *j, uint32_t carry_status, uint32_t hist_max, int fmt)
{
	if ((!j->prev && j->prev_len) || (j->flags & ~(uint32_t)NXZ_PART_FLAGS) || ((j->flags & NXZ_PART_FIRST) && j->prev_len)) return NXZ_CC_INVALID_OP;
	if (!(j->flags & NXZ_PART_FIRST) && carry_status) return NXZ_CC_INVALID_OP;
	nxz_stream_job_t p;
	p.src = j->src; p.dst = j->dst; p.src_len = j->src_len; p.dst_cap = j->dst_cap;
	return nxz_streams_refusal_at(&p, nxz_streams_part_bound(j->src_len, hist_max, fmt, j->flags));
}

/* ---- the carry ---- */
/* what a part starts from: a fresh stream with FIRST, else what the call before left */
NXZ_STREAMS_HD inline nxz_stream_carry_t nxz_streams_part_carry_in(const nxz_stream_carry_t *c, uint32_t flags)
{
	nxz_stream_carry_t o;
	if (flags & NXZ_PART_FIRST) { o.crc = 0; o.adler = 1; o.total_in = 0; o.total_out = 0; o.parts = 0; o.status = 0; }
	else o = *c;
	return o;
}
/* ... and what it leaves: crc / adler the running values through this part */
NXZ_STREAMS_HD inline nxz_stream_carry_t nxz_streams_part_carry_out(const nxz_stream_carry_t *in, uint32_t crc, uint32_t adler, uint64_t src_len,
								    uint64_t out_len, uint32_t flags)
{
	nxz_stream_carry_t o;
	o.crc = crc; o.adler = adler;
	o.total_in = in->total_in + src_len; o.total_out = in->total_out + out_len;
	o.parts = in->parts + 1;
	o.status = flags & NXZ_PART_LAST ? 1 : 0;
	return o;
}
#endif
