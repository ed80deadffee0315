// nxz_streams_index.h -- the rules of nxz_batch_deflate_streams_indexed (include/nxz_engine.h: nxz_batch_deflate_streams that writes the
// checkpoint index of its streams while it lays them out) as plain code that compiles for the device (nxz_streams_index.hip) and for
// a host test program (tests/native/streams_index_host.cpp).  The index is the one nxz_batch_checkpoint_index would find by walking
// the finished stream (nxz_checkpoint.h has its rules); nothing is walked here, because the layout knows every block header:
//
//   a piece        is what one block of the plan occupies in its stream (stream_piece, nxz_pack_block.h): laid at byte P, with
//                  u0 = k * B bytes of output in front of it.  One compress job writes ONE deflate block (nxz_encode.hip: one
//                  header, the symbols, one end-of-block code), so a piece holds at most two block headers:
//                    compressed   its own at (8 P, u0); with a marker (!final && tebc != 0) the empty stored block's at
//                                 (8 (P + keep - 1) + tebc, u0 + len) -- inside a byte;
//                    stored       its own at (8 P, u0); with len > 65535 the second stored block's at (8 (P + 5 + 65535), u0 + 65535);
//   the sentinel   the bit behind the final piece's end-of-block code: 8 (P + keep - 1) + (tebc ? tebc : 8) for a compressed
//                  piece, the piece's end for a stored one; uoff = src_len;
//   an empty buffer has no piece: its one header (01 00 00 ff ff) stands at 8 * hdr_len, the sentinel 40 bits further, both at uoff 0;
//   rule 2         the headers in stream order, c = the uoff of the last checkpoint (0 behind checkpoint 0, which is the first header):
//                  a header is a checkpoint when u - c >= span, and then c = u.  A marker and the next piece's header have the same
//                  u: the first of them in the stream is taken.
#ifndef NXZ_STREAMS_INDEX_H
#define NXZ_STREAMS_INDEX_H
#include <stdint.h>
#include "nxz_streams.h"
#include "nxz_checkpoint.h"

#define NXZ_SI_NONE 0xffffffffu         /* a header that got no window slot */
#define NXZ_SI_STORED_FIRST 65535u      /* source bytes of the first stored block of a stored piece */

/* a piece as the layout sees it: stream_piece's fields and the job's tebc */
typedef struct nxz_si_piece {
	uint32_t stored, len, keep, tebc, final;
} nxz_si_piece_t;

/* the bytes a piece occupies in its stream (stream_piece's size) */
NXZ_STREAMS_HD inline uint32_t nxz_si_piece_size(const nxz_si_piece_t *p)
{
	if (p->stored) return p->len > NXZ_SI_STORED_FIRST ? p->len + 10 : p->len + 5;
	const bool marker = !p->final && p->tebc != 0;
	return p->keep + (marker ? (p->tebc + 3 > 8 ? 1u : 0u) + 4 : 0);
}
/* the block headers of a piece laid at byte P with u0 bytes of output in front of it, in stream order; returns 1 or 2 */
NXZ_STREAMS_HD inline uint32_t nxz_si_headers(const nxz_si_piece_t *p, uint64_t P, uint64_t u0, uint64_t bit[2], uint64_t u[2])
{
	bit[0] = 8 * P; u[0] = u0;
	bit[1] = 0; u[1] = 0;
	if (p->stored) {
		if (p->len <= NXZ_SI_STORED_FIRST) return 1;
		bit[1] = 8 * (P + 5 + NXZ_SI_STORED_FIRST); u[1] = u0 + NXZ_SI_STORED_FIRST;
		return 2;
	}
	if (p->final || p->tebc == 0) return 1;
	bit[1] = 8 * (P + p->keep - 1) + p->tebc; u[1] = u0 + p->len;
	return 2;
}
/* the bit behind the end-of-block code of a piece laid at byte P (the sentinel's, for the final piece) */
NXZ_STREAMS_HD inline uint64_t nxz_si_end_bit(const nxz_si_piece_t *p, uint64_t P)
{
	if (p->stored) return 8 * (P + nxz_si_piece_size(p));
	return 8 * (P + p->keep - 1) + (p->tebc ? p->tebc : 8);
}
/* an empty buffer: its header stands where checkpoint 0 always stands, its sentinel behind the five bytes of the empty stored block */
NXZ_STREAMS_HD inline uint64_t nxz_si_first_bit(uint32_t hdr_len) { return 8ull * hdr_len; }
NXZ_STREAMS_HD inline uint64_t nxz_si_empty_end_bit(uint32_t hdr_len) { return 8ull * hdr_len + 8 * NXZ_STREAMS_EMPTY_LEN; }

/* rule 2 behind checkpoint 0: does the header at u become a checkpoint when the last one stands at c?  (u < c: a header in front of
 * the last checkpoint, which a wavefront that looks at 64 pieces at once still has before it) */
NXZ_STREAMS_HD inline bool nxz_si_takes(uint64_t u, uint64_t c, uint64_t span) { return u > c && u - c >= span; }

/* a stream the index format has room for: jobs of the index calls carry 32-bit lengths */
NXZ_STREAMS_HD inline bool nxz_si_len_ok(uint64_t len) { return len <= 0xffffffffull; }
/* the call's arrays: n * (cp_cap + 1) entries, indexed by 32 bits */
NXZ_STREAMS_HD inline bool nxz_si_shape_ok(uint64_t n, uint32_t cp_cap) { return n < (1ull << 31) && n * ((uint64_t)cp_cap + 1) < (1ull << 32); }

/* the record of a stream that gets no index: NXZ_CPS_INVALID with the compress side's code, every other field 0 */
NXZ_STREAMS_HD inline nxz_checkpoint_stream_t nxz_si_no_index(uint32_t cc)
{
	nxz_checkpoint_stream_t s = nxz_cp_refused();
	s.cc = cc;
	return s;
}
/* the record of an indexed stream: what nxz_cp_summary says of a walk that reached the final end-of-block code */
NXZ_STREAMS_HD inline nxz_checkpoint_stream_t nxz_si_summary(uint32_t count, uint32_t cp_cap, int fmt, uint64_t src_len)
{
	nxz_cp_acc_t a = nxz_cp_begin();
	a.count = count;
	return nxz_cp_summary(&a, cp_cap, (uint32_t)fmt, nxz_streams_header_len(fmt), NXZ_FRAME_OK, 0, 1, src_len, false, true);
}
/* the job the readers want for stream i: src = the stream (NULL without an index), in_adler = 1, every other field 0 */
NXZ_STREAMS_HD inline nxz_batch_job_t nxz_si_reader_job(const uint8_t *stream, uint64_t out_len, bool indexed)
{
	nxz_batch_job_t j = {};
	j.in_adler = 1;
	if (indexed) { j.src = stream; j.src_len = (uint32_t)out_len; }
	return j;
}
#endif
