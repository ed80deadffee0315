// nxz_checkpoint.h -- the rules of the checkpoint calls (nxz_batch_checkpoint_index / nxz_checkpoint_read_ranges, include/nxz_engine.h)
// as plain code that compiles for the device (nxz_checkpoint.hip) and for the host (tests/native/checkpoint_host.cpp).
//
// A checkpoint is a block header of the deflate data: `bit`, the bit of the job's src where the header starts (framing included),
// and `uoff`, the bytes of output in front of it.  Everything that is not bit-walking is here:
//   the index    which headers become checkpoints (the first; then every header with span bytes or more of output behind the last
//                checkpoint), what is stored and what is only counted, the stream's record;
//   a segment    checkpoint k up to checkpoint k + 1 (entry [count] is the sentinel: the bit behind the final end-of-block code and
//                out_len): its source bytes, the unused bits of the first of them, its window, its output;
//   validity     what an index must satisfy before a kernel follows it into src or a window slot;
//   a range      onto segments: nxz_bgzf_range.h's rule over uoff (nxz_bgzf_resolve / nxz_bgzf_member_of), not restated here.
#ifndef NXZ_CHECKPOINT_H
#define NXZ_CHECKPOINT_H
#include <stdint.h>
#include "../../include/nxz_engine.h"
#include "nxz_bgzf_range.h"

#if defined(__HIPCC__)
#define NXZ_CP_HD __host__ __device__
#else
#define NXZ_CP_HD
#endif

#define NXZ_CP_WINDOW 32768u     /* bytes of a window slot */

/* ---- the index ------------------------------------------------------------------------------------------------------------- */
/* a job the index takes: fresh, no history */
NXZ_CP_HD inline bool nxz_cp_job_ok(uint32_t resume, uint32_t hist_len) { return resume == 0 && hist_len == 0; }

/* where a stream stands between two block headers */
typedef struct nxz_cp_acc {
	uint32_t count;          /* checkpoints so far, stored or not */
	uint64_t last_uoff;      /* uoff of the last of them */
} nxz_cp_acc_t;
NXZ_CP_HD inline nxz_cp_acc_t nxz_cp_begin(void)
{
	nxz_cp_acc_t a = {};
	return a;
}
/* does the header with u bytes of output in front of it become a checkpoint?  (span >= 1) */
NXZ_CP_HD inline bool nxz_cp_is_checkpoint(const nxz_cp_acc_t *a, uint64_t u, uint64_t span)
{
	return a->count == 0 || u - a->last_uoff >= span;
}
/* the header joins the index; the slot it is written to, or cp_cap when it is only counted */
NXZ_CP_HD inline uint32_t nxz_cp_add(nxz_cp_acc_t *a, uint64_t u, uint32_t cp_cap)
{
	const uint32_t k = a->count++;
	a->last_uoff = u;
	return k < cp_cap ? k : cp_cap;
}
/* the bit of the job's src for a bit the walk counts from the first byte behind hdr_len bytes of framing */
NXZ_CP_HD inline uint64_t nxz_cp_bit(uint32_t hdr_len, uint64_t walk_bit) { return 8ull * hdr_len + walk_bit; }

/* the stream's record after the walk.  frame_status: the header's (NXZ_FRAME_OK for raw); cc / final_eob: where the walk stopped
 * (nxz_size.h); have_output: the caller asked for windows and jobs[i].dst holds out_len bytes (ignored without windows) */
NXZ_CP_HD inline nxz_checkpoint_stream_t nxz_cp_summary(const nxz_cp_acc_t *a, uint32_t cp_cap, uint32_t format, uint32_t hdr_len,
							uint32_t frame_status, uint32_t cc, uint32_t final_eob, uint64_t out_len,
							bool want_windows, bool have_output)
{
	nxz_checkpoint_stream_t s = {};
	s.format = format; s.hdr_len = hdr_len; s.frame_status = frame_status;
	if (frame_status != NXZ_FRAME_OK) { s.status = NXZ_CPS_STREAM_FAILED; s.cc = NXZ_CC_INVALID_OP; return s; }
	if (cc || !final_eob) {                                            /* (count stays 0: its checkpoints are not to be used) */
		s.status = NXZ_CPS_STREAM_FAILED;
		s.cc = cc ? cc : NXZ_CC_DATA_LENGTH;
		s.frame_status = cc ? NXZ_FRAME_DEFLATE : NXZ_FRAME_TRUNCATED;
		return s;
	}
	s.count = a->count;
	s.out_len = out_len;
	s.status = a->count > cp_cap ? NXZ_CPS_MORE : (want_windows && !have_output) ? NXZ_CPS_NO_OUTPUT : NXZ_CPS_OK;
	return s;
}
/* the record of a job that was not taken: NXZ_CPS_INVALID, every other field 0 */
NXZ_CP_HD inline nxz_checkpoint_stream_t nxz_cp_refused(void)
{
	nxz_checkpoint_stream_t s = {};
	s.status = NXZ_CPS_INVALID;
	return s;
}
/* is the sentinel written?  (not when checkpoints were only counted: the index is not complete) */
NXZ_CP_HD inline bool nxz_cp_has_sentinel(uint32_t status) { return status == NXZ_CPS_OK || status == NXZ_CPS_NO_OUTPUT; }
/* are the stream's windows written?  (have_output: jobs[i].dst holds out_len bytes) */
NXZ_CP_HD inline bool nxz_cp_has_windows(uint32_t status, bool have_output) { return have_output && (status == NXZ_CPS_OK || status == NXZ_CPS_MORE); }
NXZ_CP_HD inline bool nxz_cp_have_output(const uint8_t *dst, uint32_t dst_cap, uint64_t out_len) { return dst != 0 && dst_cap >= out_len; }
/* the stored checkpoints of a stream */
NXZ_CP_HD inline uint32_t nxz_cp_stored(uint32_t count, uint32_t cp_cap) { return count < cp_cap ? count : cp_cap; }

/* ---- a segment: entries k and k + 1 of an index ---------------------------------------------------------------------------- */
NXZ_CP_HD inline uint64_t nxz_cp_src_begin(uint64_t cbit_k) { return cbit_k >> 3; }
NXZ_CP_HD inline uint64_t nxz_cp_src_end(uint64_t cbit_next) { return (cbit_next + 7) >> 3; }
/* the bits of the segment's first source byte that belong to it (the decoder's in_subc; 0: all eight) */
NXZ_CP_HD inline uint32_t nxz_cp_in_subc(uint64_t cbit_k) { return (8 - (uint32_t)(cbit_k & 7)) & 7; }
NXZ_CP_HD inline uint32_t nxz_cp_resume(uint64_t cbit_k) { return nxz_cp_in_subc(cbit_k) << 20; }
NXZ_CP_HD inline uint32_t nxz_cp_window_len(uint64_t uoff_k) { return uoff_k < NXZ_CP_WINDOW ? (uint32_t)uoff_k : NXZ_CP_WINDOW; }
NXZ_CP_HD inline uint64_t nxz_cp_out_len(uint64_t uoff_k, uint64_t uoff_next) { return uoff_next - uoff_k; }
/* [window][source bytes]: the bytes of the segment's job */
NXZ_CP_HD inline uint64_t nxz_cp_job_len(uint64_t cbit_k, uint64_t cbit_next, uint64_t uoff_k)
{
	return nxz_cp_window_len(uoff_k) + (nxz_cp_src_end(cbit_next) - nxz_cp_src_begin(cbit_k));
}

/* ---- validity -------------------------------------------------------------------------------------------------------------- */
/* Entry j against entry j + 1 of an index of L = nidx - 1 checkpoints over src_len bytes (j < L): uoff[0] is 0, cbit strictly
 * increases, uoff strictly increases over the checkpoints (the sentinel's may equal the last checkpoint's: an empty final block), nothing points
 * behind the source, and the segment's job and output fit the 32-bit fields of a job. */
NXZ_CP_HD inline bool nxz_cp_entry_ok(const uint64_t *cbit, const uint64_t *uoff, uint64_t L, uint64_t j, uint64_t src_len)
{
	const uint64_t c0 = cbit[j], c1 = cbit[j + 1], u0 = uoff[j], u1 = uoff[j + 1];
	if (src_len > (~0ull >> 3) || c1 > 8 * src_len) return false;
	if (c1 <= c0 || (j == 0 && u0 != 0)) return false;
	if (j + 1 < L ? u1 <= u0 : u1 < u0) return false;
	if (nxz_cp_job_len(c0, c1, u0) > 0xffffffffull || u1 - u0 > 0xffffffffull) return false;
	return true;
}
/* the whole index, one entry after the other (the host's form; the device checks a thread an entry) */
NXZ_CP_HD inline bool nxz_cp_index_ok(const uint64_t *cbit, const uint64_t *uoff, uint64_t nidx, uint64_t src_len)
{
	if (nidx < 2) return false;
	for (uint64_t j = 0; j + 1 < nidx; j++)
		if (!nxz_cp_entry_ok(cbit, uoff, nidx - 1, j, src_len)) return false;
	return true;
}
/* a segment decoded well: all of its output, and the decoder either ended the stream (the last segment) or ran out of source in
 * front of the next header */
NXZ_CP_HD inline bool nxz_cp_segment_good(uint32_t cc, uint32_t tpbc, uint64_t expected)
{
	return (cc == NXZ_CC_OK || cc == NXZ_CC_DATA_LENGTH) && tpbc == expected;
}

/* ---- a range onto segments: nxz_bgzf_range.h's rule over uoff ------------------------------------------------------------- */
NXZ_CP_HD inline uint32_t nxz_cp_resolve(const uint64_t *uoff, uint64_t L, uint64_t b, uint64_t e, uint64_t *ub, uint64_t *ue)
{
	return nxz_bgzf_resolve(uoff, uoff, L, NXZ_RANGE_UOFF, b, e, ub, ue);
}
NXZ_CP_HD inline uint64_t nxz_cp_segment_of(const uint64_t *uoff, uint64_t L, uint64_t u) { return nxz_bgzf_member_of(uoff, L, u); }
#endif
