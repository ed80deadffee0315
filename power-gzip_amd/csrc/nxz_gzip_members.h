// nxz_gzip_members.h -- the rules of the multi-member gzip calls (nxz_batch_gzip_members_size / _decode, include/nxz_engine.h) as
// plain code that compiles for the device (nxz_gzip_members.hip) and for the host (tests/native/gzip_members_host.cpp).
//
// Every decision that is not bit-walking is here, so that the kernels and a host program run the same code:
//   the walk    which jobs are taken, what a member's record says after its header, its deflate data and its trailer, how the
//               running sums (members, uoff, consumed, out_len) move, whether another member follows, the job's summary;
//   the decode  which jobs are expanded, how many of their members, whether a record points inside its job, and the summary
//               after the decode's verdicts are joined back.
#ifndef NXZ_GZIP_MEMBERS_H
#define NXZ_GZIP_MEMBERS_H
#include <stdint.h>
#include "../../include/nxz_engine.h"

#if defined(__HIPCC__)
#define NXZ_GZM_HD __host__ __device__
#else
#define NXZ_GZM_HD
#endif

#define NXZ_GZM_TRAILER 8u       /* CRC-32 and ISIZE */

/* ---- the walk -------------------------------------------------------------------------------------------------------------- */
/* a job the calls take: fresh, no history (rule 1) */
NXZ_GZM_HD inline bool nxz_gzm_job_ok(uint32_t resume, uint32_t hist_len) { return resume == 0 && hist_len == 0; }

/* where a job stands between two members */
typedef struct nxz_gzm_acc {
	uint32_t members, failed, consumed, cc, any_failed;
	uint64_t out_len;
} nxz_gzm_acc_t;
NXZ_GZM_HD inline nxz_gzm_acc_t nxz_gzm_begin(void)
{
	nxz_gzm_acc_t a = {};
	return a;
}

/* the record of the member that starts at `coff` behind `uoff` bytes of output, before anything of it was read */
NXZ_GZM_HD inline nxz_gzip_member_t nxz_gzm_member(uint64_t uoff, uint32_t coff)
{
	nxz_gzip_member_t m = {};
	m.uoff = uoff; m.coff = coff;
	return m;
}
/* behind a header of hdr_len bytes (read whole: hdr_len <= left) there is room for a trailer -- else the member is TRUNCATED, as
 * the header kernel of the framed calls says; the deflate data then has left - hdr_len - 8 bytes to end in */
NXZ_GZM_HD inline bool nxz_gzm_room(uint32_t left, uint32_t hdr_len) { return left - hdr_len >= NXZ_GZM_TRAILER; }
/* what the size walk's stop means for the member (nxz_size.h: cc, and final_eob when it stands behind the final end-of-block) */
NXZ_GZM_HD inline uint32_t nxz_gzm_walk_status(uint32_t cc, uint32_t final_eob)
{
	return cc ? NXZ_FRAME_DEFLATE : final_eob ? NXZ_FRAME_OK : NXZ_FRAME_TRUNCATED;
}
/* ... and the raw decoder's code that goes with it */
NXZ_GZM_HD inline uint32_t nxz_gzm_walk_cc(uint32_t cc, uint32_t final_eob) { return cc ? cc : final_eob ? NXZ_CC_OK : NXZ_CC_DATA_LENGTH; }
/* the trailer, read at byte `dend` of the member (header and deflate bytes in front of it): the status */
NXZ_GZM_HD inline uint32_t nxz_gzm_trailer(nxz_gzip_member_t *m, uint32_t dend, uint32_t check, uint32_t isize_read, uint32_t counted)
{
	m->clen = dend + NXZ_GZM_TRAILER;
	m->check = check;
	m->isize = counted;
	return isize_read == counted ? NXZ_FRAME_OK : NXZ_FRAME_BAD_LENGTH;
}
/* is the member stored?  (rule 5: those beyond member_cap are counted only) */
NXZ_GZM_HD inline bool nxz_gzm_stored(const nxz_gzm_acc_t *a, uint32_t member_cap) { return a->members < member_cap; }
/* the finished member joins the sums; false: it failed and the walk ends (rule 4) */
NXZ_GZM_HD inline bool nxz_gzm_add(nxz_gzm_acc_t *a, const nxz_gzip_member_t *m, uint32_t cc)
{
	const uint32_t idx = a->members++;
	if (m->status != NXZ_FRAME_OK) {
		a->failed = idx; a->any_failed = 1; a->cc = cc;
		return false;
	}
	a->failed = a->members;
	a->out_len += m->isize;
	a->consumed = m->coff + m->clen;
	return true;
}
/* does another member start at byte e, where an OK member ended?  (rule 3) */
NXZ_GZM_HD inline bool nxz_gzm_more(const uint8_t *src, uint32_t src_len, uint32_t e)
{
	return e < src_len && src_len - e >= 2 && src[e] == 0x1f && src[e + 1] == 0x8b;
}
NXZ_GZM_HD inline nxz_gzip_stream_t nxz_gzm_summary(const nxz_gzm_acc_t *a, uint32_t member_cap)
{
	nxz_gzip_stream_t s = {};
	s.status = a->any_failed ? NXZ_GZS_MEMBER_FAILED : a->members > member_cap ? NXZ_GZS_MORE_MEMBERS : NXZ_GZS_OK;
	s.members = a->members; s.failed = a->failed; s.consumed = a->consumed; s.out_len = a->out_len; s.cc = a->cc;
	return s;
}
/* the summary of a job that was not taken: NXZ_GZS_INVALID, every other field 0 */
NXZ_GZM_HD inline nxz_gzip_stream_t nxz_gzm_refused(void)
{
	nxz_gzip_stream_t s = {};
	s.status = NXZ_GZS_INVALID;
	return s;
}

/* ---- the decode ------------------------------------------------------------------------------------------------------------ */
/* a summary whose members the decode may expand */
NXZ_GZM_HD inline bool nxz_gzm_decodable(uint32_t status)
{
	return status == NXZ_GZS_OK || status == NXZ_GZS_MEMBER_FAILED || status == NXZ_GZS_MORE_MEMBERS;
}
/* the stored OK members of a job: the first min(failed, member_cap) */
NXZ_GZM_HD inline uint32_t nxz_gzm_stored_ok(uint32_t failed, uint32_t member_cap) { return failed < member_cap ? failed : member_cap; }
/* a record the decode may follow: an OK member that lies inside its job's source and target */
NXZ_GZM_HD inline bool nxz_gzm_record_inside(const nxz_gzip_member_t *m, uint32_t src_len, uint32_t dst_cap)
{
	return m->status == NXZ_FRAME_OK && (uint64_t)m->coff + m->clen <= src_len && m->uoff <= dst_cap && m->uoff + m->isize <= dst_cap;
}
/* What the job says before anything is decoded.  stale: one of its stored OK records failed nxz_gzm_record_inside; base: the
 * members of the jobs in front of it; total_members: the caller's bound.  *count: the members of this job that are decoded. */
NXZ_GZM_HD inline uint32_t nxz_gzm_plan(uint32_t status, uint64_t out_len, uint32_t failed, uint32_t member_cap, uint32_t dst_cap,
					bool stale, uint64_t base, uint64_t total_members, uint32_t *count)
{
	*count = 0;
	if (!nxz_gzm_decodable(status)) return NXZ_GZS_INVALID;             /* (a summary this call refused before: the size pass again) */
	if (out_len > dst_cap) return NXZ_GZS_TARGET_SPACE;
	if (stale || base + nxz_gzm_stored_ok(failed, member_cap) > total_members) return NXZ_GZS_INVALID;
	*count = nxz_gzm_stored_ok(failed, member_cap);
	return status;
}
/* The summary after the decode of a job that was expanded.  first_bad: the lowest index among its decoded members whose frame status
 * is not OK (0xffffffff: none), bad_cc: that member's raw code, decoded: the bytes of those that are OK. */
NXZ_GZM_HD inline void nxz_gzm_join(nxz_gzip_stream_t *s, uint32_t first_bad, uint32_t bad_cc, uint64_t decoded)
{
	s->out_len = decoded;
	if (first_bad != 0xffffffffu) { s->status = NXZ_GZS_MEMBER_FAILED; s->failed = first_bad; s->cc = bad_cc; }
}
#endif
