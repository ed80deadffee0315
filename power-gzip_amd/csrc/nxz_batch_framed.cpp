// nxz_batch_framed.cpp -- the calls of include/nxz_engine.h's device-resident interface that put kernels of their own around a raw
// batch (nxz_batch.cpp) or walk streams without decoding them: framed zlib / gzip streams, output sizes, verify, multi-member gzip
// jobs.  (One stream per device buffer is nxz_batch_streams.cpp's; BGZF, the checkpoint index and every range read nxz_batch_ranges.cpp's.)
#include "nxz_ctx.h"

// ---------------------------------------------------------------------------
// Framed streams (nxz_frame.hip): header kernel -> the raw batch on the derived jobs -> trailer kernel, all on `s`.
// The caller holds c->frame_use[s].
// ---------------------------------------------------------------------------
// The header kernel (with the dictionary's DICTID when there is one) into frames and *derived, the raw jobs in BUF_FRAME_JOBS of `s`.
// (the caller's frame_use[s] guards the derived jobs: no lease here, the raw batch takes its own)
static int derive_framed_jobs(nxz_ctx_t *c, int fmt, const nxz_dict *dict, const nxz_batch_job_t *jobs, size_t n, nxz_batch_frame_t *frames,
			      hipStream_t s, nxz_batch_job_t **derived)
{
	nxz_batch_job_t *const d = *derived = with_scratch(c, s, [&](nxz_ctx::Scratch &sc) {
		(void)sc.buf[BUF_FRAME_JOBS].grow(s, n * sizeof(nxz_batch_job_t));
		return sc.buf[BUF_FRAME_JOBS].as<nxz_batch_job_t>();
	});
	if (!d) return -ENOMEM;
	return launched("frame header launch", dict ? nxz_launch_frame_header_dict(fmt, jobs, n, frames, d, dict->id, s)
						    : nxz_launch_frame_header(fmt, jobs, n, frames, d, s));
}

int framed_locked(nxz_ctx_t *c, int fmt, const nxz_batch_job_t *jobs, size_t n, nxz_batch_result_t *results, nxz_batch_frame_t *frames, hipStream_t s,
		  const nxz_dict *dict)
{
	nxz_batch_job_t *derived = nullptr;
	int rc = derive_framed_jobs(c, fmt, dict, jobs, n, frames, s, &derived);
	if (rc) return rc;
	rc = dict ? batch_decompress_dict(c, dict, derived, n, results, s) : batch_decompress(c, derived, n, results, nullptr, s, 0);
	if (rc) return rc;
	return launched("frame trailer launch", nxz_launch_frame_trailer(jobs, n, results, frames, s));
}

extern "C" int nxz_batch_decompress_framed(nxz_ctx_t *c, int fmt, const nxz_batch_job_t *jobs, size_t n,
					   nxz_batch_result_t *results, nxz_batch_frame_t *frames, void *stream)
{
	if (!c || fmt < NXZ_FMT_ZLIB || fmt > NXZ_FMT_AUTO || n >= (1u << 31) || (n && (!jobs || !results || !frames))) return -EINVAL;
	const Entered in(c, stream, n != 0);
	if (in.rc != 1) return in.rc;
	return framed_locked(c, fmt, jobs, n, results, frames, in.s);
}

extern "C" int nxz_batch_decompress_framed_dict(nxz_ctx_t *c, int fmt, const nxz_dict_t *dict, const nxz_batch_job_t *jobs, size_t n,
						nxz_batch_result_t *results, nxz_batch_frame_t *frames, void *stream)
{
	if (!c || !dict || dict->device != c->device || fmt < NXZ_FMT_ZLIB || fmt > NXZ_FMT_AUTO || n >= (1u << 31) || (n && (!jobs || !results || !frames))) return -EINVAL;
	const Entered in(c, stream, n != 0);
	if (in.rc != 1) return in.rc;
	return framed_locked(c, fmt, jobs, n, results, frames, in.s, dict);
}

// ---------------------------------------------------------------------------
// Output sizes (nxz_inflate_size.hip): what the streams would produce, a wavefront each, all on `s`, nothing waits.  From 128
// streams on the long ones start first (the order is this stream's scratch, as for the decode routes: ordered_launch).  The caller holds no lease.
// ---------------------------------------------------------------------------
static int batch_size(nxz_ctx_t *c, const nxz_batch_job_t *jobs, size_t n, nxz_batch_result_t *results, uint32_t dict_window, hipStream_t s)
{
	return ordered_launch(c, s, jobs, n, "inflate size launch", [&](const uint32_t *order) { return nxz_launch_inflate_size(jobs, n, results, order, dict_window, s); });
}

extern "C" int nxz_batch_decompress_size(nxz_ctx_t *c, const nxz_batch_job_t *jobs, size_t n, nxz_batch_result_t *results, void *stream)
{
	if (!c || n >= (1u << 31) || (n && (!jobs || !results))) return -EINVAL;
	const Entered in(c, stream, n != 0, false);
	return in.rc != 1 ? in.rc : batch_size(c, jobs, n, results, 0, in.s);
}

// header kernel (the framed decode's own: derive_framed_jobs) -> the size walk on the derived jobs ->
// the trailer step without the checksum comparison.  frame_use[s] guards the derived jobs, as in framed_locked.
extern "C" int nxz_batch_decompress_size_framed(nxz_ctx_t *c, int fmt, const nxz_dict_t *dict, const nxz_batch_job_t *jobs, size_t n,
						nxz_batch_result_t *results, nxz_batch_frame_t *frames, void *stream)
{
	if (!c || (dict && dict->device != c->device) || fmt < NXZ_FMT_ZLIB || fmt > NXZ_FMT_AUTO || n >= (1u << 31) || (n && (!jobs || !results || !frames))) return -EINVAL;
	const Entered in(c, stream, n != 0);
	if (in.rc != 1) return in.rc;
	hipStream_t s = in.s;
	nxz_batch_job_t *derived = nullptr;
	int rc = derive_framed_jobs(c, fmt, dict, jobs, n, frames, s, &derived);
	if (rc) return rc;
	// (without a dictionary the header kernel sets no NXZ_JOB_NO_DICT, and there is no window to withhold: 0)
	if ((rc = batch_size(c, derived, n, results, dict ? dict->win : 0, s)) != 0) return rc;
	return launched("frame trailer launch", nxz_launch_size_trailer(jobs, n, results, frames, s));
}

// ---------------------------------------------------------------------------
// Verify (nxz_inflate_verify.hip, the rules in nxz_verify.h): the size calls with the output passing through a ring in LDS and
// checksummed there -- the same single launch, the same order, the same lease; the framed call ends with the decode's own trailer
// kernel, comparison included.  A dictionary's window is read from its one device copy.
// ---------------------------------------------------------------------------
static int batch_verify(nxz_ctx_t *c, const nxz_batch_job_t *jobs, size_t n, nxz_batch_result_t *results, const nxz_dict *dict, hipStream_t s)
{
	return ordered_launch(c, s, jobs, n, "inflate verify launch", [&](const uint32_t *order) {
		return nxz_launch_inflate_verify(jobs, n, results, order, dict ? dict->d_win : nullptr, dict ? dict->win : 0, s);
	});
}

extern "C" int nxz_batch_decompress_verify(nxz_ctx_t *c, const nxz_batch_job_t *jobs, size_t n, nxz_batch_result_t *results, void *stream)
{
	if (!c || n >= (1u << 31) || (n && (!jobs || !results))) return -EINVAL;
	const Entered in(c, stream, n != 0, false);
	return in.rc != 1 ? in.rc : batch_verify(c, jobs, n, results, nullptr, in.s);
}

extern "C" int nxz_batch_decompress_verify_framed(nxz_ctx_t *c, int fmt, const nxz_dict_t *dict, const nxz_batch_job_t *jobs, size_t n,
						  nxz_batch_result_t *results, nxz_batch_frame_t *frames, void *stream)
{
	if (!c || (dict && dict->device != c->device) || fmt < NXZ_FMT_ZLIB || fmt > NXZ_FMT_AUTO || n >= (1u << 31) || (n && (!jobs || !results || !frames))) return -EINVAL;
	const Entered in(c, stream, n != 0);
	if (in.rc != 1) return in.rc;
	hipStream_t s = in.s;
	nxz_batch_job_t *derived = nullptr;
	int rc = derive_framed_jobs(c, fmt, dict, jobs, n, frames, s, &derived);
	if (rc) return rc;
	if ((rc = batch_verify(c, derived, n, results, dict, s)) != 0) return rc;
	return launched("frame trailer launch", nxz_launch_frame_trailer(jobs, n, results, frames, s));
}

// ---------------------------------------------------------------------------
// Multi-member gzip jobs (nxz_gzip_members.hip, the rules in nxz_gzip_members.h).  The index is the size query's shape: a wavefront
// a job, from 128 jobs on the long ones first, the order in this stream's scratch under the lease.  The decode holds frame_use[s]
// from its first kernel to its last -- BUF_GZIP_MEMBERS is the framed batch framed_locked works on -- and never waits for the host.
// ---------------------------------------------------------------------------
extern "C" int nxz_batch_gzip_members_size(nxz_ctx_t *c, const nxz_batch_job_t *jobs, size_t n, uint32_t member_cap,
					   nxz_gzip_member_t *members, nxz_gzip_stream_t *streams, void *stream)
{
	if (!c || member_cap == 0 || n >= (1u << 31) || (n && (!jobs || !members || !streams))) return -EINVAL;
	const Entered in(c, stream, n != 0, false);
	if (in.rc != 1) return in.rc;
	return ordered_launch(c, in.s, jobs, n, "gzip members index launch", [&](const uint32_t *order) {
		return nxz_launch_gzip_members_index(jobs, n, member_cap, members, streams, order, in.s);
	});
}

extern "C" int nxz_batch_gzip_members_decode(nxz_ctx_t *c, const nxz_batch_job_t *jobs, size_t n, uint32_t member_cap,
					     nxz_gzip_member_t *members, nxz_gzip_stream_t *streams, size_t total_members, void *stream)
{
	if (!c || member_cap == 0 || total_members < n || n >= (1u << 31) || (n && (!jobs || !members || !streams))) return -EINVAL;
	const Entered in(c, stream, n != 0);
	if (in.rc != 1) return in.rc;
	const uint64_t slots = (uint64_t)n * member_cap;                     // (n < 2^31, member_cap < 2^32: no overflow)
	const size_t total = (size_t)std::min<uint64_t>(total_members, slots);
	if (total >= (1u << 31) || slots >= (1ull << 39)) return -E2BIG;     // (the framed batch; a thread a record slot in one grid)
	hipStream_t s = in.s;
	uint8_t *const ws = with_scratch(c, s, [&](nxz_ctx::Scratch &sc) {
		(void)sc.buf[BUF_GZIP_MEMBERS].grow(s, nxz_gzip_members_workspace(n, total));
		return sc.buf[BUF_GZIP_MEMBERS].p;
	});
	if (!ws) return -ENOMEM;
	nxz_batch_job_t *xjobs = nullptr;
	nxz_batch_result_t *xresults = nullptr;
	nxz_batch_frame_t *xframes = nullptr;
	int rc = launched("gzip members expand launch", nxz_launch_gzip_members_expand(jobs, n, member_cap, members, streams, total, ws, &xjobs, &xresults, &xframes, s));
	if (rc) return rc;
	if ((rc = framed_locked(c, NXZ_FMT_GZIP, xjobs, total, xresults, xframes, s)) != 0) return rc;
	return launched("gzip members join launch", nxz_launch_gzip_members_join(n, member_cap, members, streams, total, ws, s));
}
