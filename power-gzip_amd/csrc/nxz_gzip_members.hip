// nxz_gzip_members.hip -- multi-member gzip jobs on the device (nxz_batch_gzip_members_size / _decode; gfx950, wave64).  The rules
// are nxz_gzip_members.h's; here is the bit-walking and the plumbing.
//
// The index (index_kernel): one job per wavefront, one wavefront per workgroup, the long jobs first -- the shape of the size query
// (nxz_inflate_size.hip), and its walk (nxz_inflate_walk.h).  The wavefront loops member after member INSIDE the kernel: header
// (nxz_frame.h's parser, every lane on the same bytes, the name / comment scans and FHCRC by all of them), the size walk over the
// deflate bytes, the 8-byte trailer, the record from lane 0, the two bytes behind it.  No host round trip and no launch per member:
// a WARC-like job of thousands of small members is one wavefront's loop.  Successive members start at any byte: the walk takes its
// source at any alignment.  LDS is the walk's (tables, stage, code lengths: 6.5 KiB); the parsed header lives in registers.
//
// The decode, all on the caller's stream (nxz_batch_framed.cpp queues it, nothing waits for the host):
//   check_kernel    a thread a record slot: a stored OK record that does not lie inside its job marks the job stale
//   plan_kernel     one workgroup: per job what nxz_gzm_plan says (TARGET_SPACE / INVALID written to streams[i].status) and the
//                   exclusive prefix sum of the members to decode
//   fill_kernel     every one of the total_members slots becomes an empty framed job (src_len = dst_cap = 0: every route ends it
//                   at once -- the device of the framed header kernel for failed headers), owned by nobody
//   expand_kernel   a thread a record slot: member k of job i -> the framed gzip job base[i] + k (src + coff, clen, dst + uoff, isize)
//   ... nxz_batch_decompress_framed's path on the slots (framed_locked) ...
//   join_kernel     a thread a slot: the frame status into the member's record; per job the lowest failed index (atomicMin) and
//                   the bytes decoded (atomicAdd: integer sums, the same whatever the order)
//   finish_kernel   a thread a job: nxz_gzm_join
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "nxz_device.h"
#include "nxz_frame.h"
#include "nxz_frame_wave.h"
#include "nxz_inflate_walk.h"
#include "nxz_gzip_members.h"

namespace nxzg {

using nxzi::uni;

// (what a member leaves behind -- status, lengths, sums -- is the same in all lanes: uni() keeps it in scalar registers)
__global__ __launch_bounds__(64) void index_kernel(const nxz_batch_job_t *__restrict__ jobs, const uint32_t *__restrict__ order, uint32_t member_cap,
						   nxz_gzip_member_t *__restrict__ members, nxz_gzip_stream_t *__restrict__ streams)
{
	__shared__ __attribute__((aligned(16))) nxzs::Smem sm;
	const int lane = threadIdx.x;
	const uint32_t jid = order ? order[blockIdx.x] : blockIdx.x;
	const nxz_batch_job_t job = jobs[jid];
	if (!nxz_gzm_job_ok(job.resume, job.hist_len)) {
		if (lane == 0) streams[jid] = nxz_gzm_refused();
		return;
	}
	const uint32_t src_len = uni(job.src_len);
	nxz_gzip_member_t *const out = members + (size_t)jid * member_cap;
	nxz_gzm_acc_t acc = nxz_gzm_begin();
	uint32_t pos = 0;
	for (;;) {
		const uint8_t *const p = job.src + pos;
		const uint32_t left = src_len - pos;
		nxz_gzip_member_t m = nxz_gzm_member(acc.out_len, pos);
		nxz_batch_frame_t f;
		WaveOps ops{(uint32_t)lane};
		uint32_t st = uni(nxz_frame_parse(p, left, NXZ_FMT_GZIP, &f, ops)), cc = 0;
		if (st == NXZ_FRAME_OK) {
			m.hdr_len = uni(f.hdr_len);
			if (!nxz_gzm_room(left, m.hdr_len)) st = NXZ_FRAME_TRUNCATED;
		}
		if (st == NXZ_FRAME_OK) {
			nxz_size_stop_t stop = {};
			uint64_t end_bit;
			nxzs::walk(sm, (const NXZ_GLOBAL_AS uint8_t *)p + m.hdr_len, left - m.hdr_len - NXZ_GZM_TRAILER, 0xffffffffu, 0, lane, stop, end_bit);
			const uint32_t wcc = uni(stop.cc), eob = uni(stop.final_eob);
			st = nxz_gzm_walk_status(wcc, eob);
			cc = nxz_gzm_walk_cc(wcc, eob);
			if (st == NXZ_FRAME_OK) {
				const uint32_t dend = m.hdr_len + uni((uint32_t)((end_bit + 7) >> 3));      // (at most left - 8: the walk's source ends there)
				const uint8_t *const t = p + dend;
				st = nxz_gzm_trailer(&m, dend, uni(nxz_rd32le(t)), uni(nxz_rd32le(t + 4)), uni(stop.produced));
			}
		}
		m.status = st;
		if (nxz_gzm_stored(&acc, member_cap) && lane == 0) out[acc.members] = m;
		if (!nxz_gzm_add(&acc, &m, cc)) break;
		pos = acc.consumed;
		if (!uni(nxz_gzm_more(job.src, src_len, pos))) break;
	}
	if (lane == 0) streams[jid] = nxz_gzm_summary(&acc, member_cap);
}

// ---- the decode's plumbing --------------------------------------------------------------------------------------------------
// per job, in the stream's scratch
struct JobPlan {
	uint64_t decoded;        // join_kernel: bytes of the members that decoded OK
	uint32_t base;           // the first slot of the job's members
	uint32_t count;          // members that are decoded
	uint32_t first_bad;      // join_kernel: the lowest failed index, 0xffffffff none
	uint32_t stale;          // check_kernel: a record points outside the job
};
struct Owner { uint32_t job, k; };   // of a slot; job 0xffffffff: nobody's

__device__ inline uint32_t stored_ok(const nxz_gzip_stream_t *s, uint32_t member_cap)
{
	return nxz_gzm_decodable(s->status) ? nxz_gzm_stored_ok(s->failed, member_cap) : 0;
}

__global__ __launch_bounds__(256) void check_kernel(const nxz_batch_job_t *__restrict__ jobs, uint64_t slots, uint32_t member_cap,
						    const nxz_gzip_member_t *__restrict__ members, const nxz_gzip_stream_t *__restrict__ streams,
						    JobPlan *__restrict__ plan)
{
	const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (t >= slots) return;
	const uint32_t i = (uint32_t)(t / member_cap), k = (uint32_t)(t % member_cap);
	if (k >= stored_ok(&streams[i], member_cap)) return;
	if (!nxz_gzm_record_inside(&members[t], jobs[i].src_len, jobs[i].dst_cap)) atomicOr(&plan[i].stale, 1u);
}

// one workgroup: thread t takes the jobs [t * per, (t + 1) * per)
__global__ __launch_bounds__(1024) void plan_kernel(const nxz_batch_job_t *__restrict__ jobs, uint32_t n, uint32_t member_cap,
						     nxz_gzip_stream_t *__restrict__ streams, uint64_t total_members, JobPlan *__restrict__ plan)
{
	__shared__ uint64_t part[1024];
	const uint32_t t = threadIdx.x, per = (n + 1023) / 1024;
	const uint32_t lo = (uint64_t)t * per < n ? t * per : n, hi = (uint64_t)lo + per < n ? lo + per : n;
	// (a job that is refused for its target or a stale record counts nothing; one that does not fit total_members counts, so
	// that every job behind it is refused as well)
	auto wanted = [&](uint32_t i) -> uint32_t {
		const nxz_gzip_stream_t s = streams[i];
		uint32_t count;
		(void)nxz_gzm_plan(s.status, s.out_len, s.failed, member_cap, jobs[i].dst_cap, plan[i].stale != 0, 0, ~0ull, &count);
		return count;
	};
	uint64_t sum = 0;
	for (uint32_t i = lo; i < hi; i++) sum += wanted(i);
	uint64_t tot;
	uint64_t o = nxz_block_excl(sum, part, &tot);
	for (uint32_t i = lo; i < hi; i++) {
		const nxz_gzip_stream_t s = streams[i];
		const uint32_t w = wanted(i);
		uint32_t count;
		const uint32_t st = nxz_gzm_plan(s.status, s.out_len, s.failed, member_cap, jobs[i].dst_cap, plan[i].stale != 0, o, total_members, &count);
		if (st != s.status) streams[i].status = st;
		plan[i].base = (uint32_t)(o < total_members ? o : total_members);
		plan[i].count = count;
		plan[i].first_bad = 0xffffffffu;
		plan[i].decoded = 0;
		o += w;
	}
}

__global__ __launch_bounds__(256) void fill_kernel(uint64_t total_members, uint8_t *pad, nxz_batch_job_t *__restrict__ xjobs, Owner *__restrict__ owner)
{
	const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (t >= total_members) return;
	nxz_batch_job_t e = {};
	e.src = pad; e.dst = pad; e.in_adler = 1;                           // (16-byte aligned bytes of the scratch: nothing reads or writes them)
	xjobs[t] = e;
	owner[t] = Owner{0xffffffffu, 0};
}

__global__ __launch_bounds__(256) void expand_kernel(const nxz_batch_job_t *__restrict__ jobs, uint64_t slots, uint32_t member_cap,
						     const nxz_gzip_member_t *__restrict__ members, const JobPlan *__restrict__ plan,
						     nxz_batch_job_t *__restrict__ xjobs, Owner *__restrict__ owner)
{
	const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (t >= slots) return;
	const uint32_t i = (uint32_t)(t / member_cap), k = (uint32_t)(t % member_cap);
	if (k >= plan[i].count) return;
	const nxz_gzip_member_t m = members[t];
	nxz_batch_job_t x = {};
	x.src = jobs[i].src + m.coff; x.src_len = m.clen;
	x.dst = jobs[i].dst + m.uoff; x.dst_cap = m.isize;
	x.in_adler = 1;
	const uint64_t slot = (uint64_t)plan[i].base + k;
	xjobs[slot] = x;
	owner[slot] = Owner{i, k};
}

__global__ __launch_bounds__(256) void join_kernel(uint64_t total_members, uint32_t member_cap, const Owner *__restrict__ owner,
						   const nxz_batch_frame_t *__restrict__ xframes, nxz_gzip_member_t *__restrict__ members,
						   JobPlan *__restrict__ plan)
{
	const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (t >= total_members) return;
	const Owner o = owner[t];
	if (o.job == 0xffffffffu) return;
	nxz_gzip_member_t *const m = &members[(uint64_t)o.job * member_cap + o.k];
	const uint32_t st = xframes[t].status;
	m->status = st;
	if (st == NXZ_FRAME_OK) atomicAdd((unsigned long long *)&plan[o.job].decoded, (unsigned long long)m->isize);
	else atomicMin(&plan[o.job].first_bad, o.k);
}

__global__ __launch_bounds__(256) void finish_kernel(uint32_t n, const JobPlan *__restrict__ plan, const nxz_batch_result_t *__restrict__ xresults,
						     nxz_gzip_stream_t *__restrict__ streams)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const JobPlan p = plan[i];
	nxz_gzip_stream_t s = streams[i];
	if (!nxz_gzm_decodable(s.status)) return;                           // (refused by plan_kernel: nothing of it was decoded)
	nxz_gzm_join(&s, p.first_bad, p.first_bad != 0xffffffffu ? xresults[(uint64_t)p.base + p.first_bad].cc : 0, p.decoded);
	streams[i] = s;
}

} // namespace nxzg

// n jobs, a wavefront each; order: NULL, or nxz_launch_order_by_length's
extern "C" int nxz_launch_gzip_members_index(const nxz_batch_job_t *jobs, size_t n, uint32_t member_cap, nxz_gzip_member_t *members,
					     nxz_gzip_stream_t *streams, const uint32_t *order, hipStream_t stream)
{
	if (!n) return 0;
	hipLaunchKernelGGL(nxzg::index_kernel, dim3((unsigned)n), dim3(64), 0, stream, jobs, order, member_cap, members, streams);
	return (int)hipGetLastError();
}

// The decode's scratch for n jobs and total_members slots: [pad 256][JobPlan n][Owner][jobs][frames][results], each 256-byte aligned
static size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
struct MembersWs {
	uint8_t *pad;
	nxzg::JobPlan *plan;
	nxzg::Owner *owner;
	nxz_batch_job_t *xjobs;
	nxz_batch_frame_t *xframes;
	nxz_batch_result_t *xresults;
	size_t bytes;
};
static MembersWs members_ws(uint8_t *ws, size_t n, size_t total_members)
{
	MembersWs w;
	size_t o = 0;
	auto take = [&](size_t b) { uint8_t *q = ws + o; o += up256(b); return q; };
	w.pad = take(256);
	w.plan = (nxzg::JobPlan *)take(n * sizeof(nxzg::JobPlan));
	w.owner = (nxzg::Owner *)take(total_members * sizeof(nxzg::Owner));
	w.xjobs = (nxz_batch_job_t *)take(total_members * sizeof(nxz_batch_job_t));
	w.xframes = (nxz_batch_frame_t *)take(total_members * sizeof(nxz_batch_frame_t));
	w.xresults = (nxz_batch_result_t *)take(total_members * sizeof(nxz_batch_result_t));
	w.bytes = o;
	return w;
}
extern "C" size_t nxz_gzip_members_workspace(size_t n, size_t total_members) { return members_ws(nullptr, n, total_members).bytes; }

// check, plan, fill, expand: *xjobs, *xresults and *xframes (inside ws) are the framed batch of total_members jobs
extern "C" int nxz_launch_gzip_members_expand(const nxz_batch_job_t *jobs, size_t n, uint32_t member_cap, const nxz_gzip_member_t *members,
					      nxz_gzip_stream_t *streams, size_t total_members, uint8_t *ws, nxz_batch_job_t **xjobs,
					      nxz_batch_result_t **xresults, nxz_batch_frame_t **xframes, hipStream_t stream)
{
	const MembersWs w = members_ws(ws, n, total_members);
	*xjobs = w.xjobs; *xresults = w.xresults; *xframes = w.xframes;
	const uint64_t slots = (uint64_t)n * member_cap;
	const unsigned gs = (unsigned)((slots + 255) / 256), gt = (unsigned)((total_members + 255) / 256);
	(void)hipMemsetAsync(w.plan, 0, n * sizeof(nxzg::JobPlan), stream);
	hipLaunchKernelGGL(nxzg::check_kernel, dim3(gs), dim3(256), 0, stream, jobs, slots, member_cap, members, streams, w.plan);
	hipLaunchKernelGGL(nxzg::plan_kernel, dim3(1), dim3(1024), 0, stream, jobs, (uint32_t)n, member_cap, streams, (uint64_t)total_members, w.plan);
	hipLaunchKernelGGL(nxzg::fill_kernel, dim3(gt), dim3(256), 0, stream, (uint64_t)total_members, w.pad, w.xjobs, w.owner);
	hipLaunchKernelGGL(nxzg::expand_kernel, dim3(gs), dim3(256), 0, stream, jobs, slots, member_cap, members, w.plan, w.xjobs, w.owner);
	return (int)hipGetLastError();
}

// join, finish: behind the framed decode of the slots
extern "C" int nxz_launch_gzip_members_join(size_t n, uint32_t member_cap, nxz_gzip_member_t *members, nxz_gzip_stream_t *streams,
					    size_t total_members, uint8_t *ws, hipStream_t stream)
{
	const MembersWs w = members_ws(ws, n, total_members);
	hipLaunchKernelGGL(nxzg::join_kernel, dim3((unsigned)((total_members + 255) / 256)), dim3(256), 0, stream, (uint64_t)total_members, member_cap,
			   w.owner, w.xframes, members, w.plan);
	hipLaunchKernelGGL(nxzg::finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, (uint32_t)n, w.plan, w.xresults, streams);
	return (int)hipGetLastError();
}
