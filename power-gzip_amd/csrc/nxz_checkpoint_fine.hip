// nxz_checkpoint_fine.hip -- checkpoints INSIDE deflate blocks (nxz_batch_checkpoint_index_fine / nxz_checkpoint_read_ranges_fine;
// gfx950, wave64).  The rules are nxz_checkpoint_fine.h's on top of nxz_checkpoint.h's.  As in nxz_checkpoint.hip there is no decoder
// here: the index is the size walk (nxz_inflate_walk.h) with a hook that cuts between tokens, and a range read decodes its segments
// with nxz_batch_decompress as jobs that resume inside a block.
//
// The index (nxz_batch_ranges.cpp queues it, nothing waits for the host):
//   index_kernel     nxzcp::index_kernel's shape -- one job per wavefront, the header by nxz_frame.h's parser, then nxzs::walk -- with a
//                    hook that gives the walk a budget of span bytes a segment: the walk calls it in front of the token that does
//                    not fit (a stored run: behind the bytes that do), and lane 0 stores cbit / uoff / state; the stream's record
//                    and the sentinel last.  LDS is the walk's; the accumulator lives in scalar registers.
//   (the windows: nxzcp::window_kernel as it is, nxz_launch_checkpoint_windows)
// A range read is nxz_checkpoint_read_ranges with two steps of its own (the map, inmax, stage and verdict kernels are nxz_checkpoint.hip's):
//   check_kernel     a thread an entry: nxz_cpf_entry_ok -- nxz_cp_entry_ok and the state's rules; any fault sets ctl[0]
//   jobs_kernel      behind nxzcp::stage_kernel, a wavefront per needed segment of the chunk: the segment's table slot -- bits
//                    [tbit, tbit + dhtlen) of src shifted to bit 0, zeros behind -- and the job's resume and flag
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "nxz_device.h"
#include "nxz_frame.h"
#include "nxz_frame_wave.h"
#include "nxz_inflate_walk.h"
#include "nxz_checkpoint_fine.h"

namespace nxzcf {

using nxzi::uni;

// what the walk calls: at every block header (the first is checkpoint 0, no other header is one), for its budget, and in front of
// every token that does not fit it
struct Hook {
	static constexpr bool fine = true;
	nxz_cp_acc_t *acc;
	uint64_t *cbit, *uoff;
	nxz_checkpoint_state_t *state;
	uint64_t span;
	uint32_t cp_cap, hdr_len;
	int lane;
	__device__ __forceinline__ void store(uint64_t bit, uint32_t u, const nxz_checkpoint_state_t &s) const
	{
		const uint32_t k = nxz_cp_add(acc, u, cp_cap);
		if (k < cp_cap && lane == 0) { cbit[k] = nxz_cp_bit(hdr_len, bit); uoff[k] = u; state[k] = s; }
	}
	__device__ __forceinline__ void operator()(uint64_t bit, uint32_t out) const
	{
		if (acc->count == 0) store(bit, uni(out), nxz_cpf_state(0, 0, 0, 0));
	}
	__device__ __forceinline__ uint32_t budget(uint32_t cap) const { return uni(nxz_cpf_budget(acc, span, cap)); }
	__device__ __forceinline__ void cut(uint64_t bit, uint32_t out, uint32_t sfbt, uint32_t rem, uint64_t tpos, uint32_t tbits) const
	{
		store(bit, uni(out), nxz_cpf_state(uni(sfbt), uni(rem), nxz_cp_bit(hdr_len, tpos), uni(tbits)));
	}
};

__global__ __launch_bounds__(64) void index_kernel(int fmt, const nxz_batch_job_t *__restrict__ jobs, const uint32_t *__restrict__ order, uint64_t span,
						   uint32_t cp_cap, uint64_t *__restrict__ cbit, uint64_t *__restrict__ uoff,
						   nxz_checkpoint_state_t *__restrict__ state, int want_windows, nxz_checkpoint_stream_t *__restrict__ streams)
{
	__shared__ __attribute__((aligned(16))) nxzs::Smem sm;
	const int lane = threadIdx.x;
	const uint32_t jid = order ? order[blockIdx.x] : blockIdx.x;
	const nxz_batch_job_t job = jobs[jid];
	if (!nxz_cp_job_ok(job.resume, job.hist_len)) {
		if (lane == 0) streams[jid] = nxz_cp_refused();
		return;
	}
	const uint32_t src_len = uni(job.src_len);
	uint32_t format = NXZ_FMT_RAW, hdr_len = 0, st = NXZ_FRAME_OK;
	if (fmt != NXZ_FMT_RAW) {
		nxz_batch_frame_t f;
		WaveOps ops{(uint32_t)lane};
		st = uni(nxz_frame_parse(job.src, src_len, fmt, &f, ops));
		format = uni(f.format); hdr_len = uni(f.hdr_len);
	}
	const size_t base = (size_t)jid * ((size_t)cp_cap + 1);
	uint64_t *const cb = cbit + base, *const uo = uoff + base;
	nxz_checkpoint_state_t *const sta = state + base;
	nxz_cp_acc_t acc = nxz_cp_begin();
	nxz_size_stop_t stop = {};
	uint64_t end_bit = 0;
	if (st == NXZ_FRAME_OK)
		nxzs::walk(sm, (const NXZ_GLOBAL_AS uint8_t *)job.src + hdr_len, src_len - hdr_len, 0xffffffffu, 0, lane, stop, end_bit,
			   Hook{&acc, cb, uo, sta, span, cp_cap, hdr_len, lane});
	const uint32_t produced = uni(stop.produced);
	const nxz_checkpoint_stream_t s = nxz_cp_summary(&acc, cp_cap, format, hdr_len, st, uni(stop.cc), uni(stop.final_eob), produced,
							 want_windows != 0, nxz_cp_have_output(job.dst, job.dst_cap, produced));
	if (lane == 0) {
		streams[jid] = s;
		if (nxz_cp_has_sentinel(s.status)) { cb[s.count] = nxz_cp_bit(hdr_len, end_bit); uo[s.count] = produced; sta[s.count] = nxz_cpf_state(0, 0, 0, 0); }
	}
}

// ctl[0]: index faulty (nxzcp::check_kernel's word)
__global__ __launch_bounds__(256) void check_kernel(uint64_t src_len, const uint64_t *__restrict__ cbit, const uint64_t *__restrict__ uoff,
						    const nxz_checkpoint_state_t *__restrict__ state, uint64_t L, uint64_t *__restrict__ ctl)
{
	const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (j >= L) return;
	if (!nxz_cpf_entry_ok(cbit, uoff, state, L, j, src_len)) atomicOr((unsigned long long *)&ctl[0], 1ull);
}

// needed segment k0 + blockIdx.x, whose job nxzcp::stage_kernel has written: its table slot and what a fine segment's job adds
__global__ __launch_bounds__(64) void jobs_kernel(const uint8_t *__restrict__ src, const uint64_t *__restrict__ cbit,
						  const nxz_checkpoint_state_t *__restrict__ state, const uint32_t *__restrict__ list, uint64_t k0,
						  nxz_batch_job_t *__restrict__ jobs, nxz_batch_dht_t *__restrict__ dht)
{
	const uint64_t kk = blockIdx.x;
	const uint64_t j = list[k0 + kk];
	const nxz_checkpoint_state_t s = state[j];
	const bool dyn = nxz_cpf_is_dynamic(nxz_cpf_sfbt(s.resume));
	nxz_batch_dht_t *const t = &dht[kk];
	for (uint32_t i = threadIdx.x; i < sizeof(t->dht); i += 64) t->dht[i] = dyn ? nxz_cpf_dht_byte(src, s.tbit, s.dhtlen, i) : 0;
	if (threadIdx.x == 0) {
		t->dhtlen = dyn ? s.dhtlen : 0;
		jobs[kk].resume = nxz_cpf_resume(&s, cbit[j]);
		jobs[kk].reserved = nxz_cpf_job_flags();
	}
}

} // namespace nxzcf

// n jobs, a wavefront each (order: NULL, or nxz_launch_order_by_length's); then, with windows, nxz_checkpoint.hip's copies of them
extern "C" int nxz_launch_checkpoint_index_fine(int fmt, const nxz_batch_job_t *jobs, size_t n, uint64_t span, uint32_t cp_cap, uint64_t *cbit, uint64_t *uoff,
						nxz_checkpoint_state_t *state, uint8_t *windows, nxz_checkpoint_stream_t *streams, const uint32_t *order,
						hipStream_t stream)
{
	if (!n) return 0;
	hipLaunchKernelGGL(nxzcf::index_kernel, dim3((unsigned)n), dim3(64), 0, stream, fmt, jobs, order, span, cp_cap, cbit, uoff, state, windows ? 1 : 0, streams);
	const int rc = (int)hipGetLastError();
	return rc || !windows ? rc : nxz_launch_checkpoint_windows(jobs, n, cp_cap, uoff, streams, windows, stream);
}

// nxz_launch_checkpoint_check for a fine index
extern "C" int nxz_launch_checkpoint_check_fine(uint64_t src_len, const uint64_t *cbit, const uint64_t *uoff, const nxz_checkpoint_state_t *state, uint64_t L,
						uint8_t *ws, hipStream_t stream)
{
	if (!L) return 0;
	hipLaunchKernelGGL(nxzcf::check_kernel, dim3((unsigned)((L + 255) / 256)), dim3(256), 0, stream, src_len, cbit, uoff, state, L, (uint64_t *)ws);
	return (int)hipGetLastError();
}

// behind nxz_launch_checkpoint_stage on the same chunk: dht[k - k0] and the jobs' resume / reserved
extern "C" int nxz_launch_checkpoint_jobs_fine(const uint8_t *src, const uint64_t *cbit, const nxz_checkpoint_state_t *state, uint64_t n, uint64_t L, uint8_t *ws,
					       uint64_t k0, uint64_t cnt, nxz_batch_job_t *jobs, nxz_batch_dht_t *dht, hipStream_t stream)
{
	if (!cnt) return 0;
	if (cnt >= (1ull << 31)) return (int)hipErrorInvalidValue;
	const uint32_t *midx, *list;
	nxz_range_map_lists(ws, n, L, &midx, &list);
	hipLaunchKernelGGL(nxzcf::jobs_kernel, dim3((unsigned)cnt), dim3(64), 0, stream, src, cbit, state, list, k0, jobs, dht);
	return (int)hipGetLastError();
}
