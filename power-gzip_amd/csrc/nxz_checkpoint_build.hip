// nxz_checkpoint_build.hip -- the checkpoint index with its windows from the source alone (nxz_batch_checkpoint_build; gfx950, wave64):
// what zran and indexed_gzip do on a CPU, one pass over the compressed data with a sliding 32 KiB window.  The rules of positions,
// states and records are nxz_checkpoint.h's and nxz_checkpoint_fine.h's, the ring's are nxz_checkpoint_build.h's.  No bit-walker
// of its own: the index is the size walk (nxz_inflate_walk.h) with a hook that cuts between tokens AND receives their bytes.
//
//   build_kernel     nxzcp::index_kernel's shape -- one job per wavefront, one wavefront per workgroup, the long jobs first, the
//                    header by nxz_frame.h's parser, then nxzs::walk.  The hook applies every token to a ring of 32 KiB in LDS
//                    (nxz_ring_wave.h's writers, shared with nxz_inflate_verify.hip) and, where a checkpoint is stored, lane 0
//                    writes cbit / uoff / state and the wavefront dumps the ring to the checkpoint's slot: min(uoff, 32768)
//                    bytes, oldest first, 16 bytes a lane where the slot's
//                    alignment allows (LDS is read in aligned dwords and shifted into place).  state == NULL: checkpoints at
//                    block headers only (nxz_checkpoint.h's rule 2), the budget is never below the cap and nothing is cut.
//                    LDS is the walk's 6704 bytes and the ring: four workgroups a CU.  The accumulator lives in scalar registers.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "nxz_device.h"
#include "nxz_frame.h"
#include "nxz_frame_wave.h"
#include "nxz_inflate_walk.h"
#include "nxz_checkpoint_fine.h"
#include "nxz_checkpoint_build.h"
#include "nxz_ring_wave.h"

namespace nxzcb {

using nxzi::uni;

// ring [rs, rs + len) -> d[0, len): the 16-byte granules that lie whole inside d by 16-byte stores, the bytes in front and behind one
// by one (nxzcp::copy_any with LDS for a source: five aligned dwords a granule, shifted by the ring position's low bits)
__device__ __forceinline__ void ring_out(const uint32_t *ring, uint32_t rs, uint32_t len, uint8_t *d, int lane)
{
	const uint8_t *const rb = (const uint8_t *)ring;
	uint32_t head = (uint32_t)((16 - ((uintptr_t)d & 15)) & 15);
	if (head > len) head = len;
	const uint32_t body = (len - head) >> 4;
	for (uint32_t i = lane; i < head; i += 64) d[i] = rb[rs + i];
	for (uint32_t g = lane; g < body; g += 64) {
		const uint32_t s = rs + head + 16 * g, a = s >> 2, sh = s & 3;        // (s + 16 <= NXZ_CB_RING: the fifth dword may be the ring's first)
		const uint32_t d0 = ring[a], d1 = ring[a + 1], d2 = ring[a + 2], d3 = ring[a + 3], d4 = ring[(a + 4) & (NXZ_CB_RING / 4 - 1)];
		*(uint4 *)(d + head + 16 * g) = make_uint4(__builtin_amdgcn_alignbyte(d1, d0, sh), __builtin_amdgcn_alignbyte(d2, d1, sh),
							   __builtin_amdgcn_alignbyte(d3, d2, sh), __builtin_amdgcn_alignbyte(d4, d3, sh));
	}
	for (uint32_t i = head + 16 * body + lane; i < len; i += 64) d[i] = rb[rs + i];
}

// what the walk calls: at every block header, for its budget, in front of every token that does not fit it -- and with the bytes
// of every token
struct Hook : nxzr::Writer {             // (the bytes: lit / match / stored into the ring)
	static constexpr bool fine = true;
	static constexpr bool bytes = true;
	nxz_cp_acc_t *acc;
	uint64_t *cbit, *uoff;
	nxz_checkpoint_state_t *state;       // NULL: checkpoints at block headers only
	uint8_t *slots;                      // the job's cp_cap window slots
	uint64_t span;
	uint32_t cp_cap, hdr_len;

	// ---- the checkpoints ----
	__device__ __forceinline__ void store(uint64_t bit, uint32_t u, const nxz_checkpoint_state_t &s) const
	{
		const uint32_t k = nxz_cp_add(acc, u, cp_cap);
		if (k >= cp_cap) return;
		if (lane == 0) {
			cbit[k] = nxz_cp_bit(hdr_len, bit); uoff[k] = u;
			if (state) state[k] = s;
		}
		const nxz_cb_pieces_t d = nxz_cb_dump(u);
		uint8_t *const slot = slots + (size_t)k * NXZ_CP_WINDOW;
		__syncthreads();                                                     // (one wavefront: the ring's stores are done)
		ring_out(ring, d.start[0], d.len[0], slot, lane);
		if (d.len[1]) ring_out(ring, d.start[1], d.len[1], slot + d.len[0], lane);
	}
	__device__ __forceinline__ void operator()(uint64_t bit, uint32_t out) const
	{
		const uint32_t u = uni(out);
		if (state ? acc->count == 0 : nxz_cp_is_checkpoint(acc, u, span)) store(bit, u, nxz_cpf_state(0, 0, 0, 0));
	}
	__device__ __forceinline__ uint32_t budget(uint32_t cap) const { return state ? uni(nxz_cpf_budget(acc, span, cap)) : cap; }
	__device__ __forceinline__ void cut(uint64_t bit, uint32_t out, uint32_t sfbt, uint32_t rem, uint64_t tpos, uint32_t tbits) const
	{
		store(bit, uni(out), nxz_cpf_state(uni(sfbt), uni(rem), nxz_cp_bit(hdr_len, tpos), uni(tbits)));
	}
};

__global__ __launch_bounds__(64) void build_kernel(int fmt, const nxz_batch_job_t *__restrict__ jobs, const uint32_t *__restrict__ order, uint64_t span,
						   uint32_t cp_cap, uint64_t *__restrict__ cbit, uint64_t *__restrict__ uoff,
						   nxz_checkpoint_state_t *__restrict__ state, uint8_t *__restrict__ windows,
						   nxz_checkpoint_stream_t *__restrict__ streams)
{
	__shared__ __attribute__((aligned(16))) nxzs::Smem sm;
	__shared__ __attribute__((aligned(16))) uint32_t ring[NXZ_CB_RING / 4];
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
	nxz_checkpoint_state_t *const sta = state ? state + base : nullptr;
	nxz_cp_acc_t acc = nxz_cp_begin();
	nxz_size_stop_t stop = {};
	uint64_t end_bit = 0;
	if (st == NXZ_FRAME_OK)
		nxzs::walk(sm, (const NXZ_GLOBAL_AS uint8_t *)job.src + hdr_len, src_len - hdr_len, 0xffffffffu, 0, lane, stop, end_bit,
			   Hook{{ring, lane}, &acc, cb, uo, sta, windows + (size_t)jid * cp_cap * NXZ_CP_WINDOW, span, cp_cap, hdr_len});
	const uint32_t produced = uni(stop.produced);
	// (the windows are written already: no output is asked for, NXZ_CPS_NO_OUTPUT cannot occur)
	const nxz_checkpoint_stream_t s = nxz_cp_summary(&acc, cp_cap, format, hdr_len, st, uni(stop.cc), uni(stop.final_eob), produced, false, false);
	if (lane == 0) {
		streams[jid] = s;
		if (nxz_cp_has_sentinel(s.status)) {
			cb[s.count] = nxz_cp_bit(hdr_len, end_bit); uo[s.count] = produced;
			if (sta) sta[s.count] = nxz_cpf_state(0, 0, 0, 0);
		}
	}
}

} // namespace nxzcb

// n jobs, a wavefront each (order: NULL, or nxz_launch_order_by_length's); state NULL: checkpoints at block headers only
extern "C" int nxz_launch_checkpoint_build(int fmt, const nxz_batch_job_t *jobs, size_t n, uint64_t span, uint32_t cp_cap, uint64_t *cbit, uint64_t *uoff,
					   nxz_checkpoint_state_t *state, uint8_t *windows, nxz_checkpoint_stream_t *streams, const uint32_t *order,
					   hipStream_t stream)
{
	if (!n) return 0;
	hipLaunchKernelGGL(nxzcb::build_kernel, dim3((unsigned)n), dim3(64), 0, stream, fmt, jobs, order, span, cp_cap, cbit, uoff, state, windows, streams);
	return (int)hipGetLastError();
}
