// nxz_streams_part.hip -- the kernels around the compress batch of nxz_batch_deflate_streams_part (include/nxz_engine.h): a batch of
// streams written in PARTS, a device buffer a part, the stream's running state in a carry record on the device.  The rules are
// nxz_streams_part.h, the steps shared with the plain call (nxz_streams.hip) nxz_streams_dev.h; a block is laid into its part by
// pack_block (nxz_pack_block.h).  The call's shape is the plain call's, a kernel for a kernel, and one more:
//
//   prologue   a thread per stream: the carry (afresh with NXZ_PART_FIRST), the refusals, the header bytes with FIRST only, the
//              stream's running state seeded with the carry's checksums
//   expand     a thread per block of a chunk: the plain call's job, but for block 0 of a part with a window (h0 != 0): where the
//              window lies in front of the source in memory the job begins h0 bytes below it; else its source is a 64 KiB staging
//              slot -- slot q of the chunk, q the staged first blocks of the chunk in front of it (sg[]: the staged parts in front
//              of each stream, from the host's one pass) -- and the block is entered in the chunk's staging list
//   stage      a workgroup per entry of the list: [h0 window bytes][the block's source bytes] into the slot, 16 bytes a lane
//   -- nxz_batch_compress on those jobs --
//   layout     layout_stream with last = NXZ_PART_LAST of the stream
//   pack       pack_block with final = the stream's last block && NXZ_PART_LAST
//   epilogue   a thread per stream: the empty body and the trailer with LAST only, the carry written back, results[]
// A part that is refused on the device alone (no FIRST on a finished carry: the host cannot see the carry) has blocks in the
// batch's plan; they are compressed like any other -- its pointers have passed every other check -- and layout and pack pass over them.
#include <hip/hip_runtime.h>
#include "nxz_streams_dev.h"
#include "nxz_streams_part.h"
#include "nxz_shift_load.h"

namespace nxzsp {

using nxzst::owner_of;
using nxz::shift_bytes;

__device__ inline nxz_stream_job_t plain_job(const nxz_stream_part_job_t &j)
{
	nxz_stream_job_t p;
	p.src = j.src; p.dst = j.dst; p.src_len = j.src_len; p.dst_cap = j.dst_cap;
	return p;
}

__global__ __launch_bounds__(256) void prologue_kernel(const nxz_stream_part_job_t *__restrict__ desc, uint32_t n, uint32_t hist_max, int fmt, int level,
							 const nxz_stream_carry_t *__restrict__ carry, nxz_stream_state_t *__restrict__ state)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const nxz_stream_part_job_t j = desc[i];
	const nxz_stream_carry_t c = nxz_streams_part_carry_in(&carry[i], j.flags);
	uint8_t h[10];
	const uint32_t hl = j.flags & NXZ_PART_FIRST ? nxz_streams_header(fmt, level, h) : 0;
	nxz_stream_state_t st = nxzst::begin_stream(plain_job(j), nxz_streams_part_refusal(&j, c.status, hist_max, fmt), h, hl);
	st.crc = c.crc; st.adler = c.adler;
	state[i] = st;
}

// sg_b0: the staged first blocks of the batch in front of the chunk
__global__ __launch_bounds__(256) void expand_kernel(const nxz_stream_part_job_t *__restrict__ desc, const uint32_t *__restrict__ first,
						       const uint32_t *__restrict__ sg, uint32_t n, uint32_t b0, uint32_t m, uint32_t B, uint32_t H,
						       uint32_t hist_max, uint32_t sg_b0, uint8_t *__restrict__ slots, uint8_t *__restrict__ stage,
						       nxz_batch_job_t *__restrict__ jobs, uint32_t *__restrict__ owner, uint32_t *__restrict__ staged)
{
	const uint32_t t = blockIdx.x * 256 + threadIdx.x;
	if (t >= m) return;
	const uint32_t g = b0 + t, i = owner_of(first, n, g);
	const uint64_t k = g - first[i];
	const nxz_stream_part_job_t d = desc[i];
	const uint32_t h0 = nxz_streams_part_window(d.prev_len, hist_max);
	nxz_batch_job_t j = nxzst::block_job(plain_job(d), k, B, nxz_streams_part_block_window(k, B, H, h0), slots + (size_t)t * NXZ_STREAMS_SLOT);
	if (!k && nxz_streams_part_staged(&d, hist_max)) {
		const uint32_t q = sg[i] - sg_b0;
		j.src = stage + (size_t)q * NXZ_STREAMS_STAGE_SLOT;
		staged[q] = t;
	}
	jobs[t] = j;
	owner[t] = i;
}

// A workgroup of 256 per staged first block: slot <- [the last h0 bytes of prev][the block's source bytes].  The slot, h0 and the
// source are multiples of 16: the source moves in aligned 16-byte pieces (a tail below 16 bytes a byte a lane).  The window starts
// anywhere: 16-byte piece p of it lies in the two aligned pieces of `prev` that hold its first and its last byte -- both hold window
// bytes, so no load touches a piece that holds none -- and is put together from them by a byte shift.
__global__ __launch_bounds__(256) void stage_kernel(const nxz_stream_part_job_t *__restrict__ desc, const uint32_t *__restrict__ owner,
						      const uint32_t *__restrict__ staged, const nxz_batch_job_t *__restrict__ jobs)
{
	const uint32_t t = staged[blockIdx.x], tid = threadIdx.x;
	const nxz_stream_part_job_t d = desc[owner[t]];
	const nxz_batch_job_t j = jobs[t];
	const uint32_t h0 = j.hist_len, len = j.src_len - h0;
	uint8_t *const slot = const_cast<uint8_t *>(j.src);
	const uintptr_t w = (uintptr_t)d.prev + d.prev_len - h0;
	const uint32_t sh = (uint32_t)w & 15;
	const uint4 *const w4 = (const uint4 *)(w - sh);
	uint4 *const o4 = (uint4 *)slot;
	const uint32_t nw = h0 >> 4;
	if (sh == 0) {
		for (uint32_t p = tid; p < nw; p += 256) o4[p] = w4[p];
	} else {
		for (uint32_t p = tid; p < nw; p += 256) o4[p] = shift_bytes(w4[p], w4[p + 1], sh);
	}
	const uint4 *const s4 = (const uint4 *)d.src;
	uint4 *const b4 = (uint4 *)(slot + h0);
	const uint32_t ns = len >> 4;
	for (uint32_t p = tid; p < ns; p += 256) b4[p] = s4[p];
	for (uint32_t k = ns * 16 + tid; k < len; k += 256) slot[h0 + k] = d.src[k];
}

// One wavefront per stream of [i_lo, i_lo + gridDim.x), as nxz_streams.hip's layout_kernel; a part refused on the device keeps its state
__global__ __launch_bounds__(64) void layout_kernel(const nxz_stream_part_job_t *__restrict__ desc, const uint32_t *__restrict__ first, uint32_t i_lo,
							 uint32_t b0, uint32_t m, const nxz_batch_job_t *__restrict__ jobs,
							 const nxz_batch_result_t *__restrict__ results, uint32_t B, uint32_t op_block,
							 nxz_stream_state_t *__restrict__ state, uint64_t *__restrict__ offsets)
{
	const uint32_t i = i_lo + blockIdx.x;
	if (state[i].cc) return;
	nxzst::layout_stream(first, i, b0, m, jobs, results, B, op_block, state, offsets, (desc[i].flags & NXZ_PART_LAST) != 0);
}

__global__ __launch_bounds__(256) void pack_kernel(const nxz_stream_part_job_t *__restrict__ desc, const uint32_t *__restrict__ first,
						     const uint32_t *__restrict__ owner, uint32_t b0, const nxz_batch_job_t *__restrict__ jobs,
						     const nxz_batch_result_t *__restrict__ results, const uint64_t *__restrict__ offsets,
						     const nxz_stream_state_t *__restrict__ state)
{
	const uint32_t t = blockIdx.x, i = owner[t];
	if (state[i].cc) return;
	const bool final = b0 + t == first[i + 1] - 1 && (desc[i].flags & NXZ_PART_LAST);
	nxz::pack_block(jobs[t], results[t], final, desc[i].dst + offsets[t]);
}

__global__ __launch_bounds__(256) void epilogue_kernel(const nxz_stream_part_job_t *__restrict__ desc, const uint32_t *__restrict__ first, uint32_t n,
							 uint32_t hist_max, int fmt, const nxz_stream_state_t *__restrict__ state,
							 nxz_stream_carry_t *__restrict__ carry, nxz_stream_result_t *__restrict__ results)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const nxz_stream_part_job_t j = desc[i];
	const nxz_stream_state_t st = state[i];
	const nxz_stream_carry_t c = nxz_streams_part_carry_in(&carry[i], j.flags);
	const nxz_stream_result_t r = nxzst::finish_stream_at(plain_job(j), st, first[i + 1] - first[i], nxz_streams_part_bound(j.src_len, hist_max, fmt, j.flags),
							      fmt, (j.flags & NXZ_PART_LAST) != 0, c.total_in + j.src_len);
	if (!r.cc) carry[i] = nxz_streams_part_carry_out(&c, r.crc, r.adler, j.src_len, r.out_len, j.flags);
	results[i] = r;
}

} // namespace nxzsp

extern "C" int nxz_launch_streams_part_prologue(const nxz_stream_part_job_t *desc, uint32_t n, uint32_t hist_max, int fmt, int level,
						const nxz_stream_carry_t *carry, nxz_stream_state_t *state, hipStream_t stream)
{
	hipLaunchKernelGGL(nxzsp::prologue_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, desc, n, hist_max, fmt, level, carry, state);
	return (int)hipGetLastError();
}

extern "C" int nxz_launch_streams_part_expand(const nxz_stream_part_job_t *desc, const uint32_t *first, const uint32_t *sg, uint32_t n, uint32_t b0,
					      uint32_t m, uint32_t hist_max, uint32_t sg_b0, uint8_t *slots, uint8_t *stage, nxz_batch_job_t *jobs,
					      uint32_t *owner, uint32_t *staged, hipStream_t stream)
{
	const uint32_t H = nxz_streams_window(hist_max), B = nxz_streams_block_bytes(hist_max);
	hipLaunchKernelGGL(nxzsp::expand_kernel, dim3((m + 255) / 256), dim3(256), 0, stream, desc, first, sg, n, b0, m, B, H, hist_max, sg_b0, slots, stage,
			   jobs, owner, staged);
	return (int)hipGetLastError();
}

extern "C" int nxz_launch_streams_part_stage(const nxz_stream_part_job_t *desc, const uint32_t *owner, const uint32_t *staged, uint32_t ns,
					     const nxz_batch_job_t *jobs, hipStream_t stream)
{
	hipLaunchKernelGGL(nxzsp::stage_kernel, dim3(ns), dim3(256), 0, stream, desc, owner, staged, jobs);
	return (int)hipGetLastError();
}

extern "C" int nxz_launch_streams_part_layout(const nxz_stream_part_job_t *desc, const uint32_t *first, uint32_t i_lo, uint32_t streams, uint32_t b0,
					      uint32_t m, const nxz_batch_job_t *jobs, const nxz_batch_result_t *results, uint32_t hist_max,
					      uint32_t op_block, nxz_stream_state_t *state, uint64_t *offsets, hipStream_t stream)
{
	hipLaunchKernelGGL(nxzsp::layout_kernel, dim3(streams), dim3(64), 0, stream, desc, first, i_lo, b0, m, jobs, results,
			   nxz_streams_block_bytes(hist_max), op_block, state, offsets);
	return (int)hipGetLastError();
}

extern "C" int nxz_launch_streams_part_pack(const nxz_stream_part_job_t *desc, const uint32_t *first, const uint32_t *owner, uint32_t b0, uint32_t m,
					    const nxz_batch_job_t *jobs, const nxz_batch_result_t *results, const uint64_t *offsets,
					    const nxz_stream_state_t *state, hipStream_t stream)
{
	hipLaunchKernelGGL(nxzsp::pack_kernel, dim3(m), dim3(256), 0, stream, desc, first, owner, b0, jobs, results, offsets, state);
	return (int)hipGetLastError();
}

extern "C" int nxz_launch_streams_part_epilogue(const nxz_stream_part_job_t *desc, const uint32_t *first, uint32_t n, uint32_t hist_max, int fmt,
						const nxz_stream_state_t *state, nxz_stream_carry_t *carry, nxz_stream_result_t *results, hipStream_t stream)
{
	hipLaunchKernelGGL(nxzsp::epilogue_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, desc, first, n, hist_max, fmt, state, carry, results);
	return (int)hipGetLastError();
}
