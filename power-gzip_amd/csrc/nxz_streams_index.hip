// nxz_streams_index.hip -- the checkpoint index of nxz_batch_deflate_streams_indexed (include/nxz_engine.h), written while the streams
// are laid out: no stream is walked, the block headers are where layout put them.  The rules are nxz_streams_index.h; the kernels of
// nxz_streams.hip run as they are, these go beside them on the same stream (nxz_batch_streams.cpp queues them):
//
//   prologue   (behind the plain prologue) a thread per stream: checkpoint 0, which always stands behind the framing's header, and the
//              stream's running index state -- or `on = 0` for a stream that gets no index (refused, or too long for the row format)
//   sweep      (behind layout, the same grid) a wavefront per stream the chunk touches, its blocks 64 at a time, a lane a block: every
//              lane forms its piece's one or two headers; the wavefront finds the next checkpoint with a ballot for the first header
//              with u - c >= span -- one step per checkpoint found, not per block -- stores it while the row has room and counts it
//              anyway.  (c, count) go on to the stream's next chunk through the state: the index does not depend on the chunk size.
//              With windows the lane notes which slot each of its two headers got (marks[2 t], marks[2 t + 1]; NXZ_SI_NONE: none).
//   windows    (beside pack, the same grid: the chunk's block count is all the host knows) a workgroup per block: the
//              min(uoff, 32768) source bytes in front of each marked header into its slot.  u = k * B in a 16-byte aligned source
//              and a 16-byte aligned slot: 16 bytes a lane, a wavefront a KiB at a time.  Any other alignment (the second header of a
//              stored piece stands at u0 + 65535): dwords into the slot, each put together from two aligned dwords of the source
//              with alignbyte, as pack_block does it.
//   epilogue   (behind the plain epilogue) a thread per stream: the sentinel, streams[i] and index_jobs[i] from the final state and
//              results[i].
#include <hip/hip_runtime.h>
#include "nxz_device.h"
#include "nxz_streams_index.h"
#include "nxz_pack_block.h"

namespace nxzsi {

__global__ __launch_bounds__(256) void prologue_kernel(const nxz_stream_job_t *__restrict__ desc, uint32_t n, int fmt,
							 const nxz_stream_state_t *__restrict__ state, uint32_t cp_cap, uint64_t *__restrict__ cbit,
							 uint64_t *__restrict__ uoff, nxz_stream_index_state_t *__restrict__ ist)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const uint32_t hl = nxz_streams_header_len(fmt);
	nxz_stream_index_state_t o;
	o.c = 0; o.end_bit = nxz_si_empty_end_bit(hl); o.count = 0; o.on = 0;
	if (!state[i].cc && nxz_si_len_ok(desc[i].src_len)) {
		const size_t row = (size_t)i * ((size_t)cp_cap + 1);
		cbit[row] = nxz_si_first_bit(hl); uoff[row] = 0;                  // (cp_cap >= 1: checkpoint 0 is always stored)
		o.count = 1; o.on = 1;
	}
	ist[i] = o;
}

// One wavefront per stream of [i_lo, i_lo + gridDim.x), the stream's blocks inside the chunk [b0, b0 + m): layout_kernel's grid and
// its loop.  The headers of 64 pieces stand in stream order as lane 0's first, lane 0's second, lane 1's first, ...; their u never
// decreases, so the first header the rule takes is the lowest lane's among the first headers, or among the second ones, whichever
// comes first -- and every header in front of it has u <= c afterwards and is never asked again.
__global__ __launch_bounds__(64) void sweep_kernel(const uint32_t *__restrict__ first, uint32_t i_lo, uint32_t b0, uint32_t m,
						     const nxz_batch_job_t *__restrict__ jobs, const nxz_batch_result_t *__restrict__ results,
						     const uint64_t *__restrict__ offsets, uint32_t B, uint64_t span, uint32_t cp_cap,
						     uint64_t *__restrict__ cbit, uint64_t *__restrict__ uoff, nxz_stream_index_state_t *__restrict__ ist,
						     uint32_t *__restrict__ marks)
{
	const uint32_t i = i_lo + blockIdx.x, lane = threadIdx.x;
	const uint32_t f0 = first[i], f1 = first[i + 1];
	const uint32_t lo = f0 > b0 ? f0 : b0, hi = f1 < b0 + m ? f1 : b0 + m;
	if (lo >= hi) return;
	const nxz_stream_index_state_t st = ist[i];
	if (!st.on) {                                                           // no index: its blocks' headers get no slot
		if (marks)
			for (uint32_t g = lo + lane; g < hi; g += 64) { marks[2 * (g - b0)] = NXZ_SI_NONE; marks[2 * (g - b0) + 1] = NXZ_SI_NONE; }
		return;
	}
	uint64_t *const cb = cbit + (size_t)i * ((size_t)cp_cap + 1), *const uo = uoff + (size_t)i * ((size_t)cp_cap + 1);
	nxz_cp_acc_t acc;
	acc.count = st.count; acc.last_uoff = st.c;
	for (uint32_t i0 = lo; i0 < hi; i0 += 64) {
		const uint32_t g = i0 + lane;
		const bool valid = g < hi;
		uint64_t bit[2] = {0, 0}, u[2] = {0, 0};
		uint32_t nh = 0, slot[2] = {NXZ_SI_NONE, NXZ_SI_NONE};
		if (valid) {
			const nxz_batch_result_t r = results[g - b0];
			const bool final = g == f1 - 1;
			const nxz::StreamPiece sp = nxz::stream_piece(jobs[g - b0], r, final);
			nxz_si_piece_t p;
			p.stored = sp.stored; p.len = sp.len; p.keep = sp.keep; p.tebc = r.tebc; p.final = final;
			const uint64_t P = offsets[g - b0];
			nh = nxz_si_headers(&p, P, nxz_streams_block_start(g - f0, B), bit, u);
			if (final) ist[i].end_bit = nxz_si_end_bit(&p, P);                // (lane 0 below writes the other fields only)
		}
		for (;;) {
			const uint64_t q0 = __ballot(nh >= 1 && nxz_si_takes(u[0], acc.last_uoff, span));
			const uint64_t q1 = __ballot(nh == 2 && nxz_si_takes(u[1], acc.last_uoff, span));
			if (!(q0 | q1)) break;
			const uint32_t l0 = q0 ? (uint32_t)__builtin_ctzll(q0) : 64, l1 = q1 ? (uint32_t)__builtin_ctzll(q1) : 64;
			const uint32_t h = l0 <= l1 ? 0 : 1, from = h ? l1 : l0;          // lane l's first header stands in front of its second
			const uint64_t ut = __shfl(h ? u[1] : u[0], from);
			const uint32_t k = nxz_cp_add(&acc, ut, cp_cap);
			if (lane == from && k < cp_cap) {
				cb[k] = h ? bit[1] : bit[0]; uo[k] = ut;
				slot[h] = k;
			}
		}
		if (marks && valid) { marks[2 * (g - b0)] = slot[0]; marks[2 * (g - b0) + 1] = slot[1]; }
	}
	if (lane == 0) { ist[i].c = acc.last_uoff; ist[i].count = acc.count; }
}

// d[0, len) <- s[0, len) by a workgroup of 256
__device__ inline void copy_window(uint8_t *__restrict__ d, const uint8_t *__restrict__ s, uint32_t len, uint32_t t)
{
	if ((((uintptr_t)d | (uintptr_t)s) & 15) == 0) {
		const uint32_t n16 = len >> 4;
		const uint4 *s4 = (const uint4 *)s;
		uint4 *d4 = (uint4 *)d;
		for (uint32_t g = t; g < n16; g += 256) d4[g] = s4[g];
		for (uint32_t k = n16 * 16 + t; k < len; k += 256) d[k] = s[k];
		return;
	}
	uint32_t head = (uint32_t)((4 - ((uintptr_t)d & 3)) & 3);
	if (head > len) head = len;
	const uint32_t nd = (len - head) >> 2;
	if (t < head) d[t] = s[t];
	for (uint32_t k = head + nd * 4 + t; k < len; k += 256) d[k] = s[k];
	uint32_t *od = (uint32_t *)(d + head);
	for (uint32_t w = t; w < nd; w += 256) {
		// the two aligned dwords that hold source bytes [a, a + 4): both share a dword with a byte of the window
		const uintptr_t a = (uintptr_t)s + head + 4 * (uintptr_t)w;
		const uint32_t *q = (const uint32_t *)(a & ~(uintptr_t)3);
		const uint32_t bo = (uint32_t)a & 3;
		const uint32_t lo = q[0], hi = bo ? q[1] : 0;
		od[w] = __builtin_amdgcn_alignbyte(hi, lo, bo);
	}
}

__global__ __launch_bounds__(256) void window_kernel(const nxz_stream_job_t *__restrict__ desc, const uint32_t *__restrict__ owner,
						       const uint32_t *__restrict__ marks, uint32_t cp_cap, const uint64_t *__restrict__ uoff,
						       uint8_t *__restrict__ windows)
{
	const uint32_t t = blockIdx.x;
	for (uint32_t h = 0; h < 2; h++) {
		const uint32_t k = marks[2 * t + h];
		if (k >= cp_cap) continue;                                          // (NXZ_SI_NONE; a stored checkpoint's slot is below cp_cap)
		const uint32_t i = owner[t];
		const nxz_stream_job_t j = desc[i];
		const uint64_t u = uoff[(size_t)i * ((size_t)cp_cap + 1) + k];
		if (u > j.src_len) continue;                                        // (never: the sweep wrote it from the same plan)
		const uint32_t w = nxz_cp_window_len(u);
		copy_window(windows + ((size_t)i * cp_cap + k) * NXZ_CP_WINDOW, j.src + (u - w), w, threadIdx.x);
	}
}

__global__ __launch_bounds__(256) void epilogue_kernel(const nxz_stream_job_t *__restrict__ desc, uint32_t n, int fmt,
							 const nxz_stream_result_t *__restrict__ results,
							 const nxz_stream_index_state_t *__restrict__ ist, uint32_t cp_cap, uint64_t *__restrict__ cbit,
							 uint64_t *__restrict__ uoff, nxz_checkpoint_stream_t *__restrict__ streams,
							 nxz_batch_job_t *__restrict__ index_jobs)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const nxz_stream_job_t j = desc[i];
	const nxz_stream_result_t r = results[i];
	const nxz_stream_index_state_t st = ist[i];
	const bool indexed = !r.cc && st.on && nxz_si_len_ok(r.out_len);
	if (!indexed) {
		streams[i] = nxz_si_no_index(r.cc);
	} else {
		const nxz_checkpoint_stream_t s = nxz_si_summary(st.count, cp_cap, fmt, j.src_len);
		streams[i] = s;
		if (nxz_cp_has_sentinel(s.status)) {
			const size_t row = (size_t)i * ((size_t)cp_cap + 1);
			cbit[row + s.count] = st.end_bit; uoff[row + s.count] = j.src_len;
		}
	}
	if (index_jobs) index_jobs[i] = nxz_si_reader_job(j.dst, r.out_len, indexed);
}

} // namespace nxzsi

extern "C" int nxz_launch_streams_index_prologue(const nxz_stream_job_t *desc, uint32_t n, int fmt, const nxz_stream_state_t *state, uint32_t cp_cap,
						 uint64_t *cbit, uint64_t *uoff, nxz_stream_index_state_t *ist, hipStream_t stream)
{
	hipLaunchKernelGGL(nxzsi::prologue_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, desc, n, fmt, state, cp_cap, cbit, uoff, ist);
	return (int)hipGetLastError();
}

extern "C" int nxz_launch_streams_index_sweep(const uint32_t *first, uint32_t i_lo, uint32_t streams, uint32_t b0, uint32_t m,
					      const nxz_batch_job_t *jobs, const nxz_batch_result_t *results, const uint64_t *offsets,
					      uint32_t hist_max, uint64_t span, uint32_t cp_cap, uint64_t *cbit, uint64_t *uoff,
					      nxz_stream_index_state_t *ist, uint32_t *marks, hipStream_t stream)
{
	hipLaunchKernelGGL(nxzsi::sweep_kernel, dim3(streams), dim3(64), 0, stream, first, i_lo, b0, m, jobs, results, offsets,
			   nxz_streams_block_bytes(hist_max), span, cp_cap, cbit, uoff, ist, marks);
	return (int)hipGetLastError();
}

extern "C" int nxz_launch_streams_index_windows(const nxz_stream_job_t *desc, const uint32_t *owner, uint32_t m, const uint32_t *marks,
						uint32_t cp_cap, const uint64_t *uoff, uint8_t *windows, hipStream_t stream)
{
	hipLaunchKernelGGL(nxzsi::window_kernel, dim3(m), dim3(256), 0, stream, desc, owner, marks, cp_cap, uoff, windows);
	return (int)hipGetLastError();
}

extern "C" int nxz_launch_streams_index_epilogue(const nxz_stream_job_t *desc, uint32_t n, int fmt, const nxz_stream_result_t *results,
						 const nxz_stream_index_state_t *ist, uint32_t cp_cap, uint64_t *cbit, uint64_t *uoff,
						 nxz_checkpoint_stream_t *streams, nxz_batch_job_t *index_jobs, hipStream_t stream)
{
	hipLaunchKernelGGL(nxzsi::epilogue_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, desc, n, fmt, results, ist, cp_cap, cbit, uoff,
			   streams, index_jobs);
	return (int)hipGetLastError();
}
