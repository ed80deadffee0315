// nxz_streams_dict.hip -- what nxz_batch_deflate_streams_dict (include/nxz_engine.h) runs in place of nxz_streams.hip's prologue, expand
// and epilogue: a batch of device buffers of any length, each written as ONE raw or zlib stream whose first block has the tail of a
// shared preset dictionary as its window.  The rules are nxz_streams_dict.h, the steps shared with the plain call nxz_streams_dev.h;
// layout and pack are nxz_streams.hip's own kernels, which see one array of blocks in the batch's order as ever.
//
//   prologue   a thread per stream: refusals against the dictionary form's bound, the six header bytes (FDICT, DICTID)
//   expand     a thread per block of a chunk.  A stream's first block becomes a dictionary job as nxzl77::dict_jobs_kernel writes them
//              (src moved down by h0, hist_len = h0: NOTHING reads below src + hist_len, the LZ77 kernel takes those bytes from the
//              dictionary), every other block a plain history job.  The LZ77 kernel takes a window from the dictionary for ALL jobs of
//              a launch or for none, and indexes jobs, tokens and results by the job's place in the launch.  So the chunk's jobs are
//              written twice: in the batch's order for layout and pack, and in LAUNCH order -- the chunk's first blocks in front, the
//              rest behind, each kind in the batch's order -- for the compress batch, which then is two LZ77 launches over the two
//              parts and one table and one entropy launch over both.  pos[t] is block t's place in the launch order.
//   -- the compress batch on the launch order (nxz_batch.cpp: batch_compress_windowed) --
//   gather     a thread per block: its result from its place in the launch order to its own index
//   -- nxz_streams.hip: layout, pack --
//   epilogue   a thread per stream: as the plain call's, a refused stream is told the dictionary form's bound
#include "nxz_streams_dev.h"
#include "nxz_streams_dict.h"

namespace nxzst {

__global__ __launch_bounds__(256) void prologue_dict_kernel(const nxz_stream_job_t *__restrict__ desc, uint32_t n, uint32_t hist_max, int fmt, int level,
							      uint32_t dictid, nxz_stream_state_t *__restrict__ state)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const nxz_stream_job_t j = desc[i];
	uint8_t h[6];
	const uint32_t hl = nxz_streams_dict_header(fmt, level, dictid, h);
	state[i] = begin_stream(j, nxz_streams_dict_refusal(&j, hist_max, fmt), h, hl);
}

// nz[i]: the streams in front of stream i that have blocks, so nz[i] + (k != 0) first blocks of the batch lie in front of block k of
// stream i; nz_b0 of them in front of the chunk, nf inside it (the host knows both from its pass over the streams).
__global__ __launch_bounds__(256) void expand_dict_kernel(const nxz_stream_job_t *__restrict__ desc, const uint32_t *__restrict__ first,
							    const uint32_t *__restrict__ nz, uint32_t n, uint32_t b0, uint32_t m, uint32_t B, uint32_t H,
							    uint32_t h0, uint32_t nz_b0, uint32_t nf, uint8_t *__restrict__ slots,
							    nxz_batch_job_t *__restrict__ jobs, nxz_batch_job_t *__restrict__ ljobs,
							    uint32_t *__restrict__ owner, uint32_t *__restrict__ pos)
{
	const uint32_t t = blockIdx.x * 256 + threadIdx.x;
	if (t >= m) return;
	const uint32_t g = b0 + t, i = owner_of(first, n, g);
	const uint64_t k = g - first[i];
	const nxz_batch_job_t j = block_job(desc[i], k, B, nxz_streams_dict_block_window(k, B, H, h0), slots + (size_t)t * NXZ_STREAMS_SLOT);
	const uint32_t before = nxz_streams_dict_firsts_before(nz[i], k) - nz_b0;   // the chunk's first blocks in front of this block
	const uint32_t p = nxz_streams_dict_launch_pos(t, k, before, nf);
	jobs[t] = j;
	ljobs[p] = j;
	owner[t] = i;
	pos[t] = p;
}

__global__ __launch_bounds__(256) void gather_results_kernel(const nxz_batch_result_t *__restrict__ lresults, const uint32_t *__restrict__ pos, uint32_t m,
							       nxz_batch_result_t *__restrict__ results)
{
	const uint32_t t = blockIdx.x * 256 + threadIdx.x;
	if (t < m) results[t] = lresults[pos[t]];
}

__global__ __launch_bounds__(256) void epilogue_dict_kernel(const nxz_stream_job_t *__restrict__ desc, const uint32_t *__restrict__ first, uint32_t n,
							      uint32_t hist_max, int fmt, const nxz_stream_state_t *__restrict__ state,
							      nxz_stream_result_t *__restrict__ results)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const nxz_stream_job_t j = desc[i];
	results[i] = finish_stream(j, state[i], first[i + 1] - first[i], nxz_streams_dict_bound(j.src_len, hist_max, fmt), fmt);
}

} // namespace nxzst

extern "C" int nxz_launch_streams_dict_prologue(const nxz_stream_job_t *desc, uint32_t n, uint32_t hist_max, int fmt, int level, uint32_t dictid,
						nxz_stream_state_t *state, hipStream_t stream)
{
	hipLaunchKernelGGL(nxzst::prologue_dict_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, desc, n, hist_max, fmt, level, dictid, state);
	return (int)hipGetLastError();
}

extern "C" int nxz_launch_streams_dict_expand(const nxz_stream_job_t *desc, const uint32_t *first, const uint32_t *nz, uint32_t n, uint32_t b0,
					      uint32_t m, uint32_t hist_max, uint32_t h0, uint32_t nz_b0, uint32_t nf, uint8_t *slots,
					      nxz_batch_job_t *jobs, nxz_batch_job_t *ljobs, uint32_t *owner, uint32_t *pos, hipStream_t stream)
{
	const uint32_t H = nxz_streams_window(hist_max), B = nxz_streams_block_bytes(hist_max);
	hipLaunchKernelGGL(nxzst::expand_dict_kernel, dim3((m + 255) / 256), dim3(256), 0, stream, desc, first, nz, n, b0, m, B, H, h0, nz_b0, nf,
			   slots, jobs, ljobs, owner, pos);
	return (int)hipGetLastError();
}

extern "C" int nxz_launch_streams_dict_gather(const nxz_batch_result_t *lresults, const uint32_t *pos, uint32_t m, nxz_batch_result_t *results,
					      hipStream_t stream)
{
	hipLaunchKernelGGL(nxzst::gather_results_kernel, dim3((m + 255) / 256), dim3(256), 0, stream, lresults, pos, m, results);
	return (int)hipGetLastError();
}

extern "C" int nxz_launch_streams_dict_epilogue(const nxz_stream_job_t *desc, const uint32_t *first, uint32_t n, uint32_t hist_max, int fmt,
						const nxz_stream_state_t *state, nxz_stream_result_t *results, hipStream_t stream)
{
	hipLaunchKernelGGL(nxzst::epilogue_dict_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, desc, first, n, hist_max, fmt, state, results);
	return (int)hipGetLastError();
}
