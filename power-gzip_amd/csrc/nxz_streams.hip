// nxz_streams.hip -- the kernels around the compress batch of nxz_batch_deflate_streams (include/nxz_engine.h): a batch of device
// buffers of any length, each written as ONE raw, zlib or gzip stream.  The rules (block plan, bound, framing, checksum joins) are
// nxz_streams.h, the steps shared with the dictionary form (nxz_streams_dict.hip) nxz_streams_dev.h; a block is laid into its stream by pack_block (nxz_pack_block.h), as nxz_deflate_host's kernels lay theirs.
//
//   prologue   a thread per stream: refusals, the header bytes, the stream's running state
//   expand     a thread per block of a chunk: whose block it is (upper bound in the streams' block prefix), its compress job
//   -- nxz_batch_compress on those jobs --
//   layout     a wavefront per stream the chunk touches: where each of its blocks goes (exclusive prefix of the pieces' sizes,
//              continued from the stream's `written`), CRC-32 and Adler-32 of the chunk's part joined onto the stream's
//   pack       a workgroup per block: pack_block
//   epilogue   a thread per stream: the empty streams' body, the trailers, results[]
// A stream is indexed by a uint32_t everywhere (a batch holds fewer than 2^31 streams and blocks).
#include <hip/hip_runtime.h>
#include "nxz_streams_dev.h"
#include "nxz_pack_block.h"

namespace nxzst {

__global__ __launch_bounds__(256) void prologue_kernel(const nxz_stream_job_t *__restrict__ desc, uint32_t n, uint32_t hist_max, int fmt, int level,
							 nxz_stream_state_t *__restrict__ state)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const nxz_stream_job_t j = desc[i];
	uint8_t h[10];
	const uint32_t hl = nxz_streams_header(fmt, level, h);
	state[i] = begin_stream(j, nxz_streams_refusal(&j, hist_max, fmt), h, hl);
}

__global__ __launch_bounds__(256) void expand_kernel(const nxz_stream_job_t *__restrict__ desc, const uint32_t *__restrict__ first, uint32_t n,
						       uint32_t b0, uint32_t m, uint32_t B, uint32_t H, uint8_t *__restrict__ slots,
						       nxz_batch_job_t *__restrict__ jobs, uint32_t *__restrict__ owner)
{
	const uint32_t t = blockIdx.x * 256 + threadIdx.x;
	if (t >= m) return;
	const uint32_t g = b0 + t, i = owner_of(first, n, g);
	const uint64_t k = g - first[i];
	jobs[t] = block_job(desc[i], k, B, nxz_streams_block_window(k, B, H), slots + (size_t)t * NXZ_STREAMS_SLOT);
	owner[t] = i;
}

// One wavefront per stream of [i_lo, i_lo + gridDim.x): layout_stream (nxz_streams_dev.h); a stream's last block is the final one.
__global__ __launch_bounds__(64) void layout_kernel(const uint32_t *__restrict__ first, uint32_t i_lo, uint32_t b0, uint32_t m,
						      const nxz_batch_job_t *__restrict__ jobs, const nxz_batch_result_t *__restrict__ results,
						      uint32_t B, uint32_t op_block, nxz_stream_state_t *__restrict__ state, uint64_t *__restrict__ offsets)
{
	layout_stream(first, i_lo + blockIdx.x, b0, m, jobs, results, B, op_block, state, offsets, true);
}

__global__ __launch_bounds__(256) void pack_kernel(const nxz_stream_job_t *__restrict__ desc, const uint32_t *__restrict__ first,
						     const uint32_t *__restrict__ owner, uint32_t b0, const nxz_batch_job_t *__restrict__ jobs,
						     const nxz_batch_result_t *__restrict__ results, const uint64_t *__restrict__ offsets)
{
	const uint32_t t = blockIdx.x, i = owner[t];
	nxz::pack_block(jobs[t], results[t], b0 + t == first[i + 1] - 1, desc[i].dst + offsets[t]);
}

__global__ __launch_bounds__(256) void epilogue_kernel(const nxz_stream_job_t *__restrict__ desc, const uint32_t *__restrict__ first, uint32_t n,
							 uint32_t hist_max, int fmt, const nxz_stream_state_t *__restrict__ state,
							 nxz_stream_result_t *__restrict__ results)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const nxz_stream_job_t j = desc[i];
	results[i] = finish_stream(j, state[i], first[i + 1] - first[i], nxz_streams_bound(j.src_len, hist_max, fmt), fmt);
}

} // namespace nxzst

extern "C" int nxz_launch_streams_prologue(const nxz_stream_job_t *desc, uint32_t n, uint32_t hist_max, int fmt, int level,
					   nxz_stream_state_t *state, hipStream_t stream)
{
	hipLaunchKernelGGL(nxzst::prologue_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, desc, n, hist_max, fmt, level, state);
	return (int)hipGetLastError();
}

extern "C" int nxz_launch_streams_expand(const nxz_stream_job_t *desc, const uint32_t *first, uint32_t n, uint32_t b0, uint32_t m,
					 uint32_t hist_max, uint8_t *slots, nxz_batch_job_t *jobs, uint32_t *owner, hipStream_t stream)
{
	const uint32_t H = nxz_streams_window(hist_max), B = nxz_streams_block_bytes(hist_max);
	hipLaunchKernelGGL(nxzst::expand_kernel, dim3((m + 255) / 256), dim3(256), 0, stream, desc, first, n, b0, m, B, H, slots, jobs, owner);
	return (int)hipGetLastError();
}

extern "C" int nxz_launch_streams_layout(const uint32_t *first, uint32_t i_lo, uint32_t streams, uint32_t b0, uint32_t m,
					 const nxz_batch_job_t *jobs, const nxz_batch_result_t *results, uint32_t hist_max, uint32_t op_block,
					 nxz_stream_state_t *state, uint64_t *offsets, hipStream_t stream)
{
	hipLaunchKernelGGL(nxzst::layout_kernel, dim3(streams), dim3(64), 0, stream, first, i_lo, b0, m, jobs, results,
			   nxz_streams_block_bytes(hist_max), op_block, state, offsets);
	return (int)hipGetLastError();
}

extern "C" int nxz_launch_streams_pack(const nxz_stream_job_t *desc, const uint32_t *first, const uint32_t *owner, uint32_t b0, uint32_t m,
				       const nxz_batch_job_t *jobs, const nxz_batch_result_t *results, const uint64_t *offsets, hipStream_t stream)
{
	hipLaunchKernelGGL(nxzst::pack_kernel, dim3(m), dim3(256), 0, stream, desc, first, owner, b0, jobs, results, offsets);
	return (int)hipGetLastError();
}

extern "C" int nxz_launch_streams_epilogue(const nxz_stream_job_t *desc, const uint32_t *first, uint32_t n, uint32_t hist_max, int fmt,
					   const nxz_stream_state_t *state, nxz_stream_result_t *results, hipStream_t stream)
{
	hipLaunchKernelGGL(nxzst::epilogue_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, desc, first, n, hist_max, fmt, state, results);
	return (int)hipGetLastError();
}
