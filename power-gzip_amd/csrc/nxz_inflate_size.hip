// nxz_inflate_size.hip -- how large is the output?  The walk behind nxz_batch_decompress_size / _size_framed (gfx950, wave64).
//
// A decode needs a target the caller has sized; raw deflate and zlib streams carry no length and gzip's ISIZE is modulo 2^32
// and not to be trusted.  This kernel walks a stream as the stream-per-wavefront decoder does (nxz_inflate.hip: block headers,
// decode tables, the multi-token step) and counts the bytes every token would make -- no window, no match copies, no stores to
// dst, no checksum pass.  One nxz_batch_result_t per stream comes back, field for field what the decode would report for a
// target of dst_cap bytes (nxz_size.h holds the arithmetic: the fit against dst_cap, the reach of a distance, the record).
//
// Shape: one stream per wavefront, one wavefront per workgroup.  LDS per stream is the tables, the stage of the one-token path
// and the code lengths of a header: 6.5 KiB, so 24 streams fit a CU's 160 KiB where the decoder with its window in LDS holds 4
// (39.5 KiB) and the workgroup decoder one (161 KiB).  Registers allow six wavefronts a SIMD at 80 VGPRs, which the kernel keeps
// to: 24 streams a CU by registers too.  (Several wavefronts per workgroup would not raise that -- LDS and registers bound it, not the
// number of workgroups -- and the shared helpers of nxz_inflate_decode.h order their LDS traffic with the barrier of a
// one-wavefront workgroup, which costs nothing.)  Long streams start first (nxz_launch_order_by_length): a launch ends with
// its slowest stream.
//
// The walk itself is nxzs::walk (nxz_inflate_walk.h), which nxz_gzip_members.hip runs member after member.  Differences to the
// decoder's walk:
//   - src may have any alignment: the two 256-byte blocks of the source that the multi-token step keeps in registers are loaded
//     as dwords from the 4-byte boundary at or below src, and every bit position is taken `skew` bytes further on.  (The decoder
//     leaves such a source to its one-token path; here framed streams -- two header bytes in front -- are the common case.)
//   - the output count may come close to 2^32 (dst_cap = 0xffffffff: no limit): sums are taken in 64 bits (nxz_size.h).
//   - resume state and NXZ_JOB_SUSPEND_WHEN_FULL are not honoured, no dht_io is written.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "nxz_device.h"
#include "nxz_frame.h"
#include "nxz_inflate_walk.h"

namespace nxzs {

// sh_len: how far the distances of every job may reach in front of its output besides its own hist_len -- the inflate window of
// the dictionary of nxz_batch_decompress_size_framed, 0 otherwise; a job that says NXZ_JOB_NO_DICT does not get it.
// (The compiler is told six wavefronts a SIMD: left to itself it takes 81 registers, one more than six allow.)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(6))) void size_kernel(const nxz_batch_job_t *__restrict__ jobs,
		nxz_batch_result_t *__restrict__ results, const uint32_t *__restrict__ order, uint32_t sh_len)
{
	__shared__ __attribute__((aligned(16))) Smem sm;
	const int lane = threadIdx.x;
	const uint32_t jid = order ? order[blockIdx.x] : blockIdx.x;
	const nxz_batch_job_t job = jobs[jid];
	if (!nxz_size_job_ok(job.resume, job.hist_len)) {
		if (lane == 0) results[jid] = nxz_size_refused();
		return;
	}
	const uint32_t hist_bytes = nxz_size_hist_bytes(job.hist_len, job.src_len);
	uint32_t hist = hist_bytes + ((job.reserved & NXZ_JOB_NO_DICT) ? 0 : sh_len);
	if (hist > NXZ_SIZE_WINDOW) hist = NXZ_SIZE_WINDOW;
	const uint32_t srclen = job.src_len - hist_bytes;
	const NXZ_GLOBAL_AS uint8_t *src = (const NXZ_GLOBAL_AS uint8_t *)job.src + hist_bytes;
	const uint32_t cap = job.dst_cap;

	nxz_size_stop_t stop = {};
	uint64_t end_bit;
	walk(sm, src, srclen, cap, hist, lane, stop, end_bit);
	if (lane == 0) results[jid] = nxz_size_record(&stop, job.src_len);
}

// The trailer step of nxz_batch_decompress_size_framed, a thread a job: nxz_frame.h's trailer rule, as nxz_frame.hip's
// frame_trailer_kernel runs it, without the comparison of the checksum -- the walk has none to compare.
__global__ __launch_bounds__(256) void size_trailer_kernel(const nxz_batch_job_t *__restrict__ jobs, uint32_t n,
							   nxz_batch_result_t *__restrict__ results, nxz_batch_frame_t *__restrict__ frames)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	nxz_batch_frame_t *f = &frames[i];
	if (f->status != NXZ_FRAME_OK) {
		results[i] = nxz_size_refused();
		return;
	}
	const nxz_batch_result_t r = results[i];
	const nxz_batch_job_t job = jobs[i];
	uint32_t end, check, isize;
	const uint32_t st = nxz_frame_trailer(f->format, f->hdr_len, &r, job.src, job.src_len, false, &end, &check, &isize);
	f->status = st; f->end = end; f->check = check; f->isize = isize;
}

} // namespace nxzs

// n jobs, a wavefront each; order: NULL, or nxz_launch_order_by_length's; dict_window: see size_kernel's sh_len
extern "C" int nxz_launch_inflate_size(const nxz_batch_job_t *jobs, size_t n, nxz_batch_result_t *results, const uint32_t *order,
				       uint32_t dict_window, hipStream_t stream)
{
	if (!n) return 0;
	hipLaunchKernelGGL(nxzs::size_kernel, dim3((unsigned)n), dim3(64), 0, stream, jobs, results, order, dict_window);
	return (int)hipGetLastError();
}

extern "C" int nxz_launch_size_trailer(const nxz_batch_job_t *jobs, size_t n, nxz_batch_result_t *results, nxz_batch_frame_t *frames, hipStream_t stream)
{
	if (!n) return 0;
	hipLaunchKernelGGL(nxzs::size_trailer_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, jobs, (uint32_t)n, results, frames);
	return (int)hipGetLastError();
}
