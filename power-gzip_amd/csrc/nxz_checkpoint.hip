// nxz_checkpoint.hip -- checkpoints inside raw, zlib and gzip streams (nxz_batch_checkpoint_index / nxz_checkpoint_read_ranges;
// gfx950, wave64).  The rules are nxz_checkpoint.h's; here is the bit-walking and the plumbing.  No decoder of its own: the index
// is the size walk (nxz_inflate_walk.h) with a hook at every block header, and a range read decodes its segments with
// nxz_batch_decompress as jobs [window][source bytes] that resume inside a byte.
//
// The index, all on the caller's stream (nxz_batch_ranges.cpp queues it, nothing waits for the host):
//   index_kernel     one job per wavefront, one wavefront per workgroup, the long jobs first -- the shape of the size query
//                    (nxz_inflate_size.hip) and of the member index (nxz_gzip_members.hip): the header by nxz_frame.h's parser, every
//                    lane on the same bytes, then nxzs::walk, whose hook applies the checkpoint rule and stores the entry from lane 0;
//                    the stream's record and the sentinel last.  LDS is the walk's; the accumulator lives in scalar registers.
//   window_kernel    a workgroup per stored checkpoint (grid-stride): the min(uoff, 32768) bytes in front of uoff[k] from the job's
//                    decoded output to the start of the checkpoint's slot, 16 bytes a lane where the slot's alignment allows.
// A range read (nxz_batch_ranges.cpp runs the steps and waits once, after the map -- the shape of nxz_bgzf_read_ranges, whose map, gather
// and zero kernels it uses as they are: nxz_bgzf.hip):
//   check_kernel     a thread an entry: nxz_cp_entry_ok; any fault sets ctl[0] and every later kernel writes nothing
//   (the range map and the scans of nxz_bgzf.hip over uoff: needed segments, each once, their list)
//   inmax_kernel     a thread a segment: the largest [window][source bytes] among the needed ones (ctl[5]: the input slots' stride)
//   stage_kernel     a workgroup per needed segment of the chunk and per 64 KiB of its input: window and source bytes into the
//                    segment's input slot, the source bytes starting at a 16-byte boundary (the decoder's fast loads want the
//                    stream aligned; the window in front of it is read byte by byte); the first workgroup writes the job record
//   (nxz_batch_decompress on those jobs)
//   verdict_kernel   a thread a segment: nxz_cp_segment_good -> frames[k].status, which the BGZF gather looks at
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "nxz_device.h"
#include "nxz_frame.h"
#include "nxz_frame_wave.h"
#include "nxz_inflate_walk.h"
#include "nxz_checkpoint.h"

namespace nxzcp {

using nxzi::uni;

// what the walk calls at every block header: the checkpoint rule, the entry from lane 0 while there is room
struct Hook {
	nxz_cp_acc_t *acc;
	uint64_t *cbit, *uoff;
	uint64_t span;
	uint32_t cp_cap, hdr_len;
	int lane;
	__device__ __forceinline__ void operator()(uint64_t bit, uint32_t out) const
	{
		const uint32_t u = uni(out);
		if (!nxz_cp_is_checkpoint(acc, u, span)) return;
		const uint32_t k = nxz_cp_add(acc, u, cp_cap);
		if (k < cp_cap && lane == 0) { cbit[k] = nxz_cp_bit(hdr_len, bit); uoff[k] = u; }
	}
};

__global__ __launch_bounds__(64) void index_kernel(int fmt, const nxz_batch_job_t *__restrict__ jobs, const uint32_t *__restrict__ order, uint64_t span,
						   uint32_t cp_cap, uint64_t *__restrict__ cbit, uint64_t *__restrict__ uoff, int want_windows,
						   nxz_checkpoint_stream_t *__restrict__ streams)
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
	uint64_t *const cb = cbit + (size_t)jid * ((size_t)cp_cap + 1), *const uo = uoff + (size_t)jid * ((size_t)cp_cap + 1);
	nxz_cp_acc_t acc = nxz_cp_begin();
	nxz_size_stop_t stop = {};
	uint64_t end_bit = 0;
	if (st == NXZ_FRAME_OK)
		nxzs::walk(sm, (const NXZ_GLOBAL_AS uint8_t *)job.src + hdr_len, src_len - hdr_len, 0xffffffffu, 0, lane, stop, end_bit,
			   Hook{&acc, cb, uo, span, cp_cap, hdr_len, lane});
	const uint32_t produced = uni(stop.produced);
	const nxz_checkpoint_stream_t s = nxz_cp_summary(&acc, cp_cap, format, hdr_len, st, uni(stop.cc), uni(stop.final_eob), produced,
							 want_windows != 0, nxz_cp_have_output(job.dst, job.dst_cap, produced));
	if (lane == 0) {
		streams[jid] = s;
		if (nxz_cp_has_sentinel(s.status)) { cb[s.count] = nxz_cp_bit(hdr_len, end_bit); uo[s.count] = produced; }
	}
}

// d[0, len) <- s[0, len) by the threads t, t + nt, ...: the 16-byte granules that lie whole inside d by 16-byte stores (the loads
// at whatever alignment s has: device memory takes them), the bytes in front and behind one by one
typedef uint32_t v4u_any __attribute__((ext_vector_type(4), aligned(1)));
__device__ inline void copy_any(uint8_t *d, const uint8_t *s, uint64_t len, uint32_t t, uint32_t nt)
{
	uint64_t head = (16 - ((uintptr_t)d & 15)) & 15;
	if (head > len) head = len;
	const uint64_t body = (len - head) >> 4;
	for (uint64_t i = t; i < head; i += nt) d[i] = s[i];
	for (uint64_t g = t; g < body; g += nt) {
		const v4u_any v = *(const v4u_any *)(s + head + 16 * g);
		*(uint4 *)(d + head + 16 * g) = make_uint4(v.x, v.y, v.z, v.w);
	}
	for (uint64_t i = head + 16 * body + t; i < len; i += nt) d[i] = s[i];
}

__global__ __launch_bounds__(256) void window_kernel(const nxz_batch_job_t *__restrict__ jobs, uint64_t slots, uint32_t cp_cap,
						     const uint64_t *__restrict__ uoff, const nxz_checkpoint_stream_t *__restrict__ streams,
						     uint8_t *__restrict__ windows)
{
	for (uint64_t t = blockIdx.x; t < slots; t += gridDim.x) {
		const uint32_t i = (uint32_t)(t / cp_cap), k = (uint32_t)(t % cp_cap);
		const nxz_checkpoint_stream_t s = streams[i];
		const uint8_t *const out = jobs[i].dst;
		if (!nxz_cp_has_windows(s.status, nxz_cp_have_output(out, jobs[i].dst_cap, s.out_len)) || k >= nxz_cp_stored(s.count, cp_cap)) continue;
		const uint64_t u = uoff[(size_t)i * ((size_t)cp_cap + 1) + k];
		if (u > s.out_len) continue;                                       // (never: the index kernel wrote both)
		const uint32_t w = nxz_cp_window_len(u);
		copy_any(windows + t * NXZ_CP_WINDOW, out + (u - w), w, threadIdx.x, 256);
	}
}

// ---- the range read's plumbing ------------------------------------------------------------------------------------------------
constexpr uint32_t PART = 65536;         // bytes of a segment's input a stage workgroup copies

// ctl[0] index faulty (ctl[1..4]: the map's, nxz_bgzf.hip), ctl[5] the largest input of a needed segment, 16 for the alignment on top
__global__ __launch_bounds__(256) void check_kernel(uint64_t src_len, const uint64_t *__restrict__ cbit, const uint64_t *__restrict__ uoff, uint64_t L,
						    uint64_t *__restrict__ ctl)
{
	const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (j >= L) return;
	if (!nxz_cp_entry_ok(cbit, uoff, L, j, src_len)) atomicOr((unsigned long long *)&ctl[0], 1ull);
}

__global__ __launch_bounds__(256) void inmax_kernel(const uint64_t *__restrict__ cbit, const uint64_t *__restrict__ uoff, uint64_t L,
						    const uint32_t *__restrict__ midx, uint64_t *__restrict__ ctl)
{
	const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (j >= L || ctl[0] || midx[j] == ~0u) return;
	atomicMax((unsigned long long *)&ctl[5], (unsigned long long)(nxz_cp_job_len(cbit[j], cbit[j + 1], uoff[j]) + 16));
}

// grid (cnt, parts of PART bytes): needed segment k0 + blockIdx.x
__global__ __launch_bounds__(256) void stage_kernel(const uint8_t *__restrict__ src, const uint64_t *__restrict__ cbit, const uint64_t *__restrict__ uoff,
						    const uint8_t *__restrict__ windows, const uint32_t *__restrict__ list, uint64_t k0, uint8_t *islots,
						    uint64_t istride, uint8_t *oslots, uint64_t ostride, nxz_batch_job_t *__restrict__ jobs)
{
	const uint64_t kk = blockIdx.x;
	const uint64_t j = list[k0 + kk];
	const uint64_t c0 = cbit[j], c1 = cbit[j + 1], u0 = uoff[j];
	const uint64_t wlen = nxz_cp_window_len(u0), sb = nxz_cp_src_begin(c0), total = nxz_cp_job_len(c0, c1, u0);
	const uint64_t pad = (16 - (wlen & 15)) & 15;                         // the source bytes start at a 16-byte boundary of the slot
	if (pad + total > istride) return;                                    // (never: ctl[5] covers every needed segment)
	uint8_t *const base = islots + kk * istride + pad;
	if (blockIdx.y == 0 && threadIdx.x == 0) {
		nxz_batch_job_t jb = {};
		jb.src = base; jb.src_len = (uint32_t)total; jb.hist_len = (uint32_t)wlen;
		jb.dst = oslots + kk * ostride; jb.dst_cap = (uint32_t)nxz_cp_out_len(u0, uoff[j + 1]);
		jb.in_adler = 1;
		jb.resume = nxz_cp_resume(c0);
		jobs[kk] = jb;
	}
	const uint64_t lo = (uint64_t)blockIdx.y * PART, hi = lo + PART < total ? lo + PART : total;
	if (lo >= hi) return;
	if (lo < wlen) {
		const uint64_t e = hi < wlen ? hi : wlen;
		copy_any(base + lo, windows + j * NXZ_CP_WINDOW + lo, e - lo, threadIdx.x, 256);
	}
	if (hi > wlen) {
		const uint64_t b = lo > wlen ? lo : wlen;
		copy_any(base + b, src + sb + (b - wlen), hi - b, threadIdx.x, 256);
	}
}

__global__ __launch_bounds__(256) void verdict_kernel(const uint64_t *__restrict__ uoff, const uint32_t *__restrict__ list, uint64_t k0, uint64_t cnt,
						      const nxz_batch_result_t *__restrict__ results, nxz_batch_frame_t *__restrict__ frames)
{
	const uint64_t kk = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (kk >= cnt) return;
	const uint64_t j = list[k0 + kk];
	nxz_batch_frame_t f = {};
	f.status = nxz_cp_segment_good(results[kk].cc, results[kk].tpbc, nxz_cp_out_len(uoff[j], uoff[j + 1])) ? NXZ_FRAME_OK : NXZ_FRAME_DEFLATE;
	frames[kk] = f;
}

} // namespace nxzcp

// n jobs, a wavefront each (order: NULL, or nxz_launch_order_by_length's); then, with windows, the copies of the stored checkpoints' windows
extern "C" int nxz_launch_checkpoint_index(int fmt, const nxz_batch_job_t *jobs, size_t n, uint64_t span, uint32_t cp_cap, uint64_t *cbit, uint64_t *uoff,
					   uint8_t *windows, nxz_checkpoint_stream_t *streams, const uint32_t *order, hipStream_t stream)
{
	if (!n) return 0;
	hipLaunchKernelGGL(nxzcp::index_kernel, dim3((unsigned)n), dim3(64), 0, stream, fmt, jobs, order, span, cp_cap, cbit, uoff, windows ? 1 : 0, streams);
	const int rc = (int)hipGetLastError();
	return rc || !windows ? rc : nxz_launch_checkpoint_windows(jobs, n, cp_cap, uoff, streams, windows, stream);
}

// the windows of the stored checkpoints of n indexed jobs (behind an index kernel on the same stream: this file's, or nxz_checkpoint_fine.hip's)
extern "C" int nxz_launch_checkpoint_windows(const nxz_batch_job_t *jobs, size_t n, uint32_t cp_cap, const uint64_t *uoff, const nxz_checkpoint_stream_t *streams,
					     uint8_t *windows, hipStream_t stream)
{
	if (!n) return 0;
	const uint64_t slots = (uint64_t)n * cp_cap;
	hipLaunchKernelGGL(nxzcp::window_kernel, dim3((unsigned)(slots < (1u << 20) ? slots : (1u << 20))), dim3(256), 0, stream, jobs, slots, cp_cap, uoff,
			   streams, windows);
	return (int)hipGetLastError();
}

// between nxz_launch_range_map_clear and nxz_launch_range_map_ranges: ws[0] != 0 when the index is not valid
extern "C" int nxz_launch_checkpoint_check(uint64_t src_len, const uint64_t *cbit, const uint64_t *uoff, uint64_t L, uint8_t *ws, hipStream_t stream)
{
	if (!L) return 0;
	hipLaunchKernelGGL(nxzcp::check_kernel, dim3((unsigned)((L + 255) / 256)), dim3(256), 0, stream, src_len, cbit, uoff, L, (uint64_t *)ws);
	return (int)hipGetLastError();
}

// behind nxz_launch_range_map_ranges: ws[5] = the stride the input slots of the needed segments need
extern "C" int nxz_launch_checkpoint_inmax(const uint64_t *cbit, const uint64_t *uoff, uint64_t n, uint64_t L, uint8_t *ws, hipStream_t stream)
{
	if (!L) return 0;
	const uint32_t *midx, *list;
	nxz_range_map_lists(ws, n, L, &midx, &list);
	hipLaunchKernelGGL(nxzcp::inmax_kernel, dim3((unsigned)((L + 255) / 256)), dim3(256), 0, stream, cbit, uoff, L, midx, (uint64_t *)ws);
	return (int)hipGetLastError();
}

// The jobs of needed segments k0 .. k0 + cnt - 1: segment k's input at islots + (k - k0) * istride, its output at oslots + (k - k0) * ostride
extern "C" int nxz_launch_checkpoint_stage(const uint8_t *src, const uint64_t *cbit, const uint64_t *uoff, const uint8_t *windows, uint64_t n, uint64_t L,
					   uint8_t *ws, uint64_t k0, uint64_t cnt, uint8_t *islots, uint64_t istride, uint8_t *oslots, uint64_t ostride,
					   nxz_batch_job_t *jobs, hipStream_t stream)
{
	if (!cnt) return 0;
	const uint32_t *midx, *list;
	nxz_range_map_lists(ws, n, L, &midx, &list);
	const uint64_t parts = (istride + nxzcp::PART - 1) / nxzcp::PART;
	if (cnt >= (1ull << 31) || parts > 65535) return (int)hipErrorInvalidValue;
	hipLaunchKernelGGL(nxzcp::stage_kernel, dim3((unsigned)cnt, (unsigned)parts), dim3(256), 0, stream, src, cbit, uoff, windows, list, k0, islots, istride,
			   oslots, ostride, jobs);
	return (int)hipGetLastError();
}

// behind the decode of the chunk: frames[k].status for nxz_launch_bgzf_gather
extern "C" int nxz_launch_checkpoint_verdict(const uint64_t *uoff, uint64_t n, uint64_t L, uint8_t *ws, uint64_t k0, uint64_t cnt,
					     const nxz_batch_result_t *results, nxz_batch_frame_t *frames, hipStream_t stream)
{
	if (!cnt) return 0;
	const uint32_t *midx, *list;
	nxz_range_map_lists(ws, n, L, &midx, &list);
	hipLaunchKernelGGL(nxzcp::verdict_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, stream, uoff, list, k0, cnt, results, frames);
	return (int)hipGetLastError();
}
