// nxz_inflate_part.hip -- the kernels around the raw decode of nxz_batch_inflate_streams_part (include/nxz_engine.h): a batch of raw /
// zlib / gzip streams READ in parts, a device buffer a part, the stream's running state in a carry record on the device.  The rules
// are nxz_inflate_part.h (the header's byte-wise state machine, the trailer, the tail, the refusals, the slot), the field rules of
// the framing nxz_frame.h's.  A chunk of the batch (streams whose staging slots fit the scratch bound) goes through
//
//   open     a thread per stream: the refusals; with NXZ_PART_FIRST the carry afresh; in phase header the state machine over the
//            part's bytes; in phase trailer the trailer's bytes, and its check when the last is there; in phase body, with bytes to
//            decode, the raw job ([window][tail][part from the deflate data's first byte] in the stream's slot, resume state and
//            checksums from the carry, NXZ_JOB_SUSPEND_WHEN_FULL) and its table slot.  Every other stream gets an empty job and its
//            result here
//   stage    ONE grid over the 16-byte pieces of all the chunk's slots: a piece's stream by binary search in the slots' offsets, its
//            bytes from the window, the carry's tail or the part -- a piece that lies whole inside the window or the part through
//            aligned 16-byte loads joined by a byte shift (nxz_shift_load.h), the few that straddle a seam or the end byte by byte
//   -- nxz_batch_decompress on those jobs with the table slots as dht_io, kept off the stream-per-lane kernel --
//   close    a thread per stream that was decoded: result and table slot into the carry and the part's result
#include <hip/hip_runtime.h>
#include "nxz_device.h"
#include "nxz_inflate_part.h"
#include "nxz_shift_load.h"

namespace nxzip {

// desc, carry, results: the chunk's; off[m + 1]: where each stream's slot begins in `stage` (multiples of 16)
__global__ __launch_bounds__(256) void open_kernel(const nxz_inflate_part_job_t *__restrict__ desc, uint32_t m, int fmt,
						     nxz_inflate_carry_t *__restrict__ carry, const uint64_t *__restrict__ off, uint8_t *__restrict__ stage,
						     nxz_batch_job_t *__restrict__ jobs, nxz_batch_dht_t *__restrict__ dht,
						     nxz_inflate_part_work_t *__restrict__ work, nxz_inflate_part_result_t *__restrict__ results)
{
	const uint32_t t = blockIdx.x * 256 + threadIdx.x;
	if (t >= m) return;
	const nxz_inflate_part_job_t *const j = &desc[t];
	nxz_inflate_carry_t *const c = &carry[t];
	uint8_t *const slot = stage + off[t];
	nxz_inflate_part_work_t wk;
	wk.body = 0; wk.live = 0; wk.staged = 0; wk.reserved = 0;
	const uint32_t cc = nxz_inflate_part_refusal(j, c->phase, c->tail_len);
	if (cc) nxz_inflate_part_refuse(cc, &results[t]);
	else if (nxz_inflate_part_open(c, j, fmt, &wk.body, &results[t])) {
		wk.live = 1;
		wk.staged = nxz_inflate_part_staged(c, j);
		jobs[t] = nxz_inflate_part_decode_job(c, j, wk.body, slot, &dht[t]);
	}
	if (!wk.live) jobs[t] = nxz_inflate_part_idle_job(slot);
	work[t] = wk;
}

__global__ __launch_bounds__(256) void stage_kernel(const nxz_inflate_part_job_t *__restrict__ desc, const nxz_inflate_carry_t *__restrict__ carry,
						      const uint64_t *__restrict__ off, uint32_t m, const nxz_inflate_part_work_t *__restrict__ work,
						      const nxz_batch_job_t *__restrict__ jobs)
{
	const uint64_t at = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 16;
	if (at >= off[m]) return;
	uint32_t lo = 0, hi = m;                                             // off[lo] <= at < off[hi]
	while (hi - lo > 1) {
		const uint32_t mid = lo + (hi - lo) / 2;
		if (off[mid] <= at) lo = mid; else hi = mid;
	}
	const uint32_t i = lo;
	if (!work[i].staged) return;
	const uint64_t o64 = at - off[i];
	const uint32_t total = jobs[i].src_len, w = jobs[i].hist_len;
	if (o64 >= total) return;
	const uint32_t o = (uint32_t)o64, t = carry[i].tail_len;
	const uint8_t *const win = desc[i].prev + desc[i].prev_len - w, *const src = desc[i].src + work[i].body;
	uint4 v;
	if (o + 16 <= w) v = nxz::load16_any(win + o);
	else if (o >= w + t && total - o >= 16) v = nxz::load16_any(src + (o - w - t));
	else {
		const uint8_t *const tail = carry[i].tail;
		uint32_t x0 = 0, x1 = 0, x2 = 0, x3 = 0;
#pragma unroll
		for (uint32_t k = 0; k < 16; k++) {
			const uint32_t q = o + k;
			uint32_t b = 0;
			if (q < total) b = q < w ? win[q] : q < w + t ? tail[q - w] : src[q - w - t];
			b <<= 8 * (k & 3);
			if (k < 4) x0 |= b; else if (k < 8) x1 |= b; else if (k < 12) x2 |= b; else x3 |= b;
		}
		v = make_uint4(x0, x1, x2, x3);
	}
	*(uint4 *)(const_cast<uint8_t *>(jobs[i].src) + o) = v;
}

__global__ __launch_bounds__(256) void close_kernel(const nxz_inflate_part_job_t *__restrict__ desc, uint32_t m, nxz_inflate_carry_t *__restrict__ carry,
						      const nxz_batch_job_t *__restrict__ jobs, const nxz_batch_result_t *__restrict__ dres,
						      const nxz_batch_dht_t *__restrict__ dht, const nxz_inflate_part_work_t *__restrict__ work,
						      nxz_inflate_part_result_t *__restrict__ results)
{
	const uint32_t t = blockIdx.x * 256 + threadIdx.x;
	if (t >= m || !work[t].live) return;
	nxz_inflate_part_close(&carry[t], &desc[t], work[t].body, &jobs[t], &dres[t], &dht[t], &results[t]);
}

} // namespace nxzip

extern "C" int nxz_launch_inflate_part_open(const nxz_inflate_part_job_t *desc, uint32_t m, int fmt, nxz_inflate_carry_t *carry, const uint64_t *off,
					    uint8_t *stage, nxz_batch_job_t *jobs, nxz_batch_dht_t *dht, nxz_inflate_part_work_t *work,
					    nxz_inflate_part_result_t *results, hipStream_t stream)
{
	hipLaunchKernelGGL(nxzip::open_kernel, dim3((m + 255) / 256), dim3(256), 0, stream, desc, m, fmt, carry, off, stage, jobs, dht, work, results);
	return (int)hipGetLastError();
}

// bytes: the chunk's staging bytes (off[m] on the host)
extern "C" int nxz_launch_inflate_part_stage(const nxz_inflate_part_job_t *desc, const nxz_inflate_carry_t *carry, const uint64_t *off, uint32_t m,
					     uint64_t bytes, const nxz_inflate_part_work_t *work, const nxz_batch_job_t *jobs, hipStream_t stream)
{
	const uint64_t blocks = (bytes / 16 + 255) / 256;
	if (!blocks) return 0;
	hipLaunchKernelGGL(nxzip::stage_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream, desc, carry, off, m, work, jobs);
	return (int)hipGetLastError();
}

extern "C" int nxz_launch_inflate_part_close(const nxz_inflate_part_job_t *desc, uint32_t m, nxz_inflate_carry_t *carry, const nxz_batch_job_t *jobs,
					     const nxz_batch_result_t *dres, const nxz_batch_dht_t *dht, const nxz_inflate_part_work_t *work,
					     nxz_inflate_part_result_t *results, hipStream_t stream)
{
	hipLaunchKernelGGL(nxzip::close_kernel, dim3((m + 255) / 256), dim3(256), 0, stream, desc, m, carry, jobs, dres, dht, work, results);
	return (int)hipGetLastError();
}
