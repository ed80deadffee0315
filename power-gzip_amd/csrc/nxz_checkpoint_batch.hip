// nxz_checkpoint_batch.hip -- ranges over ALL the streams of an indexed batch in one call (nxz_batch_checkpoint_read_ranges; gfx950,
// wave64).  The rules are nxz_checkpoint_batch.h's.  The batch's index is read as ONE index of n_jobs * (cp_cap + 1) entries in the
// order the index calls wrote it, with a uoff of its own that never decreases (the rows' uoff on top of the bytes of the rows in
// front); then the map, gather and zero kernels of nxz_bgzf.hip and the inmax and verdict kernels of nxz_checkpoint.hip work as they
// stand, and nxz_batch_ranges.cpp's driver waits once for the whole batch.  What is new here, in launch order:
//   rows_kernel      a thread an entry: the stream's record (at entry 0) and nxz_cpb_entry_ok against jobs[row].src_len; any fault
//                    sets bad[row] -- the verdict is the row's, not the call's
//   base_kernel      one workgroup: base[] = exclusive prefix sum of the good rows' extents (shuffles inside a wavefront, the
//                    sixteen wavefronts' sums through 128 bytes of LDS)
//   flat_kernel      a thread an entry: the flat uoff; a thread a range: (job, begin, end) onto the flat index, [0, 0) where the
//                    range gets no bytes
//   status_kernel    behind the map, a thread a range: NXZ_RANGE_BAD_STREAM / _OUT_OF_BOUNDS where the map saw [0, 0)
//   stage_kernel     nxzcp::stage_kernel with the segment's row: source bytes from jobs[row].src, the window from slot
//                    row * cp_cap + k; the first workgroup writes the job record and, with state, what nxzcf::jobs_kernel adds:
//                    the table slot, resume and NXZ_JOB_SUSPEND_WHEN_FULL
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "nxz_device.h"
#include "nxz_checkpoint_batch.h"

namespace nxzcr {

constexpr uint32_t PART = 65536;         // bytes of a segment's input a stage workgroup copies

__global__ __launch_bounds__(256) void rows_kernel(const nxz_batch_job_t *__restrict__ jobs, uint64_t entries, uint32_t cp_cap,
						   const uint64_t *__restrict__ cbit, const uint64_t *__restrict__ uoff,
						   const nxz_checkpoint_state_t *__restrict__ state, const nxz_checkpoint_stream_t *__restrict__ streams,
						   uint32_t *__restrict__ bad)
{
	const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (e >= entries) return;
	const uint64_t row = nxz_cpb_row_of(e, cp_cap), e0 = nxz_cpb_entry(row, 0, cp_cap);
	const uint32_t k = nxz_cpb_k_of(e, cp_cap);
	const uint32_t status = streams[row].status, count = streams[row].count;
	if (!nxz_cpb_head_ok(status, count, cp_cap, jobs[row].src != nullptr)) {
		if (k == 0) bad[row] = 1;
		return;
	}
	if (k < count && !nxz_cpb_entry_ok(cbit + e0, uoff + e0, state ? state + e0 : nullptr, count, k, jobs[row].src_len)) atomicOr(&bad[row], 1u);
}

// exclusive prefix sum across one workgroup of 1024 threads: returns the thread's start, *total; wsum: 16 entries of LDS
__device__ inline uint64_t block_excl(uint64_t v, uint64_t *wsum, uint64_t *total)
{
	const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	uint64_t inc = v;
	for (uint32_t d = 1; d < 64; d <<= 1) {
		const uint64_t u = __shfl_up((unsigned long long)inc, d, 64);
		if (lane >= d) inc += u;
	}
	if (lane == 63) wsum[w] = inc;
	__syncthreads();
	uint64_t off = 0, tot = 0;
	for (uint32_t i = 0; i < 16; i++) {
		const uint64_t s = wsum[i];
		off += i < w ? s : 0;
		tot += s;
	}
	*total = tot;
	return off + inc - v;
}

__global__ __launch_bounds__(1024) void base_kernel(uint64_t n_jobs, uint32_t cp_cap, const uint64_t *__restrict__ uoff,
						    const nxz_checkpoint_stream_t *__restrict__ streams, const uint32_t *__restrict__ bad,
						    uint64_t *__restrict__ base)
{
	__shared__ uint64_t wsum[16];
	const uint32_t t = threadIdx.x;
	const uint64_t per = (n_jobs + 1023) / 1024, lo = t * per < n_jobs ? t * per : n_jobs, hi = lo + per < n_jobs ? lo + per : n_jobs;
	auto extent = [&](uint64_t row) { return nxz_cpb_extent(!bad[row], uoff + nxz_cpb_entry(row, 0, cp_cap), bad[row] ? 0 : streams[row].count); };
	uint64_t sum = 0, tot;
	for (uint64_t row = lo; row < hi; row++) sum += extent(row);
	uint64_t b = block_excl(sum, wsum, &tot);
	for (uint64_t row = lo; row < hi; row++) { base[row] = b; b += extent(row); }
	if (t == 0) base[n_jobs] = tot;
}

__global__ __launch_bounds__(256) void flat_kernel(uint64_t n_jobs, uint64_t entries, uint32_t cp_cap, const uint64_t *__restrict__ uoff,
						   const nxz_checkpoint_stream_t *__restrict__ streams, const uint32_t *__restrict__ bad,
						   const uint64_t *__restrict__ base, uint64_t *__restrict__ fuoff, const nxz_batch_range_t *__restrict__ ranges,
						   uint64_t n, nxz_bgzf_range_t *__restrict__ mapped)
{
	const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (t < entries) {
		const uint64_t row = nxz_cpb_row_of(t, cp_cap);
		const bool good = !bad[row];
		fuoff[t] = nxz_cpb_flat_uoff(good, base[row], base[row + 1], uoff + nxz_cpb_entry(row, 0, cp_cap), good ? streams[row].count : 0, nxz_cpb_k_of(t, cp_cap));
	}
	if (t < n) {
		const nxz_batch_range_t q = ranges[t];
		nxz_bgzf_range_t m;
		(void)nxz_cpb_map_range(q.job, q.begin, q.end, n_jobs, bad, base, &m.begin, &m.end);
		mapped[t] = m;
	}
}

__global__ __launch_bounds__(256) void status_kernel(uint64_t n_jobs, const uint32_t *__restrict__ bad, const uint64_t *__restrict__ base,
						     const nxz_batch_range_t *__restrict__ ranges, uint64_t n, uint32_t *__restrict__ status)
{
	const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (r >= n) return;
	const nxz_batch_range_t q = ranges[r];
	uint64_t fb, fe;
	const uint32_t st = nxz_cpb_map_range(q.job, q.begin, q.end, n_jobs, bad, base, &fb, &fe);
	if (st != NXZ_RANGE_OK) status[r] = st;
}

// d[0, len) <- s[0, len) by the threads t, t + nt, ...: nxzcp::copy_any -- the 16-byte granules that lie whole inside d by 16-byte
// stores (the loads at whatever alignment s has), the bytes in front and behind one by one
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

// grid (cnt, parts of PART bytes): needed segment k0 + blockIdx.x of the flat index.  dht: NULL without state
__global__ __launch_bounds__(256) void stage_kernel(const nxz_batch_job_t *__restrict__ in, uint64_t n_jobs, uint32_t cp_cap,
						    const uint64_t *__restrict__ cbit, const uint64_t *__restrict__ uoff,
						    const nxz_checkpoint_state_t *__restrict__ state, const uint8_t *__restrict__ windows,
						    const nxz_checkpoint_stream_t *__restrict__ streams, const uint32_t *__restrict__ bad,
						    const uint32_t *__restrict__ list, uint64_t k0, uint8_t *islots, uint64_t istride, uint8_t *oslots,
						    uint64_t ostride, nxz_batch_job_t *__restrict__ jobs, nxz_batch_dht_t *__restrict__ dht)
{
	const uint64_t kk = blockIdx.x;
	const uint64_t j = list[k0 + kk];
	const bool first = blockIdx.y == 0;
	bool ok = nxz_cpb_segment_ok(j, n_jobs, cp_cap, bad, streams);          // (always: the map needs segments of good rows only)
	uint64_t c0 = 0, c1 = 0, u0 = 0, wlen = 0, total = 0, pad = 0;
	if (ok) {
		c0 = cbit[j]; c1 = cbit[j + 1]; u0 = uoff[j];
		wlen = nxz_cp_window_len(u0); total = nxz_cp_job_len(c0, c1, u0);
		pad = (16 - (wlen & 15)) & 15;                                     // the source bytes start at a 16-byte boundary of the slot
		ok = pad + total <= istride;                                      // (always: ctl[5] covers every needed segment)
	}
	if (!ok) {                                                            // a job of nothing: the segment is not good, its ranges read zeros
		if (first && threadIdx.x == 0) { const nxz_batch_job_t none = {}; jobs[kk] = none; if (dht) dht[kk].dhtlen = 0; }
		return;
	}
	const uint64_t row = nxz_cpb_row_of(j, cp_cap);
	const uint8_t *const src = in[row].src;
	uint8_t *const base = islots + kk * istride + pad;
	if (first) {
		nxz_checkpoint_state_t s = {};
		if (state) s = state[j];
		if (dht) {
			const bool dyn = nxz_cpf_is_dynamic(nxz_cpf_sfbt(s.resume));
			nxz_batch_dht_t *const t = &dht[kk];
			for (uint32_t i = threadIdx.x; i < sizeof(t->dht); i += 256) t->dht[i] = dyn ? nxz_cpf_dht_byte(src, s.tbit, s.dhtlen, i) : 0;
			if (threadIdx.x == 0) t->dhtlen = dyn ? s.dhtlen : 0;
		}
		if (threadIdx.x == 0) {
			nxz_batch_job_t jb = {};
			jb.src = base; jb.src_len = (uint32_t)total; jb.hist_len = (uint32_t)wlen;
			jb.dst = oslots + kk * ostride; jb.dst_cap = (uint32_t)nxz_cp_out_len(u0, uoff[j + 1]);
			jb.in_adler = 1;
			jb.resume = nxz_cpf_resume(&s, c0);
			jb.reserved = state ? nxz_cpf_job_flags() : 0;
			jobs[kk] = jb;
		}
	}
	const uint64_t lo = (uint64_t)blockIdx.y * PART, hi = lo + PART < total ? lo + PART : total;
	if (lo >= hi) return;
	if (lo < wlen) {
		const uint64_t e = hi < wlen ? hi : wlen;
		copy_any(base + lo, windows + nxz_cpb_window_at(row, nxz_cpb_k_of(j, cp_cap), cp_cap) + lo, e - lo, threadIdx.x, 256);
	}
	if (hi > wlen) {
		const uint64_t b = lo > wlen ? lo : wlen;
		copy_any(base + b, src + nxz_cp_src_begin(c0) + (b - wlen), hi - b, threadIdx.x, 256);
	}
}

} // namespace nxzcr

static size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

// The call's own arrays inside bws: a word a row (bad), base (n_jobs + 1), the flat uoff (an entry each), the mapped ranges (n)
struct BatchWs {
	uint32_t *bad;
	uint64_t *base, *fuoff;
	nxz_bgzf_range_t *mapped;
};
static BatchWs batch_ws(uint8_t *bws, uint64_t n_jobs, uint32_t cp_cap, uint64_t n)
{
	BatchWs w;
	uint8_t *p = bws;
	auto take = [&](size_t b) { uint8_t *q = p; p += up256(b); return q; };
	w.bad = (uint32_t *)take(n_jobs * 4);
	w.base = (uint64_t *)take((n_jobs + 1) * 8);
	w.fuoff = (uint64_t *)take(nxz_cpb_entries(n_jobs, cp_cap) * 8);
	w.mapped = (nxz_bgzf_range_t *)take(n * sizeof(nxz_bgzf_range_t));
	return w;
}

extern "C" size_t nxz_checkpoint_batch_workspace(uint64_t n_jobs, uint32_t cp_cap, uint64_t n)
{
	return up256(n_jobs * 4) + up256((n_jobs + 1) * 8) + up256(nxz_cpb_entries(n_jobs, cp_cap) * 8) + up256(n * sizeof(nxz_bgzf_range_t));
}

// the flat uoff: what the map, gather, inmax and verdict launches take for uoff (L = entries - 1)
extern "C" const uint64_t *nxz_checkpoint_batch_uoff(uint8_t *bws, uint64_t n_jobs, uint32_t cp_cap, uint64_t n)
{
	return batch_ws(bws, n_jobs, cp_cap, n).fuoff;
}

// The map of the batch into ws (nxz_bgzf_ranges_workspace(n, entries - 1) bytes): the rows' verdicts, the bases, the flat uoff and
// the mapped ranges into bws, then nxz_bgzf.hip's map over them, the statuses it cannot know and the largest input (ws[5]).
// n_jobs >= 1 and nxz_cpb_shape_ok; ws[0] stays 0: a row that is not good is its ranges' matter
extern "C" int nxz_launch_checkpoint_batch_map(const nxz_batch_job_t *jobs, uint64_t n_jobs, uint32_t cp_cap, const uint64_t *cbit, const uint64_t *uoff,
					       const nxz_checkpoint_state_t *state, const nxz_checkpoint_stream_t *streams, const nxz_batch_range_t *ranges,
					       uint64_t n, uint64_t *offsets, uint32_t *status, uint8_t *bws, uint8_t *ws, hipStream_t stream)
{
	const BatchWs w = batch_ws(bws, n_jobs, cp_cap, n);
	const uint64_t entries = nxz_cpb_entries(n_jobs, cp_cap), L = entries - 1, most = entries > n ? entries : n;
	int rc = nxz_launch_range_map_clear(ws, n, L, stream);
	if (rc) return rc;
	(void)hipMemsetAsync(w.bad, 0, n_jobs * 4, stream);
	hipLaunchKernelGGL(nxzcr::rows_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, stream, jobs, entries, cp_cap, cbit, uoff, state, streams, w.bad);
	hipLaunchKernelGGL(nxzcr::base_kernel, dim3(1), dim3(1024), 0, stream, n_jobs, cp_cap, uoff, streams, w.bad, w.base);
	hipLaunchKernelGGL(nxzcr::flat_kernel, dim3((unsigned)((most + 255) / 256)), dim3(256), 0, stream, n_jobs, entries, cp_cap, uoff, streams, w.bad, w.base,
			   w.fuoff, ranges, n, w.mapped);
	if ((rc = (int)hipGetLastError()) != 0) return rc;
	if ((rc = nxz_launch_range_map_ranges(w.fuoff, L, w.mapped, n, offsets, status, ws, stream)) != 0) return rc;
	if (n) hipLaunchKernelGGL(nxzcr::status_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n_jobs, w.bad, w.base, ranges, n, status);
	if ((rc = (int)hipGetLastError()) != 0) return rc;
	return nxz_launch_checkpoint_inmax(cbit, uoff, n, L, ws, stream);
}

// The jobs of needed segments k0 .. k0 + cnt - 1 of the flat index (nxz_launch_checkpoint_stage's slots); dht: NULL without state,
// else the segments' table slots
extern "C" int nxz_launch_checkpoint_batch_stage(const nxz_batch_job_t *in, uint64_t n_jobs, uint32_t cp_cap, const uint64_t *cbit, const uint64_t *uoff,
						 const nxz_checkpoint_state_t *state, const uint8_t *windows, const nxz_checkpoint_stream_t *streams,
						 uint64_t n, uint8_t *bws, uint8_t *ws, uint64_t k0, uint64_t cnt, uint8_t *islots, uint64_t istride,
						 uint8_t *oslots, uint64_t ostride, nxz_batch_job_t *jobs, nxz_batch_dht_t *dht, hipStream_t stream)
{
	if (!cnt) return 0;
	const BatchWs w = batch_ws(bws, n_jobs, cp_cap, n);
	const uint32_t *midx, *list;
	nxz_range_map_lists(ws, n, nxz_cpb_entries(n_jobs, cp_cap) - 1, &midx, &list);
	const uint64_t parts = (istride + nxzcr::PART - 1) / nxzcr::PART;
	if (cnt >= (1ull << 31) || parts > 65535) return (int)hipErrorInvalidValue;
	hipLaunchKernelGGL(nxzcr::stage_kernel, dim3((unsigned)cnt, (unsigned)parts), dim3(256), 0, stream, in, n_jobs, cp_cap, cbit, uoff, state, windows, streams,
			   w.bad, list, k0, islots, istride, oslots, ostride, jobs, state ? dht : nullptr);
	return (int)hipGetLastError();
}
