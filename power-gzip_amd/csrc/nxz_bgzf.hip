// nxz_bgzf.hip -- BGZF random access on the device: a batch of byte ranges of a BGZF image, read through its member index
// (nxz_bgzf_read_ranges; nxz_batch_ranges.cpp runs the steps on the caller's stream and waits once, after the map).
//
// Map (nothing is decoded before the index has been checked):
//   index_check_kernel   a thread a member: nxz_bgzf_member_size at coff[j] - coff[0] == coff[j+1] - coff[j], uoff
//                        not decreasing; any fault sets ctl[0] and every later kernel writes nothing
//   range_map_kernel     a thread a range: nxz_bgzf_range.h's resolve, the first and last member by binary search,
//                        and +1 / -1 at first / last + 1 of a difference array over the members (atomics)
//   member_scan_kernel   one workgroup: prefix sum of the difference array = how many ranges cover member j; the covered
//                        ones compacted by a second prefix sum (midx[j] = its place, list[k] = the member), and the largest
//                        of their sizes (the slot stride)
//   range_scan_kernel    one workgroup: offsets[] = exclusive prefix sum of the ranges' lengths, poff[] = the same of their
//                        pieces (a piece = a (range, member) pair)
// Decode, a chunk of needed members at a time:
//   job_kernel           a framed gzip job per needed member, its output in a 16-byte aligned slot of `stride` bytes
//   (nxz_batch_decompress_framed on those jobs)
//   gather_kernel        a workgroup per piece (and per 64 KiB of it): its range by binary search over poff, its member,
//                        16-byte loads from the slot and 16-byte stores to dst (alignbyte for the shift between the two)
// Last, zero_kernel clears the ranges a failed member marked DAMAGED.
#include <hip/hip_runtime.h>
#include "nxz_device.h"
#include "nxz_frame.h"
#include "nxz_bgzf_range.h"

namespace nxzr {

constexpr uint32_t WIN = 65536;          // bytes of a piece a gather workgroup copies

// ctl[0] index faulty, [1] needed members, [2] bytes of all ranges, [3] pieces, [4] largest needed member (uncompressed)
__global__ __launch_bounds__(256) void index_check_kernel(const uint8_t *__restrict__ packed, uint64_t packed_len, const uint64_t *__restrict__ coff,
							  const uint64_t *__restrict__ uoff, uint64_t L, uint64_t *__restrict__ ctl)
{
	const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (j >= L) return;
	const uint64_t c0 = coff[0], cj = coff[j], cn = coff[j + 1];
	bool bad = cj < c0 || cn <= cj || cj - c0 >= packed_len || uoff[j + 1] < uoff[j] || uoff[j + 1] - uoff[j] > 0xffffffffull;
	if (!bad) bad = nxz_bgzf_member_size(packed + (cj - c0), packed_len - (cj - c0)) != cn - cj;
	if (bad) atomicOr((unsigned long long *)&ctl[0], 1ull);
}

__global__ __launch_bounds__(256) void range_map_kernel(const uint64_t *__restrict__ coff, const uint64_t *__restrict__ uoff, uint64_t L, int kind,
							const nxz_bgzf_range_t *__restrict__ ranges, uint64_t n, const uint64_t *__restrict__ ctl,
							uint32_t *__restrict__ status, uint64_t *__restrict__ rb, uint64_t *__restrict__ rfirst,
							uint64_t *__restrict__ rlen, uint64_t *__restrict__ rpieces, int32_t *__restrict__ diff)
{
	const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (r >= n || ctl[0]) return;
	const nxz_bgzf_range_t q = ranges[r];
	uint64_t ub, ue, first = 0, pieces = 0;
	const uint32_t st = nxz_bgzf_resolve(coff, uoff, L, kind, q.begin, q.end, &ub, &ue);
	if (ue > ub) {
		first = nxz_bgzf_member_of(uoff, L, ub);
		const uint64_t last = nxz_bgzf_member_of(uoff, L, ue - 1);
		pieces = last - first + 1;
		atomicAdd(&diff[first], 1);
		atomicAdd(&diff[last + 1], -1);
	}
	status[r] = st;
	rb[r] = ub; rfirst[r] = first; rlen[r] = ue - ub; rpieces[r] = pieces;
}

__global__ __launch_bounds__(1024) void member_scan_kernel(int32_t *__restrict__ diff, const uint64_t *__restrict__ uoff, uint64_t L,
							   uint64_t *__restrict__ ctl, uint32_t *__restrict__ midx, uint32_t *__restrict__ list)
{
	__shared__ uint64_t part[1024];
	if (ctl[0]) return;
	const uint32_t t = threadIdx.x;
	const uint64_t per = (L + 1023) / 1024, lo = t * per < L ? t * per : L, hi = lo + per < L ? lo + per : L;
	int64_t sum = 0;
	for (uint64_t j = lo; j < hi; j++) sum += diff[j];
	uint64_t tot;
	int64_t cover = (int64_t)nxz_block_excl((uint64_t)sum, part, &tot);    // (two's complement: the sums of a prefix are >= 0)
	uint64_t cnt = 0;
	for (uint64_t j = lo; j < hi; j++) {
		cover += diff[j];
		diff[j] = cover > 0;                                          // (the difference array becomes the needed flags)
		cnt += cover > 0;
	}
	uint64_t k = nxz_block_excl(cnt, part, &tot), big = 0;
	for (uint64_t j = lo; j < hi; j++) {
		if (diff[j]) {
			midx[j] = (uint32_t)k; list[k++] = (uint32_t)j;
			const uint64_t sz = uoff[j + 1] - uoff[j];
			big = sz > big ? sz : big;
		} else midx[j] = ~0u;
	}
	if (big) atomicMax((unsigned long long *)&ctl[4], (unsigned long long)big);
	if (t == 0) ctl[1] = tot;
}

__global__ __launch_bounds__(1024) void range_scan_kernel(const uint64_t *__restrict__ rlen, const uint64_t *__restrict__ rpieces, uint64_t n,
							  uint64_t *__restrict__ ctl, uint64_t *__restrict__ offsets, uint64_t *__restrict__ poff)
{
	__shared__ uint64_t part[1024];
	if (ctl[0]) return;
	const uint32_t t = threadIdx.x;
	const uint64_t per = (n + 1023) / 1024, lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
	uint64_t s = 0, p = 0;
	for (uint64_t r = lo; r < hi; r++) { s += rlen[r]; p += rpieces[r]; }
	uint64_t ts, tp;
	uint64_t o = nxz_block_excl(s, part, &ts), q = nxz_block_excl(p, part, &tp);
	for (uint64_t r = lo; r < hi; r++) { offsets[r] = o; poff[r] = q; o += rlen[r]; q += rpieces[r]; }
	if (t == 0) { offsets[n] = ts; poff[n] = tp; ctl[2] = ts; ctl[3] = tp; }
}

__global__ __launch_bounds__(256) void job_kernel(const uint8_t *__restrict__ packed, const uint64_t *__restrict__ coff, const uint64_t *__restrict__ uoff,
						  const uint32_t *__restrict__ list, uint64_t k0, uint64_t cnt, uint8_t *slots, uint64_t stride,
						  nxz_batch_job_t *__restrict__ jobs)
{
	const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (k >= cnt) return;
	const uint32_t j = list[k0 + k];
	nxz_batch_job_t jb = {};
	jb.src = packed + (coff[j] - coff[0]);
	jb.src_len = (uint32_t)(coff[j + 1] - coff[j]);
	jb.dst = slots + k * stride;
	jb.dst_cap = (uint32_t)(uoff[j + 1] - uoff[j]);
	jb.in_adler = 1;
	jobs[k] = jb;
}

// bytes [s, s + 16) of two aligned granules w[0..7] (s = 0..15 of the first): word i is alignbyte of words q + i + 1, q + i
template <int I>
__device__ inline uint32_t shifted_word(const uint32_t (&w)[8], uint32_t q, uint32_t b)
{
	const uint32_t lo0 = (q & 2) ? w[I + 2] : w[I], lo1 = (q & 2) ? w[I + 3] : w[I + 1];
	const uint32_t hi1 = (q & 2) ? w[(I + 4) & 7] : w[I + 2];
	const uint32_t lo = (q & 1) ? lo1 : lo0, hi = (q & 1) ? hi1 : lo1;
	return __builtin_amdgcn_alignbyte(hi, lo, b);
}

// d[0, len) <- s[0, len): whole 16-byte granules of d by 16-byte loads and stores, the partial ones at either end byte by byte
// (another piece may own their other bytes).  s reads whole aligned granules: the slot is 16-byte aligned and a multiple of 16.
__device__ inline void copy_bytes(uint8_t *d, const uint8_t *s, uint64_t len)
{
	const uint64_t da = (uintptr_t)d & 15;
	const uint8_t *g0 = d - da;                                         // the granule that holds d[0]
	const uint64_t ng = (da + len + 15) >> 4;
	const uint32_t sh = (uint32_t)(((uintptr_t)s - (uintptr_t)d) & 15);   // s[k] sits sh bytes further into its granule than d[k]
	const uint32_t q = sh >> 2, b = sh & 3;
	for (uint64_t g = threadIdx.x; g < ng; g += blockDim.x) {
		uint8_t *gp = (uint8_t *)g0 + g * 16;
		const int64_t k0 = (int64_t)(g * 16) - (int64_t)da;              // the piece byte at gp[0]
		if (k0 >= 0 && (uint64_t)k0 + 16 <= len) {
			const uint8_t *sp = s + k0, *sa = sp - sh;
			const uint4 a = *(const uint4 *)sa;
			const uint4 c = sh ? *(const uint4 *)(sa + 16) : make_uint4(0, 0, 0, 0);
			const uint32_t w[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
			*(uint4 *)gp = make_uint4(shifted_word<0>(w, q, b), shifted_word<1>(w, q, b), shifted_word<2>(w, q, b), shifted_word<3>(w, q, b));
		} else {
			for (int64_t k = k0 < 0 ? 0 : k0; k < k0 + 16 && (uint64_t)k < len; k++) d[k] = s[k];
		}
	}
}

// grid (pieces, parts of WIN bytes): the pieces whose member is needed member k0 .. k0 + cnt - 1
__global__ __launch_bounds__(256) void gather_kernel(const uint64_t *__restrict__ uoff, const uint32_t *__restrict__ midx, const uint64_t *__restrict__ poff,
						     uint64_t n, const uint64_t *__restrict__ rb, const uint64_t *__restrict__ rfirst,
						     const uint64_t *__restrict__ rlen, const uint64_t *__restrict__ offsets, const uint8_t *slots,
						     uint64_t stride, uint64_t k0, uint64_t cnt, const nxz_batch_frame_t *__restrict__ frames,
						     const nxz_batch_result_t *__restrict__ results, uint8_t *dst, uint32_t *__restrict__ status)
{
	const uint64_t p = blockIdx.x;
	const uint64_t r = nxz_bgzf_upper(poff, n + 1, p) - 1;             // (ranges without pieces share their poff with the next)
	const uint64_t j = rfirst[r] + (p - poff[r]);
	const uint64_t k = midx[j];
	if (k < k0 || k >= k0 + cnt) return;
	const uint64_t mb = uoff[j], me = uoff[j + 1], b0 = rb[r], e0 = b0 + rlen[r];
	const uint64_t a = mb > b0 ? mb : b0, e = me < e0 ? me : e0;
	const uint64_t kk = k - k0;
	if (frames[kk].status != NXZ_FRAME_OK || results[kk].tpbc != me - mb) {   // (an empty member inside the range counts too)
		if (blockIdx.y == 0 && threadIdx.x == 0) status[r] = NXZ_RANGE_DAMAGED;
		return;
	}
	const uint64_t lo = (uint64_t)blockIdx.y * WIN;
	if (a + lo >= e) return;
	const uint64_t len = e - a - lo < WIN ? e - a - lo : WIN;
	copy_bytes(dst + offsets[r] + (a - b0) + lo, slots + kk * stride + (a - mb) + lo, len);
}

__global__ __launch_bounds__(256) void zero_kernel(const uint64_t *__restrict__ offsets, const uint32_t *__restrict__ status, uint8_t *dst)
{
	const uint64_t r = blockIdx.x;
	if (status[r] != NXZ_RANGE_DAMAGED) return;
	for (uint64_t i = offsets[r] + threadIdx.x; i < offsets[r + 1]; i += 256) dst[i] = 0;
}

} // namespace nxzr

static size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

// The map's arrays inside ws: ctl (8), per range rb, rfirst, rlen, rpieces, poff (n + 1), per member diff (L + 1), midx, list
struct RangeWs {
	uint64_t *ctl, *rb, *rfirst, *rlen, *rpieces, *poff;
	int32_t *diff;
	uint32_t *midx, *list;
};
static RangeWs range_ws(uint8_t *ws, uint64_t n, uint64_t L)
{
	RangeWs w;
	uint8_t *p = ws;
	auto take = [&](size_t b) { uint8_t *q = p; p += up256(b); return q; };
	w.ctl = (uint64_t *)take(8 * 8);
	w.rb = (uint64_t *)take(n * 8); w.rfirst = (uint64_t *)take(n * 8); w.rlen = (uint64_t *)take(n * 8); w.rpieces = (uint64_t *)take(n * 8);
	w.poff = (uint64_t *)take((n + 1) * 8);
	w.diff = (int32_t *)take((L + 1) * 4);
	w.midx = (uint32_t *)take(L * 4 + 4); w.list = (uint32_t *)take(L * 4 + 4);
	return w;
}

extern "C" size_t nxz_bgzf_ranges_workspace(uint64_t n, uint64_t L)
{
	return up256(64) + 4 * up256(n * 8) + up256((n + 1) * 8) + up256((L + 1) * 4) + 2 * up256(L * 4 + 4);
}

// The map in two steps, for a caller that checks an index of its own kind between them (nxz_checkpoint.hip): _clear zeroes ctl and
// the difference array; the caller's check sets ctl[0] = ws[0] when its index is faulty; _ranges maps ranges in uncompressed
// offsets (no coff), scans the members (here: the caller's segments) and the ranges.
extern "C" int nxz_launch_range_map_clear(uint8_t *ws, uint64_t n, uint64_t L, hipStream_t stream)
{
	const RangeWs w = range_ws(ws, n, L);
	(void)hipMemsetAsync(w.ctl, 0, 8 * 8, stream);
	(void)hipMemsetAsync(w.diff, 0, (L + 1) * 4, stream);
	return (int)hipGetLastError();
}
static void range_map_steps(const uint64_t *coff, const uint64_t *uoff, uint64_t L, int kind, const nxz_bgzf_range_t *ranges, uint64_t n,
			    uint64_t *offsets, uint32_t *status, const RangeWs &w, hipStream_t stream)
{
	if (n)
		hipLaunchKernelGGL(nxzr::range_map_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, coff, uoff, L, kind, ranges, n, w.ctl,
				   status, w.rb, w.rfirst, w.rlen, w.rpieces, w.diff);
	if (L) hipLaunchKernelGGL(nxzr::member_scan_kernel, dim3(1), dim3(1024), 0, stream, w.diff, uoff, L, w.ctl, w.midx, w.list);
	hipLaunchKernelGGL(nxzr::range_scan_kernel, dim3(1), dim3(1024), 0, stream, w.rlen, w.rpieces, n, w.ctl, offsets, w.poff);
}
extern "C" int nxz_launch_range_map_ranges(const uint64_t *uoff, uint64_t L, const nxz_bgzf_range_t *ranges, uint64_t n, uint64_t *offsets,
					   uint32_t *status, uint8_t *ws, hipStream_t stream)
{
	range_map_steps(uoff, uoff, L, NXZ_RANGE_UOFF, ranges, n, offsets, status, range_ws(ws, n, L), stream);
	return (int)hipGetLastError();
}
// midx[j]: the place of member j among the needed ones (~0: not needed); list[k]: the k-th needed member
extern "C" void nxz_range_map_lists(uint8_t *ws, uint64_t n, uint64_t L, const uint32_t **midx, const uint32_t **list)
{
	const RangeWs w = range_ws(ws, n, L);
	*midx = w.midx; *list = w.list;
}

// The map: ws[0..4] (uint64, device) = faulty index, needed members, bytes of all ranges, pieces, largest needed member.
// L = nidx - 1 members; status / offsets written unless the index is faulty.
extern "C" int nxz_launch_bgzf_map(const uint8_t *packed, uint64_t packed_len, const uint64_t *coff, const uint64_t *uoff, uint64_t L, int kind,
				   const nxz_bgzf_range_t *ranges, uint64_t n, uint64_t *offsets, uint32_t *status, uint8_t *ws, hipStream_t stream)
{
	const RangeWs w = range_ws(ws, n, L);
	(void)nxz_launch_range_map_clear(ws, n, L, stream);
	if (L) hipLaunchKernelGGL(nxzr::index_check_kernel, dim3((unsigned)((L + 255) / 256)), dim3(256), 0, stream, packed, packed_len, coff, uoff, L, w.ctl);
	range_map_steps(coff, uoff, L, kind, ranges, n, offsets, status, w, stream);
	return (int)hipGetLastError();
}

// The framed jobs of needed members k0 .. k0 + cnt - 1, member k's output at slots + (k - k0) * stride
extern "C" int nxz_launch_bgzf_jobs(const uint8_t *packed, const uint64_t *coff, const uint64_t *uoff, uint64_t n, uint64_t L, uint8_t *ws,
				    uint64_t k0, uint64_t cnt, uint8_t *slots, uint64_t stride, nxz_batch_job_t *jobs, hipStream_t stream)
{
	const RangeWs w = range_ws(ws, n, L);
	if (cnt) hipLaunchKernelGGL(nxzr::job_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, stream, packed, coff, uoff, w.list, k0, cnt, slots, stride, jobs);
	return (int)hipGetLastError();
}

// The pieces of those members from their slots to dst (after the framed decode wrote frames / results of the chunk)
extern "C" int nxz_launch_bgzf_gather(const uint64_t *uoff, uint64_t n, uint64_t L, uint64_t pieces, uint8_t *ws, const uint64_t *offsets,
				      const uint8_t *slots, uint64_t stride, uint64_t k0, uint64_t cnt, const nxz_batch_frame_t *frames,
				      const nxz_batch_result_t *results, uint8_t *dst, uint32_t *status, hipStream_t stream)
{
	const RangeWs w = range_ws(ws, n, L);
	const uint64_t parts = (stride + nxzr::WIN - 1) / nxzr::WIN;
	if (!pieces || !cnt) return 0;
	if (pieces >= (1ull << 31) || parts > 65535) return (int)hipErrorInvalidValue;
	hipLaunchKernelGGL(nxzr::gather_kernel, dim3((unsigned)pieces, (unsigned)parts), dim3(256), 0, stream, uoff, w.midx, w.poff, n, w.rb, w.rfirst,
			   w.rlen, offsets, slots, stride, k0, cnt, frames, results, dst, status);
	return (int)hipGetLastError();
}

extern "C" int nxz_launch_bgzf_zero(uint64_t n, const uint64_t *offsets, const uint32_t *status, uint8_t *dst, hipStream_t stream)
{
	if (!n) return 0;
	if (n >= (1ull << 31)) return (int)hipErrorInvalidValue;
	hipLaunchKernelGGL(nxzr::zero_kernel, dim3((unsigned)n), dim3(256), 0, stream, offsets, status, dst);
	return (int)hipGetLastError();
}
