// nxz_shuffle.hip -- the byte-shuffle filter on device buffers (nxz_batch_shuffle / nxz_batch_unshuffle, include/nxz_engine.h; the
// rules, the tile and the LDS layout are nxz_shuffle.h's).  One grid over the tiles of all jobs: workgroup g finds its job in the
// tile prefix first[] and takes T elements of it.  A tile has a CONTIGUOUS side (T * elem bytes of elements: the source of a shuffle,
// the target of an unshuffle) and a PLANES side (elem runs of T bytes, run j at + j * N: any alignment each).  Both sides move in
// 16-byte slots on 16-byte boundaries of global memory, a vector where the slot lies inside the run and byte by byte where the run
// begins or ends inside it -- nothing outside a run is read or written.  Between them the tile lies in LDS as planes, plane j shifted
// by the low four bits of its run's address, so that the planes side is 16-byte vectors on both ends; the contiguous side scatters
// (shuffle) or gathers (unshuffle) its slot's 16 bytes one by one.  No thread leaves before the last barrier.
#include <hip/hip_runtime.h>
#include "nxz_device.h"
#include "nxz_shuffle.h"

namespace nxzsh {
typedef uint32_t v4 __attribute__((ext_vector_type(4)));
typedef NXZ_GLOBAL_AS uint8_t *gptr;
static_assert(NXZ_SHUFFLE_ELEM_MAX == 256, "a thread a plane fills the plane table");

// ELEM: the element size as a constant (2, 4, 8, 16), or 0: `elem_rt`, any size from 1 to 256.  Elements e0 .. e0 + cnt - 1 of the job.
template <uint32_t ELEM, bool UNDO>
__device__ __forceinline__ void tile_body(uint8_t *lds, const uint32_t *pbase, const nxz_shuffle_plan_t &p, uint32_t elem_rt, uint64_t e0, uint32_t cnt)
{
	const uint32_t t = threadIdx.x;
	const uint32_t elem = ELEM ? ELEM : elem_rt;
	const uint32_t T = nxz_shuffle_tile_elems_of(elem), stride = T + 16, S = nxz_shuffle_plane_slots(T);
	const uint64_t N = p.n_elems;
	const gptr C = (gptr)(UNDO ? p.dst : const_cast<uint8_t *>(p.src)) + e0 * elem;      // the contiguous side
	const gptr P = (gptr)(UNDO ? const_cast<uint8_t *>(p.src) : p.dst) + e0;             // plane 0's run
	const uint32_t L = cnt * elem;

	// byte k of the contiguous side is byte i = k / elem of plane j = k % elem: lds[pbase[j] + i]
	auto contig = [&]() {
		const uint32_t ca = (uint32_t)(uintptr_t)C & 15, ns = (ca + L + 15) >> 4;
		for (uint32_t s = t; s < ns; s += 256) {
			const int32_t k0 = (int32_t)(16 * s) - (int32_t)ca;
			if (k0 >= 0 && (uint32_t)k0 + 16 <= L) {
				uint32_t j = (uint32_t)k0 % elem, i = (uint32_t)k0 / elem;
				v4 v = {0, 0, 0, 0};
				if (!UNDO) v = *(const NXZ_GLOBAL_AS v4 *)(C + k0);
#pragma unroll
				for (int q = 0; q < 16; q++) {
					if (ELEM) { j = ((uint32_t)k0 + q) % elem; i = ((uint32_t)k0 + q) / elem; }
					if (!UNDO) lds[pbase[j] + i] = (uint8_t)(v[q >> 2] >> (8 * (q & 3)));
					else v[q >> 2] |= (uint32_t)lds[pbase[j] + i] << (8 * (q & 3));
					if (!ELEM && ++j == elem) { j = 0; i++; }
				}
				if (UNDO) *(NXZ_GLOBAL_AS v4 *)(C + k0) = v;
			} else {
				for (int q = 0; q < 16; q++) {
					const int32_t k = k0 + q;
					if (k < 0 || (uint32_t)k >= L) continue;
					const uint32_t a = pbase[(uint32_t)k % elem] + (uint32_t)k / elem;
					if (!UNDO) lds[a] = C[k]; else C[k] = lds[a];
				}
			}
		}
	};
	// slot s of plane j: 16 bytes of LDS at j * stride + 16 s, bytes i0 .. i0 + 15 of the run
	auto planes = [&]() {
		for (uint32_t w = t; w < elem * S; w += 256) {
			const uint32_t j = w / S, s = w - j * S;
			const gptr Pj = P + (uint64_t)j * N;
			const int32_t i0 = (int32_t)(16 * s) - (int32_t)((uint32_t)(uintptr_t)Pj & 15);
			if (i0 >= (int32_t)cnt) continue;
			uint8_t *const l = lds + j * stride + 16 * s;
			if (i0 >= 0 && (uint32_t)i0 + 16 <= cnt) {
				if (!UNDO) *(NXZ_GLOBAL_AS v4 *)(Pj + i0) = *(const v4 *)l;
				else *(v4 *)l = *(const NXZ_GLOBAL_AS v4 *)(Pj + i0);
			} else {
				for (int q = 0; q < 16; q++) {
					const int32_t i = i0 + q;
					if (i < 0 || (uint32_t)i >= cnt) continue;
					if (!UNDO) Pj[i] = l[q]; else l[q] = Pj[i];
				}
			}
		}
	};
	if (UNDO) planes(); else contig();
	__syncthreads();
	if (UNDO) contig(); else planes();
}

template <bool UNDO>
__global__ __launch_bounds__(256) void shuffle_kernel(const nxz_shuffle_plan_t *__restrict__ plan, const uint32_t *__restrict__ first, uint32_t n)
{
	__shared__ v4 planes4[NXZ_SHUFFLE_PLANES_BYTES / 16];
	__shared__ uint32_t pbase[NXZ_SHUFFLE_ELEM_MAX];
	uint8_t *const lds = (uint8_t *)planes4;
	const uint32_t t = threadIdx.x, g = blockIdx.x;
	// the job of tile g: the first whose tiles end behind it (the grid has exactly first[n] workgroups)
	uint32_t lo = 0, hi = n - 1;
	while (lo < hi) {
		const uint32_t mid = lo + (hi - lo) / 2;
		if (first[mid + 1] > g) hi = mid; else lo = mid + 1;
	}
	const nxz_shuffle_plan_t p = plan[lo];
	const uint32_t elem = p.elem, T = nxz_shuffle_tile_elems_of(elem);
	const uint64_t e0 = (uint64_t)(g - first[lo]) * T;
	const uint32_t cnt = p.n_elems - e0 < T ? (uint32_t)(p.n_elems - e0) : T;
	// where plane t begins in LDS: its region, shifted as its run is in global memory
	if (t < elem) pbase[t] = t * (T + 16) + (((uint32_t)(uintptr_t)(UNDO ? p.src : p.dst) + (uint32_t)e0 + t * (uint32_t)p.n_elems) & 15);
	__syncthreads();
	switch (elem) {
	case 2: tile_body<2, UNDO>(lds, pbase, p, elem, e0, cnt); break;
	case 4: tile_body<4, UNDO>(lds, pbase, p, elem, e0, cnt); break;
	case 8: tile_body<8, UNDO>(lds, pbase, p, elem, e0, cnt); break;
	case 16: tile_body<16, UNDO>(lds, pbase, p, elem, e0, cnt); break;
	default: tile_body<0, UNDO>(lds, pbase, p, elem, e0, cnt); break;
	}
	// the job's last tile: the bytes behind the elements, unchanged
	if (e0 + cnt == p.n_elems && t < p.tail) {
		const uint64_t at = p.n_elems * elem + t;
		((gptr)p.dst)[at] = ((const NXZ_GLOBAL_AS uint8_t *)p.src)[at];
	}
}

__global__ __launch_bounds__(256) void shuffle_status_kernel(const uint32_t *__restrict__ st, uint32_t n, uint32_t *__restrict__ status)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i < n) status[i] = st[i];
}
} // namespace nxzsh

// plan[n], first[n + 1], st[n]: the host's pass (nxz_shuffle_plan_batch) in device memory; tiles = first[n]
extern "C" int nxz_launch_shuffle(const nxz_shuffle_plan_t *plan, const uint32_t *first, const uint32_t *st, uint32_t n, uint32_t tiles, int undo,
				  uint32_t *status, hipStream_t stream)
{
	if (!n) return 0;
	hipLaunchKernelGGL(nxzsh::shuffle_status_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, st, n, status);
	if (tiles && undo) hipLaunchKernelGGL(nxzsh::shuffle_kernel<true>, dim3(tiles), dim3(256), 0, stream, plan, first, n);
	else if (tiles) hipLaunchKernelGGL(nxzsh::shuffle_kernel<false>, dim3(tiles), dim3(256), 0, stream, plan, first, n);
	return (int)hipGetLastError();
}
