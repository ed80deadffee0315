// nxz_shuffle.h -- the rules of nxz_batch_shuffle / nxz_batch_unshuffle (include/nxz_engine.h: the byte-shuffle filter of HDF5 and
// numcodecs on device buffers) as plain code that compiles for the device (nxz_shuffle.hip), for the engine's host side
// (nxz_batch_streams.cpp) and for a host test program (tests/native/shuffle_host.cpp).
//
//   the transform   N = len / elem elements, r = len % elem bytes behind them.  dst[j * N + i] = src[i * elem + j] (i < N, j < elem);
//                   the r bytes go unchanged to dst[N * elem ..]; unshuffle is the inverse under the same (len, elem).  elem == 1 and
//                   len < elem are plain copies: the plan turns them into elements of one byte, so the kernel knows one form only;
//   the refusals    src or dst NULL with len != 0, elem == 0 or > NXZ_SHUFFLE_ELEM_MAX, reserved != 0, overlapping byte ranges;
//   the tiles       a workgroup takes T = nxz_shuffle_tile_elems(elem) elements: the most that fit NXZ_SHUFFLE_TILE_BYTES, rounded down
//                   to a multiple of 16 (never below 64: elem <= 256).  A job has ceil(N / T) tiles, first[i] are the tiles in front of
//                   job i, and the workgroup of a job's last tile also copies its r bytes;
//   which path      elem 2, 4, 8 and 16 run the kernel with the element size as a constant (byte -> plane by mask and shift, the slot
//                   bound a constant divisor); every other size from 1 to 256 -- the copies as elem 1 -- runs the generic path, which
//                   divides once per 16 bytes and steps from byte to byte;
//   the LDS         a tile lies in LDS as planes: plane j at j * (T + 16), shifted by the low four bits of its address in global
//                   memory, so that a 16-byte aligned vector of the plane in global memory is a 16-byte aligned vector in LDS.
//                   elem * (T + 16) <= NXZ_SHUFFLE_TILE_BYTES + 16 * NXZ_SHUFFLE_ELEM_MAX bytes, and a table of 256 plane offsets:
//                   NXZ_SHUFFLE_LDS_BYTES in all.
#ifndef NXZ_SHUFFLE_H
#define NXZ_SHUFFLE_H
#include <stdint.h>
#include <stddef.h>
#include "../../include/nxz_engine.h"

#if defined(__HIPCC__)
#define NXZ_SHUFFLE_HD __host__ __device__
#else
#define NXZ_SHUFFLE_HD
#endif

#define NXZ_SHUFFLE_TILE_BYTES 16384u
#define NXZ_SHUFFLE_PLANES_BYTES (NXZ_SHUFFLE_TILE_BYTES + 16u * NXZ_SHUFFLE_ELEM_MAX)
#define NXZ_SHUFFLE_LDS_BYTES (NXZ_SHUFFLE_PLANES_BYTES + 4u * NXZ_SHUFFLE_ELEM_MAX)

/* what the kernel reads of a job: a refused or empty job has no elements and no tail, a copy has elements of one byte */
typedef struct nxz_shuffle_plan {
	const uint8_t *src;
	uint8_t       *dst;
	uint64_t       n_elems;
	uint32_t       elem;          /* 1 .. NXZ_SHUFFLE_ELEM_MAX */
	uint32_t       tail;          /* the r bytes behind the elements, < elem */
} nxz_shuffle_plan_t;

/* ---- the tiles ---- */
NXZ_SHUFFLE_HD inline uint32_t nxz_shuffle_tile_elems_of(uint32_t elem) { return (NXZ_SHUFFLE_TILE_BYTES / elem) & ~15u; }
NXZ_SHUFFLE_HD inline uint64_t nxz_shuffle_tiles(uint64_t n_elems, uint32_t elem)
{
	const uint32_t T = nxz_shuffle_tile_elems_of(elem);
	return n_elems / T + (n_elems % T ? 1 : 0);
}
/* the 16-byte slots a plane's run of a tile touches at most: T bytes from any of the 16 alignments */
NXZ_SHUFFLE_HD inline uint32_t nxz_shuffle_plane_slots(uint32_t T) { return T / 16 + 1; }

/* ---- the refusals ---- */
/* do [a, a + len) and [b, b + len) share a byte?  (ranges that touch do not; empty ranges never do) */
NXZ_SHUFFLE_HD inline bool nxz_shuffle_overlap(uint64_t a, uint64_t b, uint64_t len)
{
	return a <= b ? b - a < len : a - b < len;
}
/* 0, or the status of a job that is not taken */
NXZ_SHUFFLE_HD inline uint32_t nxz_shuffle_refusal(const nxz_shuffle_job_t *j)
{
	if (j->elem == 0 || j->elem > NXZ_SHUFFLE_ELEM_MAX || j->reserved != 0) return NXZ_CC_INVALID_OP;
	if (j->len != 0 && (!j->src || !j->dst)) return NXZ_CC_INVALID_OP;
	if (nxz_shuffle_overlap((uint64_t)(uintptr_t)j->src, (uint64_t)(uintptr_t)j->dst, j->len)) return NXZ_CC_INVALID_OP;
	return 0;
}

/* ---- the plan of one job: its status; *p is what the kernel gets ---- */
NXZ_SHUFFLE_HD inline uint32_t nxz_shuffle_plan_job(const nxz_shuffle_job_t *j, nxz_shuffle_plan_t *p)
{
	const uint32_t st = nxz_shuffle_refusal(j);
	p->src = j->src; p->dst = j->dst; p->n_elems = 0; p->elem = 1; p->tail = 0;
	if (st) return st;
	if (j->elem == 1 || j->len < j->elem) { p->n_elems = j->len; return 0; }
	p->elem = j->elem; p->n_elems = j->len / j->elem; p->tail = (uint32_t)(j->len % j->elem);
	return 0;
}

/* ---- the host's one pass: plan[n], first[n + 1], status[n].  The tiles in all, or -1 once they reach 2^31 (a grid's limit; 32 TiB
 * of elements at the least: nothing is queued, -E2BIG) ---- */
inline int64_t nxz_shuffle_plan_batch(const nxz_shuffle_job_t *jobs, size_t n, nxz_shuffle_plan_t *plan, uint32_t *first, uint32_t *status)
{
	uint64_t total = 0;
	for (size_t i = 0; i < n; i++) {
		first[i] = (uint32_t)total;
		status[i] = nxz_shuffle_plan_job(&jobs[i], &plan[i]);
		const uint64_t tiles = nxz_shuffle_tiles(plan[i].n_elems, plan[i].elem);
		if (tiles >= (1ull << 31) || (total += tiles) >= (1ull << 31)) return -1;
	}
	first[n] = (uint32_t)total;
	return (int64_t)total;
}
#endif
