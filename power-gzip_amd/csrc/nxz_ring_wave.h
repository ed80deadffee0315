// nxz_ring_wave.h -- one wavefront writes the tokens of nxzs::walk (nxz_inflate_walk.h, a hook with `bytes`) into a ring of the last
// 32 KiB of output in LDS.  The ring's rules are nxz_checkpoint_build.h's; the writers are shared by nxz_checkpoint_build.hip (the ring
// is dumped where a checkpoint is stored) and nxz_inflate_verify.hip (the ring is checksummed as the output passes through it).
// Literals a lane each; a match by the whole wavefront: all its loads, then all its stores, so that a copy that feeds on itself or
// lies across the wrap reads what stood there before; stored runs from src, four bytes a lane.  Device code only.
#ifndef NXZ_RING_WAVE_H
#define NXZ_RING_WAVE_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "nxz_device.h"
#include "nxz_inflate_decode.h"
#include "nxz_checkpoint_build.h"

namespace nxzr {

using nxzi::uni;

typedef uint32_t u32_any __attribute__((aligned(1)));

// p[0, len) -> ring [rs, rs + len) (no wrap inside): the dwords that lie whole inside the piece by dword stores (the loads at whatever
// alignment p has: device memory takes them), the bytes in front and behind one by one
__device__ __forceinline__ void ring_in(uint32_t *ring, uint32_t rs, uint32_t len, const NXZ_GLOBAL_AS uint8_t *p, int lane)
{
	uint8_t *const rb = (uint8_t *)ring;
	uint32_t head = (4 - (rs & 3)) & 3;
	if (head > len) head = len;
	const uint32_t body = (len - head) >> 2;
	if ((uint32_t)lane < head) rb[rs + lane] = p[lane];
	for (uint32_t g = lane; g < body; g += 64) ring[((rs + head) >> 2) + g] = *(const NXZ_GLOBAL_AS u32_any *)(p + head + 4 * g);
	const uint32_t done = head + 4 * body;
	if (done + (uint32_t)lane < len) rb[rs + done + lane] = p[done + lane];
}

// The `bytes` members of a walk hook (nxz_inflate_walk.h): a hook that keeps the ring derives from this.
struct Writer {
	uint32_t *ring;                      // NXZ_CB_RING bytes of LDS
	int lane;

	// a lane with `on` set holds the literal of output byte `at`
	__device__ __forceinline__ void lit(bool on, uint32_t at, uint32_t sym) const
	{
		if (on) ((uint8_t *)ring)[nxz_cb_ring_pos(at)] = (uint8_t)sym;
	}

	// a lane a byte, five rounds at most (len <= 258): every source byte lies in front of `at`, and all loads go before the first store
	__device__ __forceinline__ void match(uint32_t at, uint32_t dist, uint32_t len) const
	{
		at = uni(at); dist = uni(dist); len = uni(len);
		uint8_t *const rb = (uint8_t *)ring;
		const bool self = dist < len;
		const uint32_t m = self ? nxz_cb_recip(dist) : 0;
		if (len <= 64) {
			const uint32_t i = self ? nxz_cb_mod((uint32_t)lane, dist, m) : (uint32_t)lane;
			const uint32_t v = (uint32_t)lane < len ? rb[nxz_cb_ring_pos(at - dist + i)] : 0;
			if ((uint32_t)lane < len) rb[nxz_cb_ring_pos(at + lane)] = (uint8_t)v;
			return;
		}
		uint32_t v[5];
#pragma unroll
		for (int k = 0; k < 5; k++) {
			const uint32_t i = lane + 64 * k;
			const uint32_t r = self ? nxz_cb_mod(i, dist, m) : i;
			v[k] = (k < 2 || len > 64u * k) && i < len ? rb[nxz_cb_ring_pos(at - dist + r)] : 0;
		}
#pragma unroll
		for (int k = 0; k < 5; k++) {
			const uint32_t i = lane + 64 * k;
			if ((k < 2 || len > 64u * k) && i < len) rb[nxz_cb_ring_pos(at + i)] = (uint8_t)v[k];
		}
	}

	// n stored bytes at p are output bytes `at` on (a run longer than the ring leaves its last 32 KiB)
	__device__ __forceinline__ void stored(uint32_t at, const NXZ_GLOBAL_AS uint8_t *p, uint32_t n) const
	{
		const uint32_t skip = (uint32_t)nxz_cb_run_skip(uni(n));
		const nxz_cb_pieces_t r = nxz_cb_run((uint64_t)uni(at) + skip, uni(n) - skip);
		ring_in(ring, r.start[0], r.len[0], p + skip, lane);
		if (r.len[1]) ring_in(ring, r.start[1], r.len[1], p + skip + r.len[0], lane);
	}
};

} // namespace nxzr
#endif
