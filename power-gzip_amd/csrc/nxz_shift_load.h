// nxz_shift_load.h -- 16 bytes from any address through aligned 16-byte loads joined by a byte shift: what the staging kernels of
// nxz_streams_part.hip (a first block's window) and nxz_inflate_part.hip (window, tail and part of a stream read in parts) move their
// bytes with, one copy.  Device code only.
#ifndef NXZ_SHIFT_LOAD_H
#define NXZ_SHIFT_LOAD_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nxz {

// out = the 16 bytes at byte `sh` (1 .. 15) of the 32 bytes [lo][hi]
__device__ inline uint4 shift_bytes(const uint4 lo, const uint4 hi, uint32_t sh)
{
	uint64_t q0 = lo.x | (uint64_t)lo.y << 32, q1 = lo.z | (uint64_t)lo.w << 32, q2 = hi.x | (uint64_t)hi.y << 32;
	const uint64_t q3 = hi.z | (uint64_t)hi.w << 32;
	if (sh >= 8) { q0 = q1; q1 = q2; q2 = q3; sh -= 8; }
	const uint32_t s = sh * 8;
	const uint64_t a = s ? q0 >> s | q1 << (64 - s) : q0, b = s ? q1 >> s | q2 << (64 - s) : q1;
	return make_uint4((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32));
}

// The 16 bytes at p, all of which the caller may read: they lie in the one or two aligned 16-byte pieces that hold the first and the
// last of them -- both hold bytes of the 16, so no load touches a piece that holds none.
__device__ inline uint4 load16_any(const uint8_t *p)
{
	const uint32_t sh = (uint32_t)(uintptr_t)p & 15;
	const uint4 *const a = (const uint4 *)(p - sh);
	return sh ? shift_bytes(a[0], a[1], sh) : a[0];
}

} // namespace nxz
#endif
