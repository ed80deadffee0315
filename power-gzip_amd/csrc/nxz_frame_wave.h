// nxz_frame_wave.h -- the `Ops` of nxz_frame.h's header parser for a wavefront, device only: the two steps that use all 64 lanes
// (every lane runs the parser on the same bytes).  For the header kernels of nxz_frame.hip and the index kernels of
// nxz_gzip_members.hip and nxz_checkpoint.hip.
#ifndef NXZ_FRAME_WAVE_H
#define NXZ_FRAME_WAVE_H
#include <hip/hip_runtime.h>
#include "nxz_device.h"
#include "nxz_frame.h"

struct WaveOps {
	uint32_t lane;
	__device__ uint32_t find_nul(const uint8_t *p, uint32_t from, uint32_t len)
	{
		for (uint32_t q = from; q < len; q += 64) {
			const uint32_t i = q + lane;
			const uint64_t m = __ballot(i < len && p[i] == 0);
			if (m) return q + (uint32_t)__builtin_ctzll(m);
		}
		return len;
	}
	__device__ uint32_t crc32(const uint8_t *p, uint32_t n)
	{
		uint32_t lo, hi;
		nxz_slice(n, 64, lane, &lo, &hi);
		uint32_t v = nxz_crc_part(p, lo, hi, n);
		for (int o = 32; o > 0; o >>= 1) v ^= (uint32_t)__shfl_xor((int)v, o, 64);
		return nxz_crc_finish(v, n);
	}
};

#endif
