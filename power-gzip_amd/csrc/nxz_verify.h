// nxz_verify.h -- the rules of the batched verify (nxz_batch_decompress_verify[_framed], include/nxz_engine.h) as plain code that
// compiles for the device (nxz_inflate_verify.hip) and for the host (tests/native/verify_host.cpp, which runs it "as 64 lanes would").
// The kernel is the size walk with the ring of nxz_checkpoint_build.h: the last 32 KiB of output in LDS, output byte u at ring
// position u mod 32768.  This file adds what checksumming the output on its way through the ring needs:
//   the budget   the walk is cut every PASS bytes of output at the latest (budget); at a cut, at output u, one pass takes the whole
//                64-byte slices of [done, u & ~63) -- `done` is a multiple of 64, so a slice is aligned in the ring and never lies
//                across its wrap -- and sets done to that.  u <= cut + PASS and done > cut - 64: a pass is at most PASS / 64 slices
//                and every byte of it is less than PASS + 64 <= 32768 behind u, still in the ring.
//   a pass       lane l of 64 takes slices l, l + 64, l + 128, l + 192 of the pass (nxzck::PER_LANE of them, four CRC states side by
//                side), weighs them with nxz_cksum_slices.h's rules (a slice followed by k more is multiplied by CRC_POW[k]; the
//                Adler terms are reduced mod 65521 a slice), and the lanes' parts are XORed / added (lane_pass);
//   the join     the running CRC state is the seed of the pass's first slice; the Adler pair (s1, s2) in front of a pass of n bytes
//                adds n * s1 to s2 (join).  Behind the walk one more pass, then the last 0..63 bytes by one serial chain (tail).
#ifndef NXZ_VERIFY_H
#define NXZ_VERIFY_H
#include <stdint.h>
#include "nxz_cksum_slices.h"
#include "nxz_checkpoint_build.h"

namespace nxzv {

constexpr uint32_t LANES = 64;                                         // one wavefront a job
constexpr uint32_t PASS = LANES * nxzck::PER_LANE * nxzck::SLICE;      // bytes of output between two cuts at most: 16 KiB
static_assert(PASS % nxzck::SLICE == 0 && PASS + nxzck::SLICE <= NXZ_CB_RING, "every byte of a pass is still in the ring");

// The running checksums of a job: crc is the raw register state (the seed XOR ~0 in front of the first byte), s1 and s2 are below
// 65521; cut: the output at the last cut; done: the bytes checksummed so far (whole slices until the tail).
struct State { uint32_t cut, done, crc, s1, s2; };

NXZ_CK_FN State begin(uint32_t in_crc, uint32_t in_adler)
{
	State s;
	s.cut = 0; s.done = 0;
	s.crc = in_crc ^ 0xffffffffu;
	s.s1 = (in_adler & 0xffff) % nxzck::ADLER_MOD; s.s2 = (in_adler >> 16) % nxzck::ADLER_MOD;
	return s;
}

// ---- the geometry ------------------------------------------------------------------------------------------------------------
// the output the walk may reach before the next cut: cap itself once a pass's worth reaches it (no cut is made then, the walk ends
// at cap as it does without a hook)
NXZ_CK_FN uint32_t budget(uint32_t cut, uint32_t cap)
{
	const uint64_t b = (uint64_t)cut + PASS;
	return b >= cap ? cap : (uint32_t)b;
}
// the slices of the pass at output u: [done, done + 64 * that)
NXZ_CK_FN uint32_t pass_slices(uint32_t done, uint32_t u) { return ((u & ~(nxzck::SLICE - 1)) - done) / nxzck::SLICE; }

// ---- a pass --------------------------------------------------------------------------------------------------------------------
struct Part { uint32_t crc, s1, s2; };        // XOR over the lanes; plain sums (s1 <= 4 x 64 x 255 a lane, s2 four terms below 65521)

// Lane `lane` of LANES in a pass of ns slices (1..256) from output byte `done` on: ring is the 32 KiB ring as dwords (16-byte aligned), crc the running
// state (it seeds slice 0), T the slice-by-4 table (nxzck::table_column).  A slice this lane has not is read as zeros, which leave
// its zero state alone.
NXZ_CK_FN Part lane_pass(const uint32_t *ring, uint32_t done, uint32_t ns, uint32_t crc, uint32_t lane, const uint32_t *T)
{
	Part p = { 0, 0, 0 };
	if (lane >= ns) return p;
	const uint32_t n = ns * nxzck::SLICE;
	uint32_t c[nxzck::PER_LANE], S[nxzck::PER_LANE], W[nxzck::PER_LANE], at[nxzck::PER_LANE];
#pragma unroll
	for (uint32_t k = 0; k < nxzck::PER_LANE; k++) {
		const uint32_t j = lane + LANES * k;
		at[k] = nxz_cb_ring_pos(done + j * nxzck::SLICE) / 4;          // (j >= ns: a place in the ring all the same, never read)
		c[k] = j == 0 ? crc : 0; S[k] = 0; W[k] = 0;
	}
#pragma unroll
	for (uint32_t q = 0; q < nxzck::SLICE / 16; q++) {
		nxzck::ck_v4u v[nxzck::PER_LANE];
#pragma unroll
		for (uint32_t k = 0; k < nxzck::PER_LANE; k++) {
			v[k] = (nxzck::ck_v4u){ 0, 0, 0, 0 };
			if (lane + LANES * k < ns) v[k] = *(const nxzck::ck_v4u *)(ring + at[k] + 4 * q);     // (16-byte aligned: one ds_read_b128)
		}
#pragma unroll
		for (uint32_t d = 0; d < 4; d++) {
#pragma unroll
			for (uint32_t k = 0; k < nxzck::PER_LANE; k++) {
				nxzck::adler_dword(v[k][d], 4 * q + d, S[k], W[k]);
				c[k] = nxzck::crc_dword(T, c[k], v[k][d]);
			}
		}
	}
#pragma unroll
	for (uint32_t k = 0; k < nxzck::PER_LANE; k++) {
		const uint32_t j = lane + LANES * k;
		if (j >= ns) break;
		p.crc ^= nxzck::gf_mul(c[k], nxzck::CRC_POW.v[ns - 1 - j]);
		p.s1 += S[k];
		p.s2 += (S[k] * (n - j * nxzck::SLICE) - W[k]) % nxzck::ADLER_MOD;    // (S <= 16 320, n <= 16 384: below 2^32)
	}
	return p;
}

// ---- the joins -----------------------------------------------------------------------------------------------------------------
// the lanes' parts of a pass of ns slices, XORed and summed, go into the running state (ns == 0: nothing changes)
NXZ_CK_FN void join(State &s, uint32_t ns, uint32_t crc, uint32_t s1, uint32_t s2)
{
	if (!ns) return;
	const uint32_t n = ns * nxzck::SLICE;
	s.crc = crc;
	s.s2 = (uint32_t)(((uint64_t)s.s2 + (uint64_t)n * s.s1 + s2) % nxzck::ADLER_MOD);
	s.s1 = (s.s1 + s1) % nxzck::ADLER_MOD;
	s.done += n;
}

// the last r = 0..63 bytes, from output byte s.done (a multiple of 64) on: one serial chain, whole dwords first
NXZ_CK_FN void tail(State &s, const uint32_t *ring, uint32_t r, const uint32_t *T)
{
	const uint32_t a = nxz_cb_ring_pos(s.done);
	const uint8_t *const rb = (const uint8_t *)ring;
	uint32_t c = s.crc, St = 0, Wt = 0;
	const uint32_t nd = r >> 2;
	for (uint32_t k = 0; k < nd; k++) {
		const uint32_t w = ring[a / 4 + k];
		nxzck::adler_dword(w, k, St, Wt);
		c = nxzck::crc_dword(T, c, w);
	}
	for (uint32_t k = 4 * nd; k < r; k++) {
		const uint32_t b = rb[a + k];
		St += b; Wt += b * k;
		c = nxzck::crc_byte(T, c, b);
	}
	s.crc = c;
	s.s2 = (s.s2 + r * s.s1 + St * r - Wt) % nxzck::ADLER_MOD;           // (63 x 65520 + 63 x 255 x 63: far below 2^32)
	s.s1 = (s.s1 + St) % nxzck::ADLER_MOD;
	s.done += r;
}

NXZ_CK_FN uint32_t crc_of(const State &s) { return s.crc ^ 0xffffffffu; }
NXZ_CK_FN uint32_t adler_of(const State &s) { return (s.s2 << 16) | s.s1; }

} // namespace nxzv
#endif
