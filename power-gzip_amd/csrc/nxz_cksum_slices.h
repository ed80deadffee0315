// nxz_cksum_slices.h -- CRC-32 and Adler-32 of a job's source, cut into 64-byte slices that the lanes of a workgroup
// take side by side (the entropy kernel, nxz_encode.hip, for the blocks it encodes; the GF(2) weights are also what the
// LZ77 kernel's own checksum phase, nxz_lz77.hip, multiplies with).  Plain functions over a byte pointer and a lane /
// slice index: __device__ code under hipcc, host C++ otherwise, so that the CPU test (tests/test_cksum_slices_host.py)
// runs exactly this arithmetic "as 256 lanes would".
//
// The stream of n bytes is slices 0 .. K1 of 64 bytes, K1 = (n - 1) / 64; the last one, the tail, holds r = 1..64 bytes.
//   CRC-32   every slice gets a raw CRC of its own (state 0 in front of it; slice 0 starts from in_crc ^ ~0 instead,
//            which is the seed XORed in front of the first data byte).  A state followed by L more bytes weighs x^(8 L)
//            mod P: the full slice j is multiplied by x^(512 (K1 - 1 - j)) (CRC_POW), the products are XORed -- lane,
//            wavefront, workgroup, the reduce is linear --, the sum takes x^(8 r) once (CRC_POW8) and the tail's CRC joins.
//   Adler-32 S = sum of a slice's bytes, Wt = sum of byte * (offset in the slice); the byte at stream offset i weighs
//            (n - i) in the second sum, so a slice at offset a adds S to s1 and S * (n - a) - Wt to s2.  That is below
//            2^32 for one slice of a 64 KiB stream (64 * 255 * 65536) and not for two: it is reduced mod 65521 per slice,
//            BEFORE any sum over slices or lanes.
#ifndef NXZ_CKSUM_SLICES_H
#define NXZ_CKSUM_SLICES_H
#include <stdint.h>
#ifdef __HIPCC__
#define NXZ_CK_FN __device__ __forceinline__
#define NXZ_CK_TABLE __device__ const
#define NXZ_CK_GLOBAL __attribute__((address_space(1)))        // job buffers are device memory: global_load, not flat_load
#define NXZ_CK_UDOT4(a, b, c) __builtin_amdgcn_udot4(a, b, c, false)
#else
#define NXZ_CK_FN inline
#define NXZ_CK_TABLE static const
#define NXZ_CK_GLOBAL
static inline uint32_t nxz_ck_udot4(uint32_t a, uint32_t b, uint32_t c)
{
	for (int k = 0; k < 4; k++) c += ((a >> (8 * k)) & 0xff) * ((b >> (8 * k)) & 0xff);
	return c;
}
#define NXZ_CK_UDOT4(a, b, c) nxz_ck_udot4(a, b, c)
#endif

namespace nxzck {

constexpr uint32_t POLY = 0xedb88320u;       // CRC-32, reflected
constexpr uint32_t ADLER_MOD = 65521u;
constexpr uint32_t SLICE = 64;               // bytes
constexpr uint32_t LANES = 256;              // lanes that share a stream (the entropy kernel's workgroup)
constexpr uint32_t PER_LANE = 4;             // consecutive full slices of a lane: 4 x 256 >= 1023, a 64 KiB stream's

// GF(2)[x] multiply modulo the reflected CRC-32 polynomial
NXZ_CK_FN uint32_t gf_mul(uint32_t a, uint32_t b)
{
	uint32_t r = 0;
#pragma unroll 8
	for (int i = 0; i < 32; i++) {
		r ^= (b & 0x80000000u) ? a : 0;
		a = (a >> 1) ^ ((a & 1) ? POLY : 0);
		b <<= 1;
	}
	return r;
}

// x^(8*64*k) mod P for k = 0..1023 (compile-time): what a 64-byte slice that is followed by k
// more slices has to be multiplied with.
constexpr uint32_t cgf_mul(uint32_t a, uint32_t b)
{
	uint32_t r = 0;
	for (int i = 0; i < 32; i++) {
		if (b & 0x80000000u) r ^= a;
		a = (a >> 1) ^ ((a & 1) ? POLY : 0);
		b <<= 1;
	}
	return r;
}
struct PowTab { uint32_t v[1024]; };
constexpr PowTab make_pow()
{
	PowTab p{};
	uint32_t m = 0x00800000u;                 // x^8
	for (int k = 0; k < 6; k++) m = cgf_mul(m, m);   // x^512
	p.v[0] = 0x80000000u;
	for (int i = 1; i < 1024; i++) p.v[i] = cgf_mul(p.v[i - 1], m);
	return p;
}
NXZ_CK_TABLE PowTab CRC_POW = make_pow();
// x^(8 r) mod P for r = 0..64
struct Pow8Tab { uint32_t v[65]; };
constexpr Pow8Tab make_pow8()
{
	Pow8Tab p{};
	p.v[0] = 0x80000000u;
	for (int i = 1; i <= 64; i++) p.v[i] = cgf_mul(p.v[i - 1], 0x00800000u);
	return p;
}
NXZ_CK_TABLE Pow8Tab CRC_POW8 = make_pow8();

// The slice-by-4 table, 1024 dwords: T[k * 256 + i] = i advanced by k + 1 zero bytes.  Lane i of 256 makes its four.
NXZ_CK_FN void table_column(uint32_t *T, uint32_t i)
{
	uint32_t c = i;
	for (int k = 0; k < 4; k++) {
		for (int b = 0; b < 8; b++) c = (c >> 1) ^ ((c & 1) ? POLY : 0);
		T[k * 256 + i] = c;
	}
}
NXZ_CK_FN uint32_t crc_dword(const uint32_t *T, uint32_t crc, uint32_t w)
{
	const uint32_t c = crc ^ w;
	return T[768 + (c & 0xff)] ^ T[512 + ((c >> 8) & 0xff)] ^ T[256 + ((c >> 16) & 0xff)] ^ T[c >> 24];
}
NXZ_CK_FN uint32_t crc_byte(const uint32_t *T, uint32_t crc, uint32_t b) { return T[(crc ^ b) & 0xff] ^ (crc >> 8); }

// the stream's shape
struct Shape {
	uint32_t n, K1, r;                        // bytes; the tail slice; its bytes (n == 0: no slice at all)
};
NXZ_CK_FN Shape shape_of(uint32_t n)
{
	Shape s;
	s.n = n; s.K1 = n ? (n - 1) >> 6 : 0; s.r = n - s.K1 * SLICE;
	return s;
}

// A lane's share, ready for the sums over lanes: the weighted CRCs of its full slices XORed, the tail's CRC (lane
// K1 / 4 has it, 0 elsewhere), s1 a plain sum (<= 5 x 64 x 255 a lane), s2 a sum of at most five terms below 65521.
struct Part { uint32_t crc, tailcrc, s1, s2; };

typedef uint32_t ck_v4u __attribute__((vector_size(16)));

NXZ_CK_FN void adler_dword(uint32_t w, uint32_t k, uint32_t &S, uint32_t &Wt)      // dword k of its slice
{
	S = NXZ_CK_UDOT4(w, 0x01010101u, S);
	Wt = NXZ_CK_UDOT4(w, 0x03020100u + 0x04040404u * k, Wt);
}

// Lane `lane` of LANES: the full slices 4 lane .. 4 lane + 3 (those below K1), two at a time -- two independent CRC states
// advance side by side, and the 128 bytes of a pair are one cache line that this lane alone asks for, in one burst of
// loads -- and the tail slice if it is this lane's.
// src: the first byte of the stream (16-byte loads at any alignment); nothing at or behind src + n is read.
NXZ_CK_FN Part lane_part(const uint8_t *src_, const Shape sh, uint32_t initx, uint32_t lane, const uint32_t *T)
{
	const NXZ_CK_GLOBAL uint8_t *src = (const NXZ_CK_GLOBAL uint8_t *)src_;
	Part p = { 0, 0, 0, 0 };
	if (!sh.n) return p;
#pragma unroll
	for (uint32_t pr = 0; pr < PER_LANE / 2; pr++) {
		const uint32_t j0 = PER_LANE * lane + 2 * pr;
		if (j0 >= sh.K1) break;
		const bool have1 = j0 + 1 < sh.K1;
		ck_v4u v[2][SLICE / 16];
#pragma unroll
		for (uint32_t q = 0; q < SLICE / 16; q++) {
			__builtin_memcpy(&v[0][q], src + (size_t)j0 * SLICE + 16 * q, 16);
			v[1][q] = (ck_v4u){ 0, 0, 0, 0 };
			if (have1) __builtin_memcpy(&v[1][q], src + (size_t)(j0 + 1) * SLICE + 16 * q, 16);
		}
		uint32_t c0 = j0 == 0 ? initx : 0, c1 = 0, S0 = 0, S1 = 0, W0 = 0, W1 = 0;   // (slice 0 as the tail: below)
#pragma unroll
		for (uint32_t k = 0; k < SLICE / 4; k++) {
			const uint32_t w0 = v[0][k >> 2][k & 3], w1 = v[1][k >> 2][k & 3];
			adler_dword(w0, k, S0, W0);
			adler_dword(w1, k, S1, W1);
			c0 = crc_dword(T, c0, w0);
			c1 = crc_dword(T, c1, w1);          // (no second slice: zeros leave the zero state alone)
		}
		// K1 - 1 - j more full slices follow slice j: 0..1022
		p.crc ^= gf_mul(c0, CRC_POW.v[sh.K1 - 1 - j0]);
		p.s1 += S0;
		p.s2 += (S0 * (sh.n - j0 * SLICE) - W0) % ADLER_MOD;
		if (have1) {
			p.crc ^= gf_mul(c1, CRC_POW.v[sh.K1 - 2 - j0]);
			p.s1 += S1;
			p.s2 += (S1 * (sh.n - (j0 + 1) * SLICE) - W1) % ADLER_MOD;
		}
	}
	if (sh.K1 / PER_LANE == lane) {
		// the tail: r = 1..64 bytes, whole dwords first, then the last 1..3 bytes one by one
		const uint32_t a = sh.K1 * SLICE;
		uint32_t c = sh.K1 == 0 ? initx : 0, St = 0, Wtt = 0;
		const uint32_t nd = sh.r >> 2;
		for (uint32_t k = 0; k < nd; k++) {
			uint32_t w;
			__builtin_memcpy(&w, src + a + 4 * k, 4);
			adler_dword(w, k, St, Wtt);
			c = crc_dword(T, c, w);
		}
		for (uint32_t k = 4 * nd; k < sh.r; k++) {
			const uint32_t b = src[a + k];
			St += b; Wtt += b * k;
			c = crc_byte(T, c, b);
		}
		p.tailcrc = c;
		p.s1 += St;
		p.s2 += (St * sh.r - Wtt) % ADLER_MOD;
	}
	return p;
}

// The workgroup's sums -- crc and tailcrc XORed, s1 and s2 added: at most 1024 slices, so s1 <= 2^24 and s2 < 2^26, no
// reduction on the way -- and the seeds make the two checksums.  n == 0: the seeds come back.
NXZ_CK_FN void finish(const Shape sh, uint32_t in_crc, uint32_t in_adler, uint32_t crc, uint32_t tailcrc, uint32_t s1, uint32_t s2,
		      uint32_t &out_crc, uint32_t &out_adler)
{
	const uint32_t initx = in_crc ^ 0xffffffffu;
	const uint32_t c = sh.n ? gf_mul(crc, CRC_POW8.v[sh.r]) ^ tailcrc : initx;
	const uint32_t ia = in_adler & 0xffff, ib = in_adler >> 16;
	const uint32_t s1f = (ia + s1) % ADLER_MOD;
	const uint32_t s2f = (uint32_t)(((uint64_t)ib + (uint64_t)sh.n * ia + s2) % ADLER_MOD);
	out_crc = c ^ 0xffffffffu;
	out_adler = (s2f << 16) | s1f;
}

} // namespace nxzck
#endif
