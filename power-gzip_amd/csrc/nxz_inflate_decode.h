// nxz_inflate_decode.h -- what the kernels that walk a deflate stream a wavefront each share: the bit reader over the
// source, the construction of the decode tables (nxz_inflate_tables.h), the header of a dynamic block and the look-up of one
// symbol.  Used by nxz_inflate.hip (the decoder) and nxz_inflate_size.hip (the walk that only counts the output).
// Everything here is written for a workgroup of ONE wavefront: __syncthreads() orders that wavefront's LDS traffic.
#ifndef NXZ_INFLATE_DECODE_H
#define NXZ_INFLATE_DECODE_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "nxz_device.h"
#include "nxz_inflate_tables.h"

namespace nxzi {


// a value that is the same in all lanes but sits in a vector register: tell the compiler
__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

constexpr uint32_t STAGE = 512;              // staged compressed bytes (one-token path and headers only)
// (LBITS, DBITS, Huff, HuffD: nxz_inflate_tables.h)

// Build the decode tables for `n` symbols with code lengths len[] (wave cooperative).
// All of it by the whole wave: symbol i = row * 64 + lane; counts per length, first codes and the rank
// of a symbol among those of its length come out of ballots (RFC 1951 3.2.2), every symbol then writes
// its slots of the fast table and its place in the (length, symbol) order of the slow path.
template <int FB, typename H>
__device__ __forceinline__ void build(H &h, const uint8_t *len, int n, int lane)
{
	constexpr int ROWS = 5;                                          // n <= 288 + 32
	const uint64_t below = (1ull << lane) - 1;
	uint32_t l[ROWS], code[ROWS], place[ROWS];
#pragma unroll
	for (int r = 0; r < ROWS; r++) { const int i = r * 64 + lane; l[r] = i < n ? len[i] : 0; code[r] = 0; place[r] = 0; }
	for (int i = lane; i < (1 << FB); i += 64) h.fast[i] = 0;
	uint32_t c = 0, prevcnt = 0, offs = 0;
	for (uint32_t b = 1; b <= 15; b++) {
		c = (c + prevcnt) << 1;
		uint32_t run = 0;
#pragma unroll
		for (int r = 0; r < ROWS; r++) {
			const uint64_t m = __ballot(l[r] == b);
			const uint32_t k = run + (uint32_t)__popcll(m & below);
			if (l[r] == b) { code[r] = c + k; place[r] = offs + k; }
			run += (uint32_t)__popcll(m);
		}
		if (lane == 0) h.count[b] = (uint16_t)run;
		prevcnt = run; offs += run;
	}
	if (lane == 0) h.count[0] = 0;
	__syncthreads();
#pragma unroll
	for (int r = 0; r < ROWS; r++) {
		const uint32_t i = r * 64 + lane;
		if (!l[r]) continue;
		h.sym[place[r]] = (uint16_t)i;
		if (l[r] > (uint32_t)FB) continue;
		const uint32_t rev = __builtin_bitreverse32(code[r]) >> (32 - l[r]);
		for (uint32_t idx = rev; idx < (1u << FB); idx += (1u << l[r])) h.fast[idx] = (uint16_t)(i | (l[r] << 12));
	}
	__syncthreads();
}

struct Bits {
	const NXZ_GLOBAL_AS uint8_t *src;   // device memory, used through address space 1 (a generic access makes the compiler drain the LDS queue at every later wait)
	uint32_t srclen;
	uint64_t total_bits;      // 8*srclen
	uint64_t pos;             // next unread bit
	uint32_t stage_base;      // byte offset of stage[0] in src (multiple of 16), 0xffffffff = none
	uint32_t *stage;
	int lane;

	__device__ __forceinline__ void restage(uint32_t byte)
	{
		// all lanes: load STAGE bytes starting at byte & ~15
		uint32_t base = byte & ~15u;
		__syncthreads();
		for (uint32_t i = lane; i < STAGE / 16; i += 64) {
			uint32_t off = base + i * 16;
			uint4 v = make_uint4(0, 0, 0, 0);
			if (off + 16 <= srclen) v = *(const uint4 *)(src + off);
			else if (off < srclen) {
				uint32_t w[4] = {0, 0, 0, 0};
				for (uint32_t k = 0; off + k < srclen; k++) w[k >> 2] |= (uint32_t)src[off + k] << (8 * (k & 3));
				v = make_uint4(w[0], w[1], w[2], w[3]);
			}
			((uint4 *)stage)[i] = v;
		}
		stage_base = base;
		__syncthreads();
	}
	// make sure [byte, byte+span) is staged (wave-uniform call)
	__device__ __forceinline__ void ensure(uint32_t byte, uint32_t span)
	{
		if (stage_base == 0xffffffffu || byte < stage_base || byte + span > stage_base + STAGE) restage(byte);
	}
	// peek up to 32 bits at the current position (bits past the end read as 0)
	__device__ __forceinline__ uint32_t peek()
	{
		ensure((uint32_t)(pos >> 3), 8);
		return raw_peek();
	}
	__device__ __forceinline__ uint32_t raw_peek() const
	{
		uint32_t byte = (uint32_t)(pos >> 3);
		uint32_t o = byte - stage_base;
		uint32_t a = stage[o >> 2], b = stage[(o >> 2) + 1], c = stage[(o >> 2) + 2];
		uint32_t lo = __builtin_amdgcn_alignbyte(b, a, o & 3);
		uint32_t hi = __builtin_amdgcn_alignbyte(c, b, o & 3);
		uint32_t sh = (uint32_t)pos & 7;
		return (uint32_t)((((uint64_t)hi << 32) | lo) >> sh);
	}
	__device__ __forceinline__ bool have(uint32_t n) const { return pos + n <= total_bits; }

	// ---- register bit buffer for the symbol loop: `bb` holds bits [pos, pos+bc) ----
	uint64_t bb = 0; uint32_t bc = 0;
	__device__ __forceinline__ void bb_sync() { bb = 0; bc = 0; }            // after pos was changed by hand
	__device__ __forceinline__ void bb_fill()                                 // make bc >= 32
	{
		if (bc >= 32) return;
		uint64_t p2 = pos + bc;                                               // first bit not in bb
		uint32_t byte = (uint32_t)(p2 >> 3);
		ensure(byte, 12);
		uint32_t o = byte - stage_base;
		uint32_t a = stage[o >> 2], b = stage[(o >> 2) + 1];
		uint32_t v = __builtin_amdgcn_alignbyte(b, a, o & 3);
		uint32_t sh = (uint32_t)p2 & 7;                                       // bits of that byte already consumed/held
		// take the (32 - sh) fresh bits of v
		bb |= (uint64_t)(v >> sh) << bc;
		bc += 32 - sh;
	}
	__device__ __forceinline__ void bb_drop(uint32_t n) { bb >>= n; bc -= n; pos += n; }
};

// RFC1951 3.2.5 length / distance code parameters, computed
__device__ __forceinline__ void len_params(uint32_t s, uint32_t &base, uint32_t &extra)
{
	extra = s < 8 || s == 28 ? 0 : (s - 4) >> 2;
	base = s < 8 ? 3 + s : s == 28 ? 258 : ((4 + (s & 3)) << extra) + 3;
}
__device__ __forceinline__ void dist_params(uint32_t d, uint32_t &base, uint32_t &extra)
{
	extra = d < 4 ? 0 : (d - 2) >> 1;
	base = d < 4 ? d + 1 : ((2 + (d & 1)) << extra) + 1;
}

template <int FB, typename H>
__device__ __forceinline__ int decode_sym(const H &h, uint32_t bits, uint32_t &nbits)
{
	uint32_t e = h.fast[bits & ((1u << FB) - 1)];
	if (e) { nbits = e >> 12; return (int)(e & 0xfff); }
	// slow canonical walk (codes longer than FB bits)
	int code = 0, first = 0, index = 0;
	for (int len = 1; len <= 15; len++) {
		code |= (int)(bits & 1); bits >>= 1;
		int count = h.count[len];
		if (code - count < first) { nbits = len; return h.sym[index + (code - first)]; }
		index += count; first += count; first <<= 1; code <<= 1;
	}
	nbits = 16;
	return -2;
}

// Parse a dynamic block header at b.pos (after the 3 header bits).  Returns
// 0 ok (lens filled, b.pos advanced, *tbits = table bits), 1 out of source, <0 invalid.
// The header (at most 2283 bits) is taken into two registers per lane (lane k: dwords k and 64 + k
// from the dword the header starts in; a copy in sm.stage for the one step where lanes read at
// different places), so the serial part -- one code-length symbol after the other -- reads its bits
// with v_readlane and looks the 7-bit code-length code up in two more registers: no LDS round trip
// per symbol.  The code-length code's canonical codes come from ballots (lane = symbol).
template <typename Smem>
__device__ __forceinline__ int read_dht(Bits &b, Smem &sm, int &hlit, int &hdist, uint32_t &tbits)
{
	const int lane = b.lane;
	const uint64_t start = b.pos;
	if (!b.have(14)) return 1;
	const uint32_t d0 = (uint32_t)(start >> 5);                       // first dword of the header
	auto dword = [&](uint32_t idx) __attribute__((always_inline)) -> uint32_t {
		const uint64_t byte = (uint64_t)idx * 4;
		uint32_t w = 0;
		if (byte + 4 <= b.srclen && ((uintptr_t)b.src & 3) == 0) w = ((const NXZ_GLOBAL_AS uint32_t *)b.src)[idx];
		else for (uint32_t k = 0; k < 4 && byte + k < b.srclen; k++) w |= (uint32_t)b.src[byte + k] << (8 * k);
		return w;
	};
	const uint32_t R0 = dword(d0 + lane), R1 = dword(d0 + 64 + lane);
	__syncthreads();
	sm.stage[lane] = R0; sm.stage[64 + lane] = R1;
	b.stage_base = 0xffffffffu;                                       // (the stage no longer holds what Bits put there)
	__syncthreads();
	// up to 25 bits at bit p of the source (p >= start), wave-uniform
	auto peek = [&](uint64_t p) __attribute__((always_inline)) -> uint32_t {
		const uint32_t o = uni((uint32_t)(p - (uint64_t)d0 * 32)), i = o >> 5, sh = o & 31;
		const uint32_t lo = i < 64 ? (uint32_t)__builtin_amdgcn_readlane((int)R0, (int)i) : (uint32_t)__builtin_amdgcn_readlane((int)R1, (int)(i - 64));
		const uint32_t j = i + 1;
		const uint32_t hi = j < 64 ? (uint32_t)__builtin_amdgcn_readlane((int)R0, (int)j) : (uint32_t)__builtin_amdgcn_readlane((int)R1, (int)(j & 63));
		return (uint32_t)(((((uint64_t)hi << 32) | lo) >> sh));
	};
	uint32_t v = peek(start);
	hlit = (int)(v & 31) + 257; hdist = (int)((v >> 5) & 31) + 1;
	const int hclen = (int)((v >> 10) & 15) + 4;
	uint64_t pos = start + 14;
	if (hlit > 286 || hdist > 30) return -1;
	if (pos + 3 * (uint32_t)hclen > b.total_bits) return 1;
	// the code-length code: lane i < hclen reads the i-th 3-bit length, which belongs to symbol order[i]
	uint32_t myl = 0;
	{
		const uint8_t order[19] = { 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 };
		if (lane < 32) sm.cl[lane] = 0;
		__syncthreads();
		if (lane < hclen) {
			const uint32_t o = (uint32_t)(pos - (uint64_t)d0 * 32) + 3 * (uint32_t)lane;
			const uint64_t w = (uint64_t)sm.stage[o >> 5] | ((uint64_t)sm.stage[(o >> 5) + 1] << 32);
			sm.cl[order[lane]] = (uint8_t)((w >> (o & 31)) & 7);
		}
		__syncthreads();
		myl = lane < 19 ? sm.cl[lane] : 0;
	}
	pos += 3 * (uint32_t)hclen;
	// canonical codes by ranks (lane = symbol), then the look-up: entries `lane` and `lane + 64` of the
	// 7-bit table, symbol | length << 5, 0xff = no code
	uint32_t tlo = 0xff, thi = 0xff;
	{
		uint32_t c = 0, prevcnt = 0, kraft = 0, mycode = 0;
		for (uint32_t bl = 1; bl <= 7; bl++) {
			c = (c + prevcnt) << 1;
			const uint64_t m = __ballot(myl == bl);
			if (myl == bl) mycode = c + (uint32_t)__popcll(m & ((1ull << lane) - 1));
			prevcnt = (uint32_t)__popcll(m);
			kraft += prevcnt << (7 - bl);
		}
		if (kraft > 128) return -2;
		const uint32_t myrev = myl ? __builtin_bitreverse32(mycode) >> (32 - myl) : 0;
		for (int sy = 0; sy < 19; sy++) {
			const uint32_t l = (uint32_t)__builtin_amdgcn_readlane((int)myl, sy);
			if (!l) continue;
			const uint32_t rev = (uint32_t)__builtin_amdgcn_readlane((int)myrev, sy), mask = (1u << l) - 1;
			if (((uint32_t)lane & mask) == rev) tlo = (uint32_t)sy | (l << 5);
			if ((((uint32_t)lane + 64) & mask) == rev) thi = (uint32_t)sy | (l << 5);
		}
	}
	int n = 0, prev = 0;
	const int total = hlit + hdist;
	// (the bits at pos in a scalar window, refilled from the lanes' registers every few symbols: a symbol takes 14
	// bits at most -- two trips through v_readlane per symbol would otherwise be the better part of the loop)
	uint64_t win = 0;
	uint32_t wbits = 0;
	auto word = [&](uint32_t i) __attribute__((always_inline)) -> uint32_t {
		const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)R0, (int)(i & 63)), hi = (uint32_t)__builtin_amdgcn_readlane((int)R1, (int)(i & 63));
		return i < 64 ? lo : hi;
	};
	while (n < total) {
		if (pos + 1 > b.total_bits) return 1;
		if (wbits < 14) {
			const uint32_t o = uni((uint32_t)(pos - (uint64_t)d0 * 32)), i = o >> 5, sh = o & 31;
			win = (((uint64_t)word(i + 1) << 32) | word(i)) >> sh;
			wbits = 64 - sh;
		}
		const uint32_t bits = (uint32_t)win;
		const uint32_t k = bits & 127;
		const uint32_t e = k < 64 ? (uint32_t)__builtin_amdgcn_readlane((int)tlo, (int)k) : (uint32_t)__builtin_amdgcn_readlane((int)thi, (int)(k - 64));
		if (e == 0xff) return pos + 7 <= b.total_bits ? -3 : 1;
		const int sym = (int)(e & 31), len = (int)(e >> 5);
		if (pos + (uint32_t)len > b.total_bits) return 1;
		pos += (uint32_t)len;
		win >>= len; wbits -= (uint32_t)len;
		if (sym < 16) { if (lane == 0) sm.lens[n] = (uint8_t)sym; n++; prev = sym; }
		else {
			const int eb = sym == 16 ? 2 : sym == 17 ? 3 : 7;
			if (pos + (uint32_t)eb > b.total_bits) return 1;
			const int rep = (int)((bits >> len) & ((1u << eb) - 1)) + (sym == 18 ? 11 : 3);
			pos += (uint32_t)eb;
			win >>= eb; wbits -= (uint32_t)eb;
			int val = 0;
			if (sym == 16) { if (n == 0) return -4; val = prev; }
			if (n + rep > total) return -5;
			for (int q = lane; q < rep; q += 64) sm.lens[n + q] = (uint8_t)val;
			n += rep;
			if (sym != 16) prev = 0;
		}
	}
	b.pos = pos;
	tbits = (uint32_t)(pos - start);
	__syncthreads();
	if (uni(sm.lens[256]) == 0) return -6;
	// over-subscription check: lane per symbol
	uint32_t k1 = 0, k2 = 0;
	for (int i = lane; i < hlit; i += 64) if (sm.lens[i]) k1 += 1u << (15 - sm.lens[i]);
	if (lane < hdist && sm.lens[hlit + lane]) k2 = 1u << (15 - sm.lens[hlit + lane]);
	for (int o = 32; o > 0; o >>= 1) { k1 += __shfl_xor(k1, o, 64); k2 += __shfl_xor(k2, o, 64); }
	if (uni(k1) > (1u << 15) || uni(k2) > (1u << 15)) return -7;
	return 0;
}

} // namespace nxzi
#endif
