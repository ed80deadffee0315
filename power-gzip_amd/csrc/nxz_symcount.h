// nxz_symcount.h -- the LZ symbol counts of a block (286 literal / length + 30 distance symbols: the COUNT function codes'
// out_lzcount and the input of the table generator) from what the LZ77 kernel leaves in the token scratch: the two position
// bitmaps and the match records (nxz_device.h, NXZ_TOK_*).  The arithmetic of nxzsc::count_kernel (nxz_symcount.hip) as plain
// functions over a lane's share: __device__ code under hipcc, host C++ otherwise, so that the CPU test
// (tests/test_symcount_host.py) runs exactly this "as 256 lanes would".
//
// A block of n positions is walked in rounds of RPOS = 2048, 8 consecutive positions a lane (the entropy kernel's geometry):
// the lane at p0 takes the 8 source bytes from p0 and byte p0 / 8 of the literal bitmap, and adds one count per set bit.
// A match adds one length symbol and one distance symbol; the histogram does not depend on the order of the parse, so the
// records are taken as they lie, and there are as many as the match bitmap has bits in [0, n).  What lies behind position n
// -- the rest of the last bitmap word, the words after it, the bytes after the source -- is not the block's: masked, or not read.
#ifndef NXZ_SYMCOUNT_H
#define NXZ_SYMCOUNT_H
#include <stdint.h>
#ifdef __HIPCC__
#define NXZ_SC_FN __device__ __forceinline__
#define NXZ_SC_GLOBAL __attribute__((address_space(1)))        // job buffers are device memory: global_load, not flat_load
#else
#define NXZ_SC_FN inline
#define NXZ_SC_GLOBAL
#endif

namespace nxzsc {

constexpr uint32_t NSYM = 316;               // counts of a job: literals 0..255, [256] = 1 (EOB), lengths, distances
constexpr uint32_t EOB = 256, LEN0 = 257, DIST0 = 286;
constexpr uint32_t LANES = 256;              // lanes that share a block
constexpr uint32_t RPOS = 2048;              // positions per round: 8 per lane
constexpr uint32_t BLOCK_MAX = 65536;        // positions the bitmaps have room for

// length - 3 (0..255) -> length symbol - 257 (0..28)
NXZ_SC_FN uint32_t length_symbol(uint32_t l3)
{
	const uint32_t le = l3 < 8 ? 0 : (29 - (uint32_t)__builtin_clz(l3 | 8));
	return l3 == 255 ? 28 : (le << 2) + (l3 >> le);
}
// distance - 1 (0..32767) -> distance symbol (0..29)
NXZ_SC_FN uint32_t distance_symbol(uint32_t d)
{
	const uint32_t de = d < 4 ? 0 : (30 - (uint32_t)__builtin_clz(d | 4));
	return d < 4 ? d : 2 * de + 2 + ((d >> de) & 1);
}
// a match record (length - 3 | (distance - 1) << 8) -> its two places among the counts
NXZ_SC_FN void record_symbols(uint32_t r, uint32_t &ls, uint32_t &ds)
{
	ls = LEN0 + length_symbol(r & 0xff);
	ds = DIST0 + distance_symbol((r >> 8) & 0x7fff);
}

// the bits of bitmap word w that are positions of the block
NXZ_SC_FN uint32_t word_mask(uint32_t w, uint32_t n)
{
	const uint32_t first = w << 5;
	return first >= n ? 0u : n - first >= 32 ? 0xffffffffu : (1u << (n - first)) - 1;
}
// ... and of the 8 positions from p0 (a bitmap byte)
NXZ_SC_FN uint32_t byte_mask(uint32_t p0, uint32_t n)
{
	return p0 >= n ? 0u : n - p0 >= 8 ? 0xffu : (1u << (n - p0)) - 1;
}

// The 8 source bytes from p0, first byte lowest; the ragged end byte-wise: nothing is read past src + n.
NXZ_SC_FN uint64_t lane_bytes(const uint8_t NXZ_SC_GLOBAL *src, uint32_t p0, uint32_t n)
{
	uint64_t v = 0;
	if (p0 + 8 <= n) {
#ifdef __HIPCC__
		typedef uint32_t v2u __attribute__((ext_vector_type(2)));
		const v2u b = *(const v2u NXZ_SC_GLOBAL *)(src + p0);
		v = (uint64_t)b.x | ((uint64_t)b.y << 32);
#else
		for (uint32_t i = 0; i < 8; i++) v |= (uint64_t)src[p0 + i] << (8 * i);
#endif
	} else {
		for (uint32_t i = 0; i < 8; i++) if (p0 + i < n) v |= (uint64_t)src[p0 + i] << (8 * i);
	}
	return v;
}

// A lane's 8 positions from p0: one add(symbol) per literal that starts there.  litw: the word of the literal bitmap that
// holds them (word p0 / 32).
template <class Add>
NXZ_SC_FN void lane_literals(uint64_t bytes, uint32_t litw, uint32_t p0, uint32_t n, Add add)
{
	const uint32_t lo = (uint32_t)bytes, hi = (uint32_t)(bytes >> 32);
	for (uint32_t lb = (litw >> (p0 & 24)) & byte_mask(p0, n); lb; lb &= lb - 1) {
		const uint32_t k = (uint32_t)__builtin_ctz(lb);
		add((((k & 4) ? hi : lo) >> (8 * (k & 3))) & 0xff);
	}
}

} // namespace nxzsc
#endif
