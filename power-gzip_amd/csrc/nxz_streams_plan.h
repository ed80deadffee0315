// nxz_streams_plan.h -- the host's plans for the calls of nxz_batch_streams.cpp (and the carve for every nxz_batch_*.cpp) as plain code
// without a HIP include: it compiles for the engine's host side and for the host test programs (tests/native/streams_part_host.cpp,
// streams_dict_host.cpp, inflate_part_host.cpp), which run THESE functions against brute force.  No allocation: the arrays are the caller's.
#ifndef NXZ_STREAMS_PLAN_H
#define NXZ_STREAMS_PLAN_H
#include <stddef.h>
#include <stdint.h>
#include "nxz_streams_dict.h"

// ---- the carve: a buffer's arrays one behind the other, each on a 256-byte boundary.  take(bytes) is where the next array starts;
// `end` is where the last one ended (unpadded: a layout's total) ----
struct nxz_carve {
	size_t next = 0, end = 0;
	size_t take(size_t bytes) { const size_t at = next; end = at + bytes; next = (end + 255) & ~(size_t)255; return at; }
};

// ---- the block prefix: stream i has blocks_of(i, &flag) blocks (0: refused, or empty); one with blocks is flagged unless the call
// clears flag -- every such stream for the dictionary form, those whose first block is staged for parts.  first[i]: the blocks in
// front of stream i; second[i] (NULL: not kept): the flagged streams in front of it.  The blocks in all, or -1 once they reach 2^31
// (nothing is queued yet: -E2BIG) ----
template <class F> inline int64_t nxz_plan_prefix(size_t n, uint32_t *first, uint32_t *second, F blocks_of)
{
	uint64_t total = 0;
	uint32_t flagged = 0;
	for (size_t i = 0; i < n; i++) {
		first[i] = (uint32_t)total;
		if (second) second[i] = flagged;
		bool flag = true;
		const uint64_t blocks = blocks_of(i, &flag);
		total += blocks;
		if (total >= (1ull << 31)) return -1;
		if (blocks && flag) flagged++;
	}
	first[n] = (uint32_t)total;
	if (second) second[n] = flagged;
	return (int64_t)total;
}

// ---- the chunk walk: blocks b0 .. b0 + m - 1, stream i_lo owns the first and i_hi the last (both have blocks).  The chunks go in
// order: from {0, 0, 0, 0} each call moves *k to the chunk behind it; false when there is none (C != 0 unless nblk is 0) ----
struct nxz_plan_chunk { uint32_t b0, m, i_lo, i_hi; };
inline bool nxz_plan_next_chunk(const uint32_t *first, uint32_t nblk, uint32_t C, nxz_plan_chunk *k)
{
	const uint32_t b0 = k->b0 + k->m;
	if (b0 >= nblk) return false;
	const uint32_t m = nblk - b0 < C ? nblk - b0 : C;
	uint32_t i_lo = k->i_hi;
	while (first[i_lo + 1] <= b0) i_lo++;
	uint32_t i_hi = i_lo;
	while (first[i_hi + 1] < b0 + m) i_hi++;
	*k = {b0, m, i_lo, i_hi};
	return true;
}

// ---- the chunk counts: the flagged first blocks in front of the chunk, and inside it ----
struct nxz_plan_count { uint32_t before, inside; };
// the dictionary form, nz[]: i_lo's first block lies in front unless it IS b0; i_hi's is not behind the chunk
inline nxz_plan_count nxz_plan_dict_firsts(const uint32_t *first, const uint32_t *nz, const nxz_plan_chunk &k)
{
	const uint32_t before = nxz_streams_dict_firsts_before(nz[k.i_lo], k.b0 - first[k.i_lo]);
	return {before, nxz_streams_dict_firsts_before(nz[k.i_hi], 1) - before};
}
// parts, sg[]: the same two ends, but a stream with blocks need not be flagged (sg[i + 1] counts stream i if it is)
inline nxz_plan_count nxz_plan_part_staged(const uint32_t *first, const uint32_t *sg, const nxz_plan_chunk &k)
{
	const uint32_t before = first[k.i_lo] < k.b0 ? sg[k.i_lo + 1] : sg[k.i_lo];
	return {before, sg[k.i_hi + 1] - before};
}

// ---- the inflate cut: stream i's slot takes at most bound_of(i) bytes (never 0: nxz_inflate_part_slot_bound holds a full tail).  A
// chunk ends in front of the stream that would carry its slots beyond `scratch` bytes (a larger stream is a chunk of its own) or at
// max_streams streams.  off[] (room for 2 n entries): a chunk of m streams has m + 1, the first 0, the last its staging bytes ----
// (max_cnt, max_bytes: the most streams and the most staging bytes a chunk holds)
struct nxz_plan_cut { size_t entries; uint32_t max_cnt; uint64_t max_bytes; };
template <class F> inline nxz_plan_cut nxz_plan_inflate_cut(size_t n, uint64_t scratch, uint32_t max_streams, uint64_t *off, F bound_of)
{
	nxz_plan_cut p = {0, 0, 0};
	uint64_t cur = 0;
	uint32_t cnt = 0;
	for (size_t i = 0; i < n; i++) {
		const uint64_t b = bound_of(i);
		if (cnt && (cur + b > scratch || cnt == max_streams)) { off[p.entries++] = cur; cur = 0; cnt = 0; }
		off[p.entries++] = cur;
		cur += b; cnt++;
		if (cur > p.max_bytes) p.max_bytes = cur;
		if (cnt > p.max_cnt) p.max_cnt = cnt;
	}
	off[p.entries++] = cur;
	return p;
}
// the streams of the chunk whose entries begin at off[e0]: they end in front of the next chunk's 0
inline uint32_t nxz_plan_cut_streams(const uint64_t *off, size_t e0, size_t entries)
{
	uint32_t m = 1;
	while (e0 + m + 1 < entries && off[e0 + m + 1] != 0) m++;
	return m;
}
#endif
