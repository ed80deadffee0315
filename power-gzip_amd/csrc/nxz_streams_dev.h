// nxz_streams_dev.h -- the steps that the kernels of nxz_batch_deflate_streams (nxz_streams.hip) and of its dictionary form
// (nxz_streams_dict.hip) and of its form for streams written in parts (nxz_streams_part.hip) take, one copy of each: whose block a
// block is, its compress job, how a stream begins and how it ends, where a chunk's blocks go in their stream.
#ifndef NXZ_STREAMS_DEV_H
#define NXZ_STREAMS_DEV_H
#include <hip/hip_runtime.h>
#include "nxz_device.h"
#include "nxz_streams.h"
#include "nxz_pack_block.h"

namespace nxzst {

// the stream that block g of the batch belongs to: the i with first[i] <= g < first[i + 1] (streams without blocks are passed over)
__device__ inline uint32_t owner_of(const uint32_t *__restrict__ first, uint32_t n, uint32_t g)
{
	uint32_t lo = 0, hi = n - 1;
	while (lo < hi) {
		const uint32_t mid = lo + (hi - lo) / 2;
		if (first[mid + 1] > g) hi = mid; else lo = mid + 1;
	}
	return lo;
}

// the compress job of block k of buffer d with hk bytes of window in front of it; its output goes to `slot`
__device__ inline nxz_batch_job_t block_job(const nxz_stream_job_t &d, uint64_t k, uint32_t B, uint32_t hk, uint8_t *slot)
{
	nxz_batch_job_t j;
	j.src = d.src + nxz_streams_block_start(k, B) - hk;
	j.dst = slot;
	j.src_len = hk + nxz_streams_block_len(d.src_len, k, B);
	j.hist_len = hk;
	j.dst_cap = NXZ_STREAMS_SLOT;
	j.in_crc = 0; j.in_adler = 1;
	j.dht_index = 0; j.resume = 0; j.reserved = 0;
	return j;
}

// a stream's state in front of its first block: refused with cc, or its hl header bytes written
__device__ inline nxz_stream_state_t begin_stream(const nxz_stream_job_t &j, uint32_t cc, const uint8_t *h, uint32_t hl)
{
	nxz_stream_state_t st;
	st.cc = cc;
	st.written = 0; st.len_done = 0; st.crc = 0; st.adler = 1; st.stored = 0;
	if (!st.cc) {
		for (uint32_t k = 0; k < hl; k++) j.dst[k] = h[k];
		st.written = hl;
	}
	return st;
}

// behind the last block of a call: the result (bound: what a refused stream is told) and, where the stream ends here (last), the body
// of an empty source and the trailer over total_len source bytes -- all the stream's, of which j.src_len are this call's
__device__ inline nxz_stream_result_t finish_stream_at(const nxz_stream_job_t &j, const nxz_stream_state_t &st, uint32_t blocks, uint64_t bound, int fmt,
						       const bool last, uint64_t total_len)
{
	nxz_stream_result_t r;
	r.cc = st.cc; r.blocks = 0; r.out_len = 0; r.crc = 0; r.adler = 0; r.stored = 0; r.reserved = 0;
	if (st.cc) {
		if (st.cc == NXZ_CC_TARGET_SPACE) r.out_len = bound;
		return r;
	}
	uint64_t at = st.written;
	if (last && !j.src_len) {
		uint8_t e[NXZ_STREAMS_EMPTY_LEN];
		nxz_streams_empty(e);
		for (uint32_t k = 0; k < NXZ_STREAMS_EMPTY_LEN; k++) j.dst[at + k] = e[k];
		at += NXZ_STREAMS_EMPTY_LEN;
	}
	uint8_t tr[8];
	const uint32_t tl = last ? nxz_streams_trailer(fmt, st.crc, st.adler, total_len, tr) : 0;
	for (uint32_t k = 0; k < tl; k++) j.dst[at + k] = tr[k];
	r.blocks = blocks;
	r.out_len = at + tl;
	r.crc = st.crc; r.adler = st.adler; r.stored = st.stored;
	return r;
}

// ... of a stream that is written in one call
__device__ inline nxz_stream_result_t finish_stream(const nxz_stream_job_t &j, const nxz_stream_state_t &st, uint32_t blocks, uint64_t bound, int fmt)
{
	return finish_stream_at(j, st, blocks, bound, fmt, true, j.src_len);
}

__device__ inline uint32_t wave_xor(uint32_t v)
{
	for (int d = 32; d; d >>= 1) v ^= __shfl_xor(v, d);
	return v;
}
__device__ inline uint64_t wave_sum(uint64_t v)
{
	for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d);
	return v;
}

// Where the blocks of stream i inside the chunk [b0, b0 + m) go and what they add to its checksums, by one wavefront, 64 blocks at a
// time, a lane each.  last: the stream's last block is the final one (BFINAL, nothing behind it); else it ends the bytes written so
// far on a byte boundary like every other block (nxz_batch_deflate_streams_part without NXZ_PART_LAST).
// Sizes and the Adler sums are prefix sums over the lanes.  The CRC needs no scan: every block but a stream's last has B bytes, so
// a lane knows how many bytes lie behind its block in this part and moves its block's CRC over them itself (op_block = the operator
// of B bytes, made once by the host; powers of it by square-and-multiply); the moved CRCs are XORed together.
__device__ inline void layout_stream(const uint32_t *__restrict__ first, uint32_t i, uint32_t b0, uint32_t m,
				     const nxz_batch_job_t *__restrict__ jobs, const nxz_batch_result_t *__restrict__ results,
				     uint32_t B, uint32_t op_block, nxz_stream_state_t *__restrict__ state, uint64_t *__restrict__ offsets, const bool last)
{
	const uint32_t lane = threadIdx.x;
	const uint32_t f0 = first[i], f1 = first[i + 1];
	const uint32_t lo = f0 > b0 ? f0 : b0, hi = f1 < b0 + m ? f1 : b0 + m;
	if (lo >= hi) return;
	const uint32_t fin = last ? f1 - 1 : 0xffffffffu;                     // the final block (no block of a batch has this index: none)
	const nxz_stream_state_t st = state[i];
	const uint32_t M = NXZ_ADLER_BASE;
	// the part's last block: the only one that may be short
	const uint32_t last_len = jobs[hi - 1 - b0].src_len - jobs[hi - 1 - b0].hist_len;
	const uint32_t tail = last_len == B ? 0 : last_len, last_full = last_len == B ? 1 : 0;
	uint64_t base = st.written, adler_b = 0;
	uint32_t base_da = ((st.adler & 0xffff) + M - 1) % M;                 // (Adler's low sum so far) - 1
	uint32_t crc_part = 0, stored = 0;
	for (uint32_t i0 = lo; i0 < hi; i0 += 64) {
		const uint32_t g = i0 + lane;
		const bool valid = g < hi;
		uint32_t size = 0, da = 0, len = 0, crc = 0, bsum = 0;
		bool is_stored = false;
		if (valid) {
			const nxz_batch_job_t job = jobs[g - b0];
			const nxz_batch_result_t r = results[g - b0];
			const nxz::StreamPiece p = nxz::stream_piece(job, r, g == fin);
			size = p.size; len = p.len; is_stored = p.stored;
			crc = r.crc; da = ((r.adler & 0xffff) + M - 1) % M; bsum = r.adler >> 16;
		}
		uint32_t incl = size, incl_da = da;                               // (64 pieces of 64 KiB and a few bytes: 32 bits hold their sum)
		for (uint32_t d = 1; d < 64; d <<= 1) {
			const uint32_t v = __shfl_up(incl, d);
			const uint32_t w = __shfl_up(incl_da, d);
			if (lane >= d) { incl += v; incl_da += w; }
		}
		if (valid) {
			offsets[g - b0] = base + incl - size;
			// the bytes behind this block in the part: hi - 1 - g blocks, all of B bytes but perhaps the last
			const uint32_t behind = hi - 1 - g;
			const uint32_t op = behind ? nxz_crc_blocks_op(op_block, (uint64_t)behind - 1 + last_full, tail) : 0x80000000u;
			crc_part ^= nxz_gf2_mul32(crc, op);
			const uint32_t P = (base_da + incl_da - da) % M;              // (the low sum in front of this block) - 1
			adler_b += (bsum + (uint64_t)(len % M) * P) % M;
		}
		base += __shfl(incl, 63);
		base_da = (base_da + __shfl(incl_da, 63)) % M;
		stored += (uint32_t)__popcll(__ballot(valid && is_stored));
	}
	crc_part = wave_xor(crc_part);
	adler_b = wave_sum(adler_b);
	if (lane == 0) {
		const uint32_t cnt = hi - lo;
		const uint64_t bytes = (uint64_t)(cnt - 1) * B + last_len;
		nxz_stream_state_t o = st;
		o.written = base;
		o.len_done = st.len_done + bytes;
		o.crc = nxz_crc_join(st.crc, crc_part, nxz_crc_blocks_op(op_block, (uint64_t)cnt - 1 + last_full, tail));
		o.adler = (uint32_t)(((st.adler >> 16) + adler_b) % M) << 16 | (base_da + 1) % M;
		o.stored = st.stored + stored;
		state[i] = o;
	}
}

} // namespace nxzst
#endif
