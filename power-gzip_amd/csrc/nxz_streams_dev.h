// nxz_streams_dev.h -- the steps that the kernels of nxz_batch_deflate_streams (nxz_streams.hip) and of its dictionary form
// (nxz_streams_dict.hip) both take, one copy of each: whose block a block is, its compress job, how a stream begins and how it ends.
#ifndef NXZ_STREAMS_DEV_H
#define NXZ_STREAMS_DEV_H
#include <hip/hip_runtime.h>
#include "nxz_device.h"
#include "nxz_streams.h"

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

// behind a stream's last block: the body of an empty stream, the trailer, the result (bound: what a refused stream is told)
__device__ inline nxz_stream_result_t finish_stream(const nxz_stream_job_t &j, const nxz_stream_state_t &st, uint32_t blocks, uint64_t bound, int fmt)
{
	nxz_stream_result_t r;
	r.cc = st.cc; r.blocks = 0; r.out_len = 0; r.crc = 0; r.adler = 0; r.stored = 0; r.reserved = 0;
	if (st.cc) {
		if (st.cc == NXZ_CC_TARGET_SPACE) r.out_len = bound;
		return r;
	}
	uint64_t at = st.written;
	if (!j.src_len) {
		uint8_t e[NXZ_STREAMS_EMPTY_LEN];
		nxz_streams_empty(e);
		for (uint32_t k = 0; k < NXZ_STREAMS_EMPTY_LEN; k++) j.dst[at + k] = e[k];
		at += NXZ_STREAMS_EMPTY_LEN;
	}
	uint8_t tr[8];
	const uint32_t tl = nxz_streams_trailer(fmt, st.crc, st.adler, j.src_len, tr);
	for (uint32_t k = 0; k < tl; k++) j.dst[at + k] = tr[k];
	r.blocks = blocks;
	r.out_len = at + tl;
	r.crc = st.crc; r.adler = st.adler; r.stored = st.stored;
	return r;
}

} // namespace nxzst
#endif
