// nxz_pack_block.h -- one block of a deflate stream that is strung together from independently compressed blocks: what it occupies
// in the stream (stream_piece) and the workgroup that writes it (pack_block).  Shared by the kernels of nxz_misc.hip (one stream from a
// batch, several callers' streams: nxz_deflate_host) and of nxz_streams.hip (a stream per device buffer: nxz_batch_deflate_streams).
#ifndef NXZ_PACK_BLOCK_H
#define NXZ_PACK_BLOCK_H
#include <hip/hip_runtime.h>
#include "nxz_device.h"

namespace nxz {

struct StreamPiece {
	bool stored;
	uint32_t len;       // source bytes
	uint32_t keep;      // compressed: bytes taken from the job's output
	uint32_t size;      // bytes this block occupies in the stream
	uint32_t pad;       // compressed: zero bytes between the output and 00 00 FF FF (the 3 header bits of the empty block may spill)
	bool marker;
};

__device__ inline StreamPiece stream_piece(const nxz_batch_job_t &job, const nxz_batch_result_t &r, bool final)
{
	StreamPiece p;
	p.len = job.src_len - job.hist_len;
	p.stored = r.cc != 0 || r.tpbc > p.len;
	if (p.stored) {
		p.keep = 0; p.pad = 0; p.marker = false;
		p.size = p.len > 65535 ? p.len + 10 : p.len + 5;
	} else {
		p.keep = r.tpbc;
		p.marker = !final && r.tebc != 0;
		p.pad = p.marker && r.tebc + 3 > 8 ? 1 : 0;
		p.size = r.tpbc + (p.marker ? p.pad + 4 : 0);
	}
	return p;
}

// one block of the stream, by one workgroup of 256: `o` is where it goes
__device__ inline void pack_block(const nxz_batch_job_t &job, const nxz_batch_result_t &r, const bool final, uint8_t *__restrict__ o)
{
	const uint32_t t = threadIdx.x;
	const StreamPiece p = stream_piece(job, r, final);
	const uint8_t *data = p.stored ? job.src + job.hist_len : job.dst;
	// stored: [hdr 5][first][hdr 5][rest]; compressed: [keep][pad][00 00 FF FF]
	const uint32_t first = p.len > 65535 ? 65535 : p.len, rest = p.len - first;
	const uint32_t d0 = p.stored ? 5 : 0;                           // first stream byte that is a plain copy of `data`
	const uint32_t dn = p.stored ? first : p.keep;
	const uint32_t lastmask = r.tebc ? (1u << r.tebc) - 1 : 0xff;
	auto byte_at = [&](uint32_t j) -> uint32_t {
		if (p.stored) {
			auto hdr = [&](uint32_t k, uint32_t n, bool last) -> uint32_t {
				return k == 0 ? (last ? 1u : 0u) : k < 3 ? (n >> (8 * (k - 1))) & 0xff : (~n >> (8 * (k - 3))) & 0xff;
			};
			if (j < 5) return hdr(j, first, final && rest == 0);
			if (j < 5 + first) return data[j - 5];
			if (j < 10 + first) return hdr(j - 5 - first, rest, final);
			return data[j - 10];
		}
		if (j < p.keep) {
			uint32_t v = data[j];
			if (j == 0) v = (v & ~1u) | (final ? 1u : 0u);          // set_bfinal (lib/nx_deflate.c:1404-1413)
			if (j == p.keep - 1) v &= lastmask;
			return v;
		}
		const uint32_t k = j - p.keep - p.pad;                      // after the pad byte: LEN = 0, NLEN = ffff
		return j < p.keep + p.pad ? 0 : k < 2 ? 0 : 0xff;
	};
	const uint32_t size = p.size;
	const uint32_t head = (uint32_t)((4 - ((uintptr_t)o & 3)) & 3);
	const uint32_t nd = size > head ? (size - head) >> 2 : 0;
	if (t < head && t < size) o[t] = (uint8_t)byte_at(t);
	for (uint32_t k = head + nd * 4 + t; k < size; k += 256) o[k] = (uint8_t)byte_at(k);
	uint32_t *od = (uint32_t *)(o + head);
	for (uint32_t w = t; w < nd; w += 256) {
		const uint32_t j = head + w * 4;
		uint32_t v;
		// whole dwords strictly inside the copied region (not its first or last byte, which are patched)
		if (j > d0 && j + 4 < d0 + dn) {
			const uintptr_t a = (uintptr_t)data + (j - d0);
			const uint32_t *q = (const uint32_t *)(a & ~(uintptr_t)3);
			const uint32_t bo = (uint32_t)a & 3;
			const uint32_t lo = q[0], hi = bo ? q[1] : 0;
			v = __builtin_amdgcn_alignbyte(hi, lo, bo);
		} else {
			v = byte_at(j) | byte_at(j + 1) << 8 | byte_at(j + 2) << 16 | byte_at(j + 3) << 24;
		}
		od[w] = v;
	}
}

} // namespace nxz
#endif
