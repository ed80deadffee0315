// nxz_inflate_verify.hip -- are the streams intact?  The kernel behind nxz_batch_decompress_verify / _verify_framed (gfx950, wave64):
// CRC-32 and Adler-32 of what a stream makes, with no target for the decoded bytes.  No bit-walker of its own: it is the size walk
// (nxz_inflate_walk.h) with a hook that receives the bytes of every token, as nxz_checkpoint_build.hip's does, and checksums them.
//
//   verify_kernel    nxzcb::build_kernel's shape -- one job per wavefront, one wavefront per workgroup, the long jobs first.  The
//                    hook applies every token to a ring of 32 KiB in LDS (nxz_ring_wave.h's writers, the ring's rules in
//                    nxz_checkpoint_build.h).  There are no checkpoints: the hook's budget cuts the walk every 16 KiB of output
//                    (nxz_verify.h: PASS), and at every cut the wavefront checksums the whole 64-byte slices that passed through
//                    the ring since the last pass, lanes side by side, four slices a lane with four CRC states in flight
//                    (nxz_verify.h's lane_pass; the weights are nxz_cksum_slices.h's).  The running CRC state and Adler pair live
//                    in scalar registers and seed the next pass.  Behind the walk: one more pass and the last 0..63 bytes.
//                    In front of the walk the ring is preloaded with the job's window -- the hist_len bytes at src, and for a job
//                    of the framed call that names the dictionary the dictionary's inflate window, read from its one device copy
//                    -- so that window byte -k stands at ring position 32768 - k; preloaded bytes are never checksummed.
//                    The record is nxz_size_record's (nxz_size.h) with crc and adler filled in where tpbc is (cc 0 and 3).
//
// LDS: the walk's 6704 bytes, the ring's 32 768 and the slice-by-4 CRC table's 4096 = 43 568: THREE workgroups a CU.  The table is
// kept in LDS: a pass is 256 dependent-in-fours look-ups a lane at addresses that differ from lane to lane, which LDS answers in
// tens of cycles where a table in device memory would answer each from the vector cache in hundreds -- with one wavefront a
// workgroup nothing else hides that latency.  Four workgroups a CU (40 960 bytes, the table outside LDS) was NOT measured.
// Registers are no bound at three wavefronts a CU; the kernel uses no scratch.
// Speed (profiles/r18_verify.txt, MI355X; tools/bench_verify.py): 64 zlib -6 streams of 16 MiB 953 ms, 4096 streams of 1 MiB 366 ms --
// 23.5 and 9.3 times nxz_batch_decompress_framed into full targets (41 ms, 39 ms), which holds 1102 MiB and 4096 MiB of device memory
// where this call holds 10 MiB and 2 MiB.  Over nxz_batch_checkpoint_build with one span (the walk plus the ring, 898 ms and 235 ms)
// the checksum passes add 6 % and 36 % of the verify's time; on 4096 streams part of that is the fourth workgroup a CU that the
// table's LDS costs.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "nxz_device.h"
#include "nxz_inflate_walk.h"
#include "nxz_ring_wave.h"
#include "nxz_verify.h"

namespace nxzv {

using nxzi::uni;

// what the walk calls: with the bytes of every token, for its budget, and in front of every token that does not fit it
struct Hook : nxzr::Writer {             // (the bytes: lit / match / stored into the ring)
	static constexpr bool fine = true;
	static constexpr bool bytes = true;
	const uint32_t *T;
	State *st;

	// ---- the checksum passes ----
	// the whole slices between st->done and output u
	__device__ __forceinline__ void pass(uint32_t u) const
	{
		const uint32_t ns = uni(pass_slices(st->done, u));
		if (!ns) return;
		__syncthreads();                                                     // (one wavefront: the ring's stores are done)
		Part p = lane_pass(ring, st->done, ns, st->crc, (uint32_t)lane, T);
#pragma unroll
		for (int o = 32; o > 0; o >>= 1) {
			p.crc ^= (uint32_t)__shfl_xor((int)p.crc, o, 64);
			p.s1 += (uint32_t)__shfl_xor((int)p.s1, o, 64);
			p.s2 += (uint32_t)__shfl_xor((int)p.s2, o, 64);
		}
		join(*st, ns, uni(p.crc), uni(p.s1), uni(p.s2));
	}
	__device__ __forceinline__ void operator()(uint64_t, uint32_t) const {}
	__device__ __forceinline__ uint32_t budget(uint32_t cap) const { return uni(nxzv::budget(st->cut, cap)); }
	__device__ __forceinline__ void cut(uint64_t, uint32_t out, uint32_t, uint32_t, uint64_t, uint32_t) const
	{
		const uint32_t u = uni(out);
		pass(u);
		st->cut = u;
	}
};

// dwin: NULL, or a dictionary's 32 KiB image whose last dlen bytes are its inflate window (a job that says NXZ_JOB_NO_DICT does
// not get it, as in nxzs::size_kernel)
__global__ __launch_bounds__(64) void verify_kernel(const nxz_batch_job_t *__restrict__ jobs, nxz_batch_result_t *__restrict__ results,
						    const uint32_t *__restrict__ order, const uint8_t *__restrict__ dwin, uint32_t dlen)
{
	__shared__ __attribute__((aligned(16))) nxzs::Smem sm;
	__shared__ __attribute__((aligned(16))) uint32_t ring[NXZ_CB_RING / 4];
	__shared__ __attribute__((aligned(16))) uint32_t T[1024];
	const int lane = threadIdx.x;
	const uint32_t jid = order ? order[blockIdx.x] : blockIdx.x;
	const nxz_batch_job_t job = jobs[jid];
	if (!nxz_size_job_ok(job.resume, job.hist_len)) {
		if (lane == 0) results[jid] = nxz_size_refused();
		return;
	}
	const uint32_t hist_bytes = uni(nxz_size_hist_bytes(job.hist_len, job.src_len));
	uint32_t dl = (dwin && !(job.reserved & NXZ_JOB_NO_DICT)) ? dlen : 0;
	if (dl > NXZ_SIZE_WINDOW - hist_bytes) dl = NXZ_SIZE_WINDOW - hist_bytes;
	dl = uni(dl);
	const uint32_t srclen = uni(job.src_len) - hist_bytes;
	const NXZ_GLOBAL_AS uint8_t *src = (const NXZ_GLOBAL_AS uint8_t *)job.src + hist_bytes;

	// the table, and the window: the job's own bytes end at ring position 32768, the dictionary's in front of them
#pragma unroll
	for (uint32_t k = 0; k < 4; k++) nxzck::table_column(T, (uint32_t)lane + 64 * k);
	if (hist_bytes) nxzr::ring_in(ring, NXZ_CB_RING - hist_bytes, hist_bytes, (const NXZ_GLOBAL_AS uint8_t *)job.src, lane);
	if (dl) nxzr::ring_in(ring, NXZ_CB_RING - hist_bytes - dl, dl, (const NXZ_GLOBAL_AS uint8_t *)dwin + (NXZ_CB_RING - dl), lane);
	__syncthreads();

	State st = begin(uni(job.in_crc), uni(job.in_adler));
	const Hook hook{{ring, lane}, T, &st};
	nxz_size_stop_t stop = {};
	uint64_t end_bit;
	nxzs::walk(sm, src, srclen, uni(job.dst_cap), hist_bytes + dl, lane, stop, end_bit, hook);
	nxz_batch_result_t r = nxz_size_record(&stop, job.src_len);
	if (r.cc == NXZ_CC_OK || r.cc == NXZ_CC_DATA_LENGTH) {
		const uint32_t produced = uni(stop.produced);
		hook.pass(produced);
		__syncthreads();
		tail(st, ring, produced - st.done, T);
		r.crc = crc_of(st); r.adler = adler_of(st);
	}
	if (lane == 0) results[jid] = r;
}

} // namespace nxzv

// n jobs, a wavefront each; order: NULL, or nxz_launch_order_by_length's; dwin / dlen: see verify_kernel
extern "C" int nxz_launch_inflate_verify(const nxz_batch_job_t *jobs, size_t n, nxz_batch_result_t *results, const uint32_t *order,
					 const uint8_t *dwin, uint32_t dlen, hipStream_t stream)
{
	if (!n) return 0;
	hipLaunchKernelGGL(nxzv::verify_kernel, dim3((unsigned)n), dim3(64), 0, stream, jobs, results, order, dwin, dlen);
	return (int)hipGetLastError();
}
