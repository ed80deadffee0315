// nxz_symcount.hip -- the LZ symbol counts of the COMPRESS function codes that count (gfx950, wave64).
//
// Runs between the LZ77 kernel (nxz_lz77.hip) and the table generator (nxz_dhtgen.hip) on the same jobs: the LZ77
// algorithm needs no counts -- only the table generator and the caller's out_lzcount read them -- and the LZ77 kernel is one
// workgroup a CU with nothing beside it to hide the latency of two data-dependent loops of LDS atomics.  Here a workgroup of 256
// threads takes a job, the entropy kernel's geometry and addressing (nxz_encode.hip): the block is [src + hist_len, src + src_len),
// the bitmaps and records are the job's slot of the token scratch.  With 5 KiB of LDS and few registers eight workgroups
// share a CU.
//   matches   the record count is the popcount of the match bitmap over the block's words (not the result record's sfbt: for
//             nxu_run_job's rounds that lies in pinned host memory); the records are walked as they lie, 256 a pass
//   literals  rounds of 2048 positions, 8 a lane: 8 source bytes, one bitmap word, one LDS atomic per literal
//   counts    one histogram a wavefront (lanes that add to the same word are served one after another, and text has about
//             30 distinct literals), summed on the way out: counts[job][316], [256] = 1 (nxzsc:: has the layout and the arithmetic)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "nxz_device.h"
#include "nxz_symcount.h"

namespace nxzsc {

constexpr int NT = (int)LANES;
constexpr int NW = NT / 64;
constexpr uint32_t HSTRIDE = 320;               // 316 counts a wavefront, padded
constexpr uint32_t GROUP = 4;                   // rounds whose loads are in flight together

typedef uint32_t v4u __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(NT) void count_kernel(const nxz_batch_job_t *__restrict__ jobs_, const uint8_t *__restrict__ tokens_,
						    uint32_t *__restrict__ counts_, uint32_t njobs)
{
	__shared__ uint32_t hist[NW][HSTRIDE];
	__shared__ uint32_t wsum[NW];
	const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
	const uint32_t bid = blockIdx.x;
	if (bid >= njobs) return;
	const nxz_batch_job_t job = jobs_[bid];
	const uint32_t total = job.src_len;
	const uint32_t h = job.hist_len < total ? job.hist_len : total;
	const uint32_t n = total - h < BLOCK_MAX ? total - h : BLOCK_MAX;
	// (the source alone: for the jobs of nxz_batch_compress_dict the h bytes below it are NOT memory of the caller's)
	const uint8_t NXZ_GLOBAL_AS *src = (const uint8_t NXZ_GLOBAL_AS *)job.src + h;
	const uint8_t NXZ_GLOBAL_AS *tk = (const uint8_t NXZ_GLOBAL_AS *)tokens_ + (size_t)bid * NXZ_TOK_STRIDE;
	const uint32_t NXZ_GLOBAL_AS *litb = (const uint32_t NXZ_GLOBAL_AS *)(tk + NXZ_TOK_LITBITS);
	const uint32_t NXZ_GLOBAL_AS *tokb = (const uint32_t NXZ_GLOBAL_AS *)(tk + NXZ_TOK_MATCHBITS);
	const uint32_t NXZ_GLOBAL_AS *recs = (const uint32_t NXZ_GLOBAL_AS *)(tk + NXZ_TOK_RECORDS);
	uint32_t NXZ_GLOBAL_AS *out = (uint32_t NXZ_GLOBAL_AS *)counts_ + (size_t)bid * NSYM;
	const uint32_t nwords = (n + 31) >> 5;          // <= 2048: 8 a lane

	// What a lane needs of a round: its 8 source bytes and the bitmap word that holds its 8 positions.  GROUP rounds are asked
	// for together, a group ahead: a block is a chain of a few trips with that many loads in flight, not of 32 with one.
	struct Fetch { uint64_t bytes[GROUP]; uint32_t litw[GROUP]; };
	auto fetch = [&](uint32_t r0, Fetch &f) {
#pragma unroll
		for (uint32_t j = 0; j < GROUP; j++) {
			const uint32_t p0 = r0 + j * RPOS + 8 * t;
			f.bytes[j] = 0; f.litw[j] = 0;
			if (p0 < n) {
				f.litw[j] = litb[p0 >> 5];
				f.bytes[j] = lane_bytes(src, p0, n);
			}
		}
	};

	// ---- how many records: the match bits of the block (the words of the bitmap's 8 KiB, all inside the job's slot) ----
	uint32_t s = 0;
	{
		const v4u NXZ_GLOBAL_AS *tw = (const v4u NXZ_GLOBAL_AS *)tokb;
		v4u a = { 0, 0, 0, 0 }, b = a;
		if (8u * t < nwords) { a = tw[2 * t]; b = tw[2 * t + 1]; }
		const uint32_t w[8] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w };
#pragma unroll
		for (int k = 0; k < 8; k++) s += (uint32_t)__popc(w[k] & word_mask(8u * t + k, n));
	}
	Fetch nx;
	fetch(0, nx);                                                // the first rounds' bytes travel meanwhile
	for (uint32_t i = t; i < NW * HSTRIDE; i += NT) (&hist[0][0])[i] = 0;
	for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
	if (lane == 0) wsum[wave] = s;
	__syncthreads();
	uint32_t nrec = 0;
#pragma unroll
	for (int w = 0; w < NW; w++) nrec += wsum[w];
	if (nrec > NXZ_TOK_MAXREC) nrec = NXZ_TOK_MAXREC;           // (what the record array holds)
	uint32_t *my = hist[wave];

	// ---- matches: four passes of 256 records in flight ----
	for (uint32_t i0 = 0; i0 < nrec; i0 += 4 * NT) {
		uint32_t r[4];
#pragma unroll
		for (int j = 0; j < 4; j++) {
			const uint32_t i = i0 + NT * j + t;
			r[j] = i < nrec ? recs[i] : 0;
		}
#pragma unroll
		for (int j = 0; j < 4; j++) {
			if (i0 + NT * j + t < nrec) {
				uint32_t ls, ds;
				record_symbols(r[j], ls, ds);
				atomicAdd(&my[ls], 1u);
				atomicAdd(&my[ds], 1u);
			}
		}
	}

	// ---- literals ----
	for (uint32_t r0 = 0; r0 < n; r0 += GROUP * RPOS) {
		const Fetch k = nx;
		if (r0 + GROUP * RPOS < n) fetch(r0 + GROUP * RPOS, nx);
#pragma unroll
		for (uint32_t j = 0; j < GROUP; j++)
			lane_literals(k.bytes[j], k.litw[j], r0 + j * RPOS + 8 * t, n, [&](uint32_t sym) { atomicAdd(&my[sym], 1u); });
	}
	__syncthreads();

	// ---- out: the wavefronts' histograms summed, coalesced ----
	for (uint32_t i = t; i < NSYM; i += NT) {
		uint32_t c = 0;
#pragma unroll
		for (int w = 0; w < NW; w++) c += hist[w][i];
		out[i] = i == EOB ? 1u : c;                              // the callers count EOB once (lib/nx_dht.c:189-195)
	}
}

} // namespace nxzsc

// counts[i * 316 ..] of jobs[i] from tokens + i * NXZ_TOK_STRIDE, as the LZ77 kernel's counting forms leave them
extern "C" int nxz_launch_symcount(const nxz_batch_job_t *jobs, size_t n, const uint8_t *tokens, uint32_t *counts, hipStream_t stream)
{
	if (n == 0) return 0;
	hipLaunchKernelGGL(nxzsc::count_kernel, dim3((unsigned)n), dim3(nxzsc::NT), 0, stream, jobs, tokens, counts, (uint32_t)n);
	return (int)hipGetLastError();
}
