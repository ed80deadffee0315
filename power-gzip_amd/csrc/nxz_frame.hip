// nxz_frame.hip -- zlib / gzip framing on the device: the kernels around a raw inflate batch that make it a batch of
// framed streams (nxz_batch_decompress_framed), and the discovery of the members of a BGZF image (nxz_batch_unpack_gzip).
//
// Framed streams (nxz_batch_framed.cpp runs the three steps on the caller's stream, nothing waits for the host):
//   1. frame_header_kernel, a wavefront a job: nxz_frame.h's parser; writes frames[i] and a DERIVED raw job -- the
//      deflate bytes alone (src + hdr_len, src_len - hdr_len - trailer), checksums from 0 / 1 -- so that the inflate
//      routes see exactly what a raw batch holds.  A job whose header fails gets a derived job with no source and no
//      room (src_len = dst_cap = 0): every route ends it at once and writes nothing.
//   2. the raw batch (nxz_batch_decompress) on the derived jobs;
//   3. frame_trailer_kernel, a thread a job: nxz_frame.h's trailer rule -- the trailer behind the final block is read a
//      byte at a time and compared with the raw result's Adler-32 / CRC-32 and length.
//
// BGZF members: a member header can lie anywhere, and a compressed payload can hold bytes that look like one, so
// every position that passes nxz_bgzf_member_size is a CANDIDATE and the members are the candidates reachable from
// position 0 by "next = here + size":
//   bgzf_scan_kernel<false>  16 bytes a lane in steps of 4 KiB, 16 KiB a workgroup: candidates per workgroup
//   tile_scan_kernel         their exclusive prefix sum (one workgroup)
//   bgzf_scan_kernel<true>   the candidates again, written in order at their place (a prefix sum in the workgroup)
//   succ_kernel              succ[k] = the candidate at pos[k] + size[k] (binary search), or the sink
//   jump_kernel              J[r + 1] = J[r] o J[r]: succ^(2^r), log2(candidates) launches
//   chain_kernel             the chain length L from candidate 0 (one lane, log steps) and the bytes it covers
//   member_kernel            the j-th member for all j at once (the bits of j pick the jumps) and its ISIZE
//   layout_kernel            offsets[] = prefix sum of ISIZE; the framed jobs of the members
#include <hip/hip_runtime.h>
#include "nxz_device.h"
#include "nxz_frame.h"
#include "nxz_frame_wave.h"
#include "nxz_size.h"

namespace nxzf {

// four wavefronts a workgroup, a job each (every lane runs the parser on the same bytes: the name / comment scans and
// the header CRC are the steps that use them all)
// (DICT, nxz_batch_decompress_framed_dict: the caller holds a preset dictionary of that DICTID.  The derived job of a zlib
// stream that names it is decoded with the dictionary; every other job's says NXZ_JOB_NO_DICT.)
template <bool DICT>
__device__ __forceinline__ void frame_header_body(int fmt, const nxz_batch_job_t *__restrict__ jobs, uint32_t n,
						  nxz_batch_frame_t *__restrict__ frames, nxz_batch_job_t *__restrict__ derived, uint32_t dictid)
{
	const uint32_t lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (i >= n) return;
	const nxz_batch_job_t job = jobs[i];
	nxz_batch_frame_t f;
	WaveOps ops{lane};
	bool use_dict = false;
	uint32_t st = DICT ? nxz_frame_parse_dict(job.src, job.src_len, fmt, &f, ops, true, dictid, &use_dict) : nxz_frame_parse(job.src, job.src_len, fmt, &f, ops);
	if (st == NXZ_FRAME_OK && (job.resume || job.hist_len)) st = NXZ_FRAME_BAD_HEADER;
	if (st == NXZ_FRAME_OK && job.src_len - f.hdr_len < nxz_frame_trailer_bytes(f.format)) st = NXZ_FRAME_TRUNCATED;
	f.status = st;
	if (lane) return;
	frames[i] = f;
	nxz_batch_job_t d = {};
	d.src = job.src; d.dst = job.dst; d.in_adler = 1;
	if (st == NXZ_FRAME_OK) {
		d.src = job.src + f.hdr_len;
		d.src_len = job.src_len - f.hdr_len - nxz_frame_trailer_bytes(f.format);
		d.dst_cap = job.dst_cap;
	}
	if (DICT && !use_dict) d.reserved = NXZ_JOB_NO_DICT;
	derived[i] = d;
}
__global__ __launch_bounds__(256) void frame_header_kernel(int fmt, const nxz_batch_job_t *__restrict__ jobs, uint32_t n,
							   nxz_batch_frame_t *__restrict__ frames, nxz_batch_job_t *__restrict__ derived)
{
	frame_header_body<false>(fmt, jobs, n, frames, derived, 0);
}
__global__ __launch_bounds__(256) void frame_header_dict_kernel(int fmt, const nxz_batch_job_t *__restrict__ jobs, uint32_t n,
								nxz_batch_frame_t *__restrict__ frames, nxz_batch_job_t *__restrict__ derived, uint32_t dictid)
{
	frame_header_body<true>(fmt, jobs, n, frames, derived, dictid);
}

__global__ __launch_bounds__(256) void frame_trailer_kernel(const nxz_batch_job_t *__restrict__ jobs, uint32_t n,
							    nxz_batch_result_t *__restrict__ results, nxz_batch_frame_t *__restrict__ frames)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	nxz_batch_frame_t *f = &frames[i];
	if (f->status != NXZ_FRAME_OK) {
		results[i] = nxz_size_refused();
		return;
	}
	const nxz_batch_result_t r = results[i];
	const nxz_batch_job_t job = jobs[i];
	uint32_t end, check, isize;
	const uint32_t st = nxz_frame_trailer(f->format, f->hdr_len, &r, job.src, job.src_len, true, &end, &check, &isize);
	f->status = st; f->end = end; f->check = check; f->isize = isize;
}

// ---- BGZF member discovery ----------------------------------------------------------------------------------------------
constexpr uint32_t SUB = 4096;           // bytes of the image a workgroup looks at in one step: 256 lanes x 16
constexpr uint32_t SUBS = 4;             // steps a workgroup (fewer, larger workgroups: 1 GiB is 65 536 of them)
constexpr uint32_t TILE = SUB * SUBS;

// Positions count from `packed`; lane work is aligned to 16-byte granules of the address space (the granule that holds
// packed[0] and the one that holds packed[len - 1] are read whole, as the inflate kernels read their sources).  A step
// covers 4 KiB, a lane's 16 bytes side by side with its neighbours' (coalesced), so the candidates come in position order
// step by step, lane by lane.
template <bool WRITE>
__global__ __launch_bounds__(256) void bgzf_scan_kernel(const uint8_t *__restrict__ packed, uint64_t len, uint32_t *__restrict__ tile_cnt,
							 const uint32_t *__restrict__ tile_off, uint64_t cap, uint64_t *__restrict__ pos,
							 uint32_t *__restrict__ size)
{
	__shared__ uint32_t wsum[SUBS][4];
	const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
	const uint64_t head = (uintptr_t)packed & 15;                           // packed[0] sits at this byte of its granule
	const uint8_t *base = packed - head;
	const uint64_t end = head + len;
	uint32_t mask[SUBS], incl[SUBS];                                        // bit k: a candidate at a0 + k
#pragma unroll
	for (uint32_t g = 0; g < SUBS; g++) {
		const uint64_t a0 = (uint64_t)blockIdx.x * TILE + g * SUB + (uint64_t)t * 16;    // granule offset from base
		uint32_t m = 0;
		if (a0 < end) {
			const uint4 g0 = *(const uint4 *)(base + a0);
			const uint4 g1 = a0 + 16 < end ? *(const uint4 *)(base + a0 + 16) : make_uint4(0, 0, 0, 0);
			const uint32_t w[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
#pragma unroll
			for (uint32_t k = 0; k < 16; k++) {
				const uint32_t v = (k & 3) ? __builtin_amdgcn_alignbyte(w[(k >> 2) + 1], w[k >> 2], k & 3) : w[k >> 2];
				const uint64_t a = a0 + k;
				if (v == 0x04088b1fu && a >= head && a < end && nxz_bgzf_member_size(base + a, end - a)) m |= 1u << k;
			}
		}
		mask[g] = m;
		// each lane's place in its wavefront's step
		uint32_t c = (uint32_t)__popc(m);
		for (int d = 1; d < 64; d <<= 1) { const uint32_t v = (uint32_t)__shfl_up((int)c, d, 64); if (lane >= (uint32_t)d) c += v; }
		incl[g] = c;
		if (lane == 63) wsum[g][wave] = c;
	}
	__syncthreads();
	if (!WRITE) {
		if (t == 0) {
			uint32_t sum = 0;
			for (uint32_t g = 0; g < SUBS; g++) sum += wsum[g][0] + wsum[g][1] + wsum[g][2] + wsum[g][3];
			tile_cnt[blockIdx.x] = sum;
		}
		return;
	}
	uint64_t o0 = tile_off[blockIdx.x];
#pragma unroll
	for (uint32_t g = 0; g < SUBS; g++) {
		uint32_t m = mask[g];
		uint64_t o = o0 + incl[g] - (uint32_t)__popc(m);
		for (uint32_t w2 = 0; w2 < wave; w2++) o += wsum[g][w2];
		const uint64_t a0 = (uint64_t)blockIdx.x * TILE + g * SUB + (uint64_t)t * 16;
		for (; m; m &= m - 1, o++) {
			const uint64_t a = a0 + (uint32_t)__builtin_ctz(m);
			if (o < cap) { pos[o] = a - head; size[o] = nxz_bgzf_member_size(base + a, end - a); }
		}
		o0 += wsum[g][0] + wsum[g][1] + wsum[g][2] + wsum[g][3];
	}
}

// exclusive prefix sum of the tiles' counts; ctl[0] = candidates
__global__ __launch_bounds__(1024) void tile_scan_kernel(const uint32_t *__restrict__ cnt, uint32_t ntiles, uint32_t *__restrict__ off,
							  uint64_t *__restrict__ ctl)
{
	__shared__ uint64_t part[1024];
	const uint32_t t = threadIdx.x, per = (ntiles + 1023) / 1024;
	const uint32_t lo = t * per < ntiles ? t * per : ntiles, hi = lo + per < ntiles ? lo + per : ntiles;
	uint64_t sum = 0;
	for (uint32_t i = lo; i < hi; i++) sum += cnt[i];
	part[t] = sum;
	__syncthreads();
	for (uint32_t d = 1; d < 1024; d <<= 1) {
		const uint64_t v = t >= d ? part[t - d] : 0;
		__syncthreads();
		part[t] += v;
		__syncthreads();
	}
	uint64_t o = part[t] - sum;
	for (uint32_t i = lo; i < hi; i++) { off[i] = (uint32_t)o; o += cnt[i]; }
	if (t == 1023) ctl[0] = part[1023];
}

__device__ inline uint32_t cands(const uint64_t *ctl, uint64_t cap) { return (uint32_t)(ctl[0] < cap ? ctl[0] : cap); }

// J0[k] = the candidate that starts where candidate k ends, or the sink (index C, its own successor)
__global__ __launch_bounds__(256) void succ_kernel(const uint64_t *__restrict__ pos, const uint32_t *__restrict__ size, const uint64_t *__restrict__ ctl,
						   uint64_t cap, uint32_t *__restrict__ J0)
{
	const uint32_t C = cands(ctl, cap);
	const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (k > C) return;
	uint32_t s = C;
	if (k < C) {
		const uint64_t want = pos[k] + size[k];
		uint32_t lo = (uint32_t)k + 1, hi = C;                             // (sorted: the successor lies further on)
		while (lo < hi) { const uint32_t m = (lo + hi) >> 1; if (pos[m] < want) lo = m + 1; else hi = m; }
		if (lo < C && pos[lo] == want) s = lo;
	}
	J0[k] = s;
}

__global__ __launch_bounds__(256) void jump_kernel(const uint32_t *__restrict__ Jr, const uint64_t *__restrict__ ctl, uint64_t cap, uint32_t *__restrict__ Jn)
{
	const uint32_t C = cands(ctl, cap);
	const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (k <= C) Jn[k] = Jr[Jr[k]];
}

// ctl[1] = L, the members: the chain from candidate 0 when that stands at position 0 (else none); ctl[2] = the bytes they cover
__global__ void chain_kernel(const uint64_t *__restrict__ pos, const uint32_t *__restrict__ size, uint64_t *__restrict__ ctl, uint64_t cap,
			     const uint32_t *__restrict__ J, uint32_t levels)
{
	const uint32_t C = cands(ctl, cap);
	uint64_t L = 0, used = 0;
	if (C && pos[0] == 0) {
		uint32_t cur = 0;
		L = 1;
		for (int r = (int)levels - 1; r >= 0; r--) {
			const uint32_t nx = J[(uint64_t)r * (cap + 1) + cur];
			if (nx != C) { cur = nx; L += 1ull << r; }
		}
		used = pos[cur] + size[cur];
	}
	ctl[1] = L; ctl[2] = used; ctl[3] = 0;
}

// members[j] for j < L, when they fit max_members, and their ISIZE
__global__ __launch_bounds__(256) void member_kernel(const uint8_t *__restrict__ packed, const uint64_t *__restrict__ pos, const uint32_t *__restrict__ size,
						     const uint64_t *__restrict__ ctl, uint64_t cap, const uint32_t *__restrict__ J, uint32_t levels,
						     uint64_t max_members, uint32_t *__restrict__ memb, uint32_t *__restrict__ isz)
{
	const uint64_t L = ctl[1], j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (L > max_members || j >= L) return;
	uint32_t cur = 0;
	for (uint32_t r = 0; r < levels; r++)
		if ((j >> r) & 1) cur = J[(uint64_t)r * (cap + 1) + cur];
	memb[j] = cur;
	isz[j] = nxz_rd32le(packed + pos[cur] + size[cur] - 4);
}

// offsets[0..L] and the members' framed jobs; ctl[3] = sum of ISIZE (one workgroup)
__global__ __launch_bounds__(1024) void layout_kernel(const uint8_t *__restrict__ packed, const uint64_t *__restrict__ pos, const uint32_t *__restrict__ size,
						      uint64_t *__restrict__ ctl, uint64_t max_members, const uint32_t *__restrict__ memb,
						      const uint32_t *__restrict__ isz, uint8_t *dst, uint64_t *__restrict__ offsets,
						      nxz_batch_job_t *__restrict__ jobs)
{
	__shared__ uint64_t part[1024];
	const uint64_t L = ctl[1];
	if (L == 0 || L > max_members) return;
	const uint32_t t = threadIdx.x;
	const uint64_t per = (L + 1023) / 1024;
	const uint64_t lo = t * per < L ? t * per : L, hi = lo + per < L ? lo + per : L;
	uint64_t sum = 0;
	for (uint64_t i = lo; i < hi; i++) sum += isz[i];
	part[t] = sum;
	__syncthreads();
	for (uint32_t d = 1; d < 1024; d <<= 1) {
		const uint64_t v = t >= d ? part[t - d] : 0;
		__syncthreads();
		part[t] += v;
		__syncthreads();
	}
	uint64_t o = part[t] - sum;
	for (uint64_t i = lo; i < hi; i++) {
		const uint32_t m = memb[i];
		nxz_batch_job_t jb = {};
		jb.src = packed + pos[m]; jb.src_len = size[m];
		jb.dst = dst + o; jb.dst_cap = isz[i]; jb.in_adler = 1;
		jobs[i] = jb;
		offsets[i] = o;
		o += isz[i];
	}
	if (t == 1023) { offsets[L] = part[1023]; ctl[3] = part[1023]; }
}

// coff[j] = where member j starts, coff[L] = the bytes the members cover (nxz_bgzf_index; uoff is layout_kernel's offsets)
__global__ __launch_bounds__(256) void coff_kernel(const uint64_t *__restrict__ pos, const uint64_t *__restrict__ ctl, uint64_t max_members,
						   const uint32_t *__restrict__ memb, uint64_t *__restrict__ coff)
{
	const uint64_t L = ctl[1], j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (L == 0 || L > max_members || j > L) return;
	coff[j] = j < L ? pos[memb[j]] : ctl[2];
}

} // namespace nxzf

extern "C" int nxz_launch_frame_header(int fmt, const nxz_batch_job_t *jobs, size_t n, nxz_batch_frame_t *frames, nxz_batch_job_t *derived, hipStream_t stream)
{
	if (!n) return 0;
	hipLaunchKernelGGL(nxzf::frame_header_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream, fmt, jobs, (uint32_t)n, frames, derived);
	return (int)hipGetLastError();
}

extern "C" int nxz_launch_frame_header_dict(int fmt, const nxz_batch_job_t *jobs, size_t n, nxz_batch_frame_t *frames, nxz_batch_job_t *derived,
					    uint32_t dictid, hipStream_t stream)
{
	if (!n) return 0;
	hipLaunchKernelGGL(nxzf::frame_header_dict_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream, fmt, jobs, (uint32_t)n, frames, derived, dictid);
	return (int)hipGetLastError();
}

extern "C" int nxz_launch_frame_trailer(const nxz_batch_job_t *jobs, size_t n, nxz_batch_result_t *results, nxz_batch_frame_t *frames, hipStream_t stream)
{
	if (!n) return 0;
	hipLaunchKernelGGL(nxzf::frame_trailer_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, jobs, (uint32_t)n, results, frames);
	return (int)hipGetLastError();
}

// Workspace of the discovery for an image of `len` bytes and room for `cap` candidates (the layout of nxz_launch_bgzf_discover)
static uint32_t bgzf_levels(uint64_t cap) { uint32_t r = 1; while ((1ull << r) <= cap + 1) r++; return r; }
static size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
extern "C" size_t nxz_bgzf_workspace(uint64_t len, uint64_t cap)
{
	const uint64_t tiles = (len + 15 + nxzf::TILE - 1) / nxzf::TILE + 1;
	return up256(4 * sizeof(uint64_t)) + 2 * up256(tiles * 4) + up256(cap * 8) + up256(cap * 4) * 3 + up256((size_t)bgzf_levels(cap) * (cap + 1) * 4) +
	       up256(cap * sizeof(nxz_batch_job_t));
}

// The discovery's arrays inside ws (nxz_launch_bgzf_discover, nxz_launch_bgzf_coff)
struct BgzfWs {
	uint64_t *ctl, *pos;
	uint32_t *tile_cnt, *tile_off, *size, *memb, *isz, *J;
	nxz_batch_job_t *jobs;
	uint64_t tiles;
	uint32_t levels;
};
static BgzfWs bgzf_ws(uint8_t *ws, const uint8_t *packed, uint64_t len, uint64_t cap)
{
	BgzfWs w;
	w.tiles = (len + ((uintptr_t)packed & 15) + nxzf::TILE - 1) / nxzf::TILE;
	w.levels = bgzf_levels(cap);
	uint8_t *p = ws;
	auto take = [&](size_t b) { uint8_t *q = p; p += up256(b); return q; };
	w.ctl = (uint64_t *)take(4 * sizeof(uint64_t));
	w.tile_cnt = (uint32_t *)take(w.tiles * 4 + 4); w.tile_off = (uint32_t *)take(w.tiles * 4 + 4);
	w.pos = (uint64_t *)take(cap * 8);
	w.size = (uint32_t *)take(cap * 4); w.memb = (uint32_t *)take(cap * 4); w.isz = (uint32_t *)take(cap * 4);
	w.J = (uint32_t *)take((size_t)w.levels * (cap + 1) * 4);
	w.jobs = (nxz_batch_job_t *)take(cap * sizeof(nxz_batch_job_t));
	return w;
}

// Finds the members of the image and lays them out.  ws[0..3] (uint64, device): candidates, members L, bytes covered, sum of ISIZE.
// When L <= max_members: offsets[0..L] and *jobs (inside ws) are written.  When candidates > cap, the chain is not complete:
// the caller grows cap to the count and runs it again.
extern "C" int nxz_launch_bgzf_discover(const uint8_t *packed, uint64_t len, uint8_t *dst, uint64_t *offsets, uint64_t max_members, uint8_t *ws,
					uint64_t cap, nxz_batch_job_t **jobs, hipStream_t stream)
{
	const BgzfWs w = bgzf_ws(ws, packed, len, cap);
	const uint64_t tiles = w.tiles;
	const uint32_t levels = w.levels;
	uint64_t *ctl = w.ctl, *pos = w.pos;
	uint32_t *tile_cnt = w.tile_cnt, *tile_off = w.tile_off, *size = w.size, *memb = w.memb, *isz = w.isz, *J = w.J;
	*jobs = w.jobs;
	(void)hipMemsetAsync(ctl, 0, 4 * sizeof(uint64_t), stream);
	if (tiles == 0 || tiles >= (1ull << 31)) return tiles ? (int)hipErrorInvalidValue : 0;
	hipLaunchKernelGGL(nxzf::bgzf_scan_kernel<false>, dim3((unsigned)tiles), dim3(256), 0, stream, packed, len, tile_cnt, nullptr, cap, nullptr, nullptr);
	hipLaunchKernelGGL(nxzf::tile_scan_kernel, dim3(1), dim3(1024), 0, stream, tile_cnt, (uint32_t)tiles, tile_off, ctl);
	hipLaunchKernelGGL(nxzf::bgzf_scan_kernel<true>, dim3((unsigned)tiles), dim3(256), 0, stream, packed, len, nullptr, tile_off, cap, pos, size);
	const unsigned g = (unsigned)((cap + 1 + 255) / 256);
	hipLaunchKernelGGL(nxzf::succ_kernel, dim3(g), dim3(256), 0, stream, pos, size, ctl, cap, J);
	// (C is known on the device only: the levels lie cap + 1 entries apart, and every kernel works on the first C + 1)
	for (uint32_t r = 0; r + 1 < levels; r++)
		hipLaunchKernelGGL(nxzf::jump_kernel, dim3(g), dim3(256), 0, stream, J + (size_t)r * (cap + 1), ctl, cap, J + (size_t)(r + 1) * (cap + 1));
	hipLaunchKernelGGL(nxzf::chain_kernel, dim3(1), dim3(1), 0, stream, pos, size, ctl, cap, J, levels);
	hipLaunchKernelGGL(nxzf::member_kernel, dim3(g), dim3(256), 0, stream, packed, pos, size, ctl, cap, J, levels, max_members, memb, isz);
	hipLaunchKernelGGL(nxzf::layout_kernel, dim3(1), dim3(1024), 0, stream, packed, pos, size, ctl, max_members, memb, isz, dst, offsets, *jobs);
	return (int)hipGetLastError();
}


// After nxz_launch_bgzf_discover on the same ws, len and cap: coff[0..L] when 0 < L <= max_members
extern "C" int nxz_launch_bgzf_coff(const uint8_t *packed, uint64_t len, uint8_t *ws, uint64_t cap, uint64_t max_members, uint64_t *coff,
				    hipStream_t stream)
{
	const BgzfWs w = bgzf_ws(ws, packed, len, cap);
	const uint64_t most = (max_members < cap ? max_members : cap) + 1;
	hipLaunchKernelGGL(nxzf::coff_kernel, dim3((unsigned)((most + 255) / 256)), dim3(256), 0, stream, w.pos, w.ctl, max_members, w.memb, coff);
	return (int)hipGetLastError();
}
