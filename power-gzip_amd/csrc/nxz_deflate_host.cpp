// nxz_deflate_host.cpp -- nxz_deflate_host: a long HOST buffer as one raw deflate stream, through a pair of lanes of the
// caller's own or merged with the calls of other threads (the GF(2) and Adler joins of the blocks' checksums are here too).
#include "nxz_ctx.h"

// ---------------------------------------------------------------------------
// nxz_deflate_host: a long HOST buffer -> one raw deflate stream in a HOST buffer
// ---------------------------------------------------------------------------
#define HOST_GROUP 256u                    /* blocks per group: 16 MiB in, one launch of each kernel */
#define STAGE_MAX_BLOCKS 64u               /* groups up to this many blocks go through the lane's pinned staging */
#define HOST_SLOT 73856u                   /* room for one block's output (nxz_compress_bound(65536) rounded) */

static uint32_t gf2_mul32(uint32_t a, uint32_t b)
{
	uint32_t p = 0;
	for (uint32_t m = 0x80000000u; m; m >>= 1) {
		if (a & m) p ^= b;
		b = (b >> 1) ^ ((b & 1) ? 0xedb88320u : 0);
	}
	return p;
}
static uint32_t crc_shift_op(uint64_t nbytes)                       // x^(8 nbytes) mod P, reflected
{
	uint32_t r = 0x80000000u, sq = 0x00800000u;
	for (uint64_t n = nbytes; n; n >>= 1) { if (n & 1) r = gf2_mul32(r, sq); sq = gf2_mul32(sq, sq); }
	return r;
}
static uint32_t adler_join(uint32_t a1, uint32_t a2, uint64_t len2)
{
	const uint64_t B = 65521, rem = len2 % B, s1 = a1 & 0xffff;
	const uint64_t sum1 = (s1 + (a2 & 0xffff) + B - 1) % B;
	const uint64_t sum2 = (rem * s1 + (a1 >> 16) + (a2 >> 16) + B - rem) % B;
	return (uint32_t)((sum2 << 16) | sum1);
}

// the source bytes a block takes when hist_max bytes of what lies in front of it are its window
// (window + block <= 64 KiB, both multiples of 16)
static inline size_t host_block_bytes(uint32_t hist_max)
{
	const uint32_t h = hist_max > 32768u ? 32768u : hist_max & ~15u;
	return SUBBLOCK - h;
}
extern "C" size_t nxz_deflate_host_bound_hist(size_t src_len, uint32_t hist_max)
{
	const size_t B = host_block_bytes(hist_max);
	return src_len + ((src_len + B - 1) / B) * 10 + 16;
}
extern "C" size_t nxz_deflate_host_bound(size_t src_len) { return nxz_deflate_host_bound_hist(src_len, 0); }

// (the two lanes of a pair get streams of different priority: the runtime maps streams onto a few hardware
// queues, and two streams of one priority may share a queue, depending on what other streams the process has
// made before -- then the copies of one lane and the kernels of the other run one after the other)
// a lane's stream (made once) and its buffers for `blocks` blocks per group (grow only, a power of two from 32 up to
// HOST_GROUP: a caller of megabyte-sized calls holds 2 x 6 MiB, not 2 x 50 -- with 16 pairs of lanes that is what a
// process of many threads pays when each makes its first call)
static bool lane_need(nxz_ctx::HostLane &l, bool high, size_t blocks)
{
	if (!l.stream) {
		int least = 0, greatest = 0;
		(void)hipDeviceGetStreamPriorityRange(&least, &greatest);
		HIPCHK(hipStreamCreateWithPriority(&l.stream, hipStreamNonBlocking, high ? greatest : least), return false);
	}
	if (blocks <= l.cap) return true;
	size_t cap = 32;
	while (cap < blocks) cap <<= 1;
	if (cap > HOST_GROUP) cap = HOST_GROUP;
	if (l.cap) {
		(void)hipStreamSynchronize(l.stream);
		(void)hipFree(l.d_base); (void)hipHostFree(l.h_base);
		l.d_base = l.h_base = nullptr;
		l.d_src = l.d_dst = l.d_packed = nullptr; l.d_jobs = l.h_jobs = nullptr; l.d_res = l.h_res = nullptr; l.d_off = nullptr; l.h_total = nullptr;
		l.h_src = l.h_packed = nullptr;
		l.cap = 0;
	}
	// one allocation on either side (round 4 made nine: with sixteen threads at their first call 30 streams and some 400
	// allocations went through the runtime's lock one after the other -- 480 ms before the first call came back)
	auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
	const size_t o_src = 0, o_dst = o_src + up(cap * SUBBLOCK), o_packed = o_dst + up(cap * HOST_SLOT), o_jobs = o_packed + up(cap * (SUBBLOCK + 16)),
		     o_res = o_jobs + up(cap * sizeof(nxz_batch_job_t)), o_off = o_res + up(cap * sizeof(nxz_batch_result_t)), d_total = o_off + up((cap + 1) * sizeof(uint64_t));
	// Calls of a few MiB from many threads: the caller's pages are not pinned, and a copy straight from them makes the
	// runtime pin and unpin them per call under the process's memory-map lock -- sixteen threads of 1 MiB calls ran at
	// 4 GiB/s that way.  Up to STAGE_MAX_BLOCKS per group the lane has pinned staging of its own: the calling thread
	// copies in and out of it (its own core's time), the DMA runs from pinned memory.
	static const bool stage_on = !(getenv("NXZ_HOST_STAGE") && atoi(getenv("NXZ_HOST_STAGE")) == 0);
	const bool stage = stage_on && cap <= STAGE_MAX_BLOCKS;
	const size_t p_jobs = 0, p_res = p_jobs + up(cap * sizeof(nxz_batch_job_t)), p_total = p_res + up(cap * sizeof(nxz_batch_result_t)),
		     p_src = p_total + 256, p_packed = p_src + (stage ? up(cap * SUBBLOCK) : 0), h_total_bytes = p_packed + (stage ? up(cap * (SUBBLOCK + 16)) : 0);
	HIPCHK(hipMalloc((void **)&l.d_base, d_total), return false);
	HIPCHK(hipHostMalloc((void **)&l.h_base, h_total_bytes), { (void)hipFree(l.d_base); l.d_base = nullptr; return false; });
	l.d_src = l.d_base + o_src; l.d_dst = l.d_base + o_dst; l.d_packed = l.d_base + o_packed;
	l.d_jobs = (nxz_batch_job_t *)(l.d_base + o_jobs); l.d_res = (nxz_batch_result_t *)(l.d_base + o_res); l.d_off = (uint64_t *)(l.d_base + o_off);
	l.h_jobs = (nxz_batch_job_t *)(l.h_base + p_jobs); l.h_res = (nxz_batch_result_t *)(l.h_base + p_res); l.h_total = (uint64_t *)(l.h_base + p_total);
	l.h_src = stage ? l.h_base + p_src : nullptr; l.h_packed = stage ? l.h_base + p_packed : nullptr;
	l.cap = cap;
	return true;
}

// ---- calls of a few MiB from many threads: one batch for the callers that are there together ------------------
// A caller takes room for its blocks in the merge that is open (same function code and window), copies its source into
// the merge's pinned staging and writes its job records -- every caller on its own core, side by side -- and waits.  The
// merge goes out when all who took room have filled it and fewer than NXZ_MERGE_RUNNING (2) merges are in flight (so the
// first caller goes alone at once and those who come while it is in flight go together, as in round_submit): whoever
// sees that first queues one copy of the staging, nxz_batch_compress over all blocks and the two kernels that pack every
// member's blocks as that member's stream straight into pinned memory, waits for the stream, and wakes the rest.  Each
// caller then joins its blocks' checksums and copies its stream out.  Returns -EAGAIN when the merges cannot be set up
// (the caller's own pair of lanes takes the call).
#define MERGE_CAP 512u                     /* block slots of a merge: 32 MiB in */
#define MERGE_MEMBERS 64u
#define MERGE_OUT_STRIDE (SUBBLOCK + 32)   /* room per block in the packed staging: nxz_deflate_host_bound of a member fits its blocks' room */
static uint32_t merge_max_blocks()
{
	const char *e = getenv("NXZ_MERGE_MAX_BLOCKS");                 // (read at every call: the tests switch it; 0: never)
	const long x = e ? atol(e) : 128;
	return (uint32_t)(x < 0 ? 0 : x > 256 ? 256 : x);
}
static bool merge_init(nxz_ctx *c, nxz_ctx::Merge &m)
{
	if (m.ready) return true;
	static std::atomic<unsigned> turn{0};
	auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
	const size_t p_src = 0, p_packed = p_src + up((size_t)MERGE_CAP * SUBBLOCK), p_jobs = p_packed + up((size_t)MERGE_CAP * MERGE_OUT_STRIDE),
		     p_res = p_jobs + up(MERGE_CAP * sizeof(nxz_batch_job_t)), p_off = p_res + up(MERGE_CAP * sizeof(nxz_batch_result_t)),
		     p_mem = p_off + up((MERGE_CAP + MERGE_MEMBERS) * sizeof(uint64_t)), p_of = p_mem + up(MERGE_MEMBERS * sizeof(nxz_pack_member_t)),
		     p_total = p_of + up(MERGE_CAP * sizeof(uint16_t));
	const size_t o_src = 0, o_dst = up((size_t)MERGE_CAP * SUBBLOCK), d_total = o_dst + up((size_t)MERGE_CAP * HOST_SLOT);
	if (!m.stream) { HIPCHK(stream_create_spread(&m.stream, turn.fetch_add(1)), return false); }
	HIPCHK(hipMalloc((void **)&m.d_base, d_total), return false);
	HIPCHK(hipHostMalloc((void **)&m.h_base, p_total), { (void)hipFree(m.d_base); m.d_base = nullptr; return false; });
	m.h_src = m.h_base + p_src; m.h_packed = m.h_base + p_packed;
	m.h_jobs = (nxz_batch_job_t *)(m.h_base + p_jobs); m.h_res = (nxz_batch_result_t *)(m.h_base + p_res); m.h_off = (uint64_t *)(m.h_base + p_off);
	m.h_mem = (nxz_pack_member_t *)(m.h_base + p_mem); m.h_member_of = (uint16_t *)(m.h_base + p_of);
	m.d_src = m.d_base + o_src; m.d_dst = m.d_base + o_dst;
	{
		// the stream's token scratch for a full merge at once (it grows only, and every step up is a free and an allocation)
		with_scratch(c, m.stream, [](nxz_ctx::Scratch &r) {
			if (r.chunk_cap < MERGE_CAP) { if (r.d_tokens) r.release_chunk(); (void)r.alloc_chunk(MERGE_CAP); }
		});
	}
	m.ready = true;
	return true;
}

static int merged_deflate(nxz_ctx_t *c, int fc, const uint8_t *src, size_t src_len, int final, uint32_t H, size_t B,
			  const uint8_t *prev, size_t prev_len, uint8_t *dst, size_t *out_len, uint32_t *crc, uint32_t *adler)
{
	typedef nxz_ctx::Merge Merge;
	static const unsigned running_max = [] { const char *e = getenv("NXZ_MERGE_RUNNING"); int v = e ? atoi(e) : 2; return (unsigned)(v < 1 ? 1 : v > 3 ? 3 : v); }();
	const uint32_t nblk = (uint32_t)((src_len + B - 1) / B);
	const uint32_t h0 = !H ? 0 : (uint32_t)std::min<size_t>(H, prev_len) & ~15u;     // the window in front of the call's first block
	const uint32_t need = nblk + (h0 ? 1 : 0);                                     // staging slots: [window][blocks]
	std::unique_lock<std::mutex> lk(c->mm);
	Merge *M = nullptr;
	for (;;) {
		Merge *fresh = nullptr;
		for (auto &m : c->merges) {
			if (m.state == Merge::OPEN && m.fc == fc && m.H == H && m.slots + need <= MERGE_CAP && m.members < MERGE_MEMBERS) { M = &m; break; }
			if (m.state == Merge::FREE && !fresh) fresh = &m;
		}
		if (!M && fresh) {
			if (!merge_init(c, *fresh)) return -EAGAIN;
			M = fresh; M->state = Merge::OPEN; M->fc = fc; M->H = H; M->slots = M->jobs = M->members = M->filled = M->left = 0; M->rc = 0;
		}
		if (M) break;
		c->mcv.wait(lk);
	}
	const uint32_t me = M->members++, s0 = M->slots, j0 = M->jobs;
	M->slots += need; M->jobs += nblk; M->left++;
	lk.unlock();

	// my part of the staging, my job records, my line of the member table
	uint8_t *const stage = M->h_src + (size_t)s0 * SUBBLOCK;
	uint8_t *const dsrc = M->d_src + (size_t)s0 * SUBBLOCK;
	if (h0) memcpy(stage, prev + prev_len - h0, h0);
	memcpy(stage + h0, src, src_len);
	for (uint32_t k = 0; k < nblk; k++) {
		nxz_batch_job_t &j = M->h_jobs[j0 + k];
		memset(&j, 0, sizeof(j));
		const uint32_t hk = (uint32_t)std::min<uint64_t>(H, h0 + (uint64_t)k * B);     // (a multiple of 16: h0, B and H are)
		j.src = dsrc + h0 + (size_t)k * B - hk; j.dst = M->d_dst + (size_t)(j0 + k) * HOST_SLOT;
		j.hist_len = hk;
		j.src_len = hk + (uint32_t)std::min<uint64_t>(B, src_len - (uint64_t)k * B);
		j.dst_cap = HOST_SLOT; j.in_crc = 0; j.in_adler = 1;
		M->h_member_of[j0 + k] = (uint16_t)me;
	}
	nxz_pack_member_t &pm = M->h_mem[me];
	pm.b0 = j0; pm.n = nblk; pm.fin = final ? j0 + nblk - 1 : 0xffffffffu; pm.off0 = j0 + me;
	pm.packed = M->h_packed + (size_t)j0 * MERGE_OUT_STRIDE;

	lk.lock();
	M->filled++;
	while (M->state == Merge::OPEN) {
		unsigned running = 0;
		for (auto &m : c->merges) if (m.state == Merge::RUNNING) running++;
		if (M->filled < M->members || running >= running_max) { c->mcv.wait(lk); continue; }
		// it goes out, and I am the one to send it
		M->state = Merge::RUNNING;
		const uint32_t nj = M->jobs, ns = M->slots, nm = M->members;
		lk.unlock();
		int rc = 0;
		(void)hipSetDevice(c->device);
		if (hipMemcpyAsync(M->d_src, M->h_src, (size_t)ns * SUBBLOCK, hipMemcpyHostToDevice, M->stream) != hipSuccess) rc = -EIO;
		if (!rc) rc = nxz_batch_compress(c, M->fc, M->h_jobs, nj, nullptr, 0, M->h_res, nullptr, M->stream);
		if (!rc && nxz_launch_pack_member_streams(M->h_jobs, M->h_res, nj, M->h_mem, nm, M->h_member_of, M->h_off, M->stream)) rc = -EIO;
		if (hipStreamSynchronize(M->stream) != hipSuccess && !rc) rc = -EIO;
		lk.lock();
		M->rc = rc;
		M->state = Merge::DONE;
		c->mcv.notify_all();
	}
	while (M->state != Merge::DONE) c->mcv.wait(lk);
	const int rc = M->rc;
	lk.unlock();

	if (!rc) {
		const uint64_t total = M->h_off[pm.off0 + nblk];
		memcpy(dst, pm.packed, total);
		const uint32_t op_block = crc_shift_op(B);
		uint32_t run_crc = 0, run_adler = 1;
		for (uint32_t k = 0; k < nblk; k++) {
			const nxz_batch_job_t &j = M->h_jobs[j0 + k];
			const uint32_t len = j.src_len - j.hist_len;
			run_crc = gf2_mul32(run_crc, len == B ? op_block : crc_shift_op(len)) ^ M->h_res[j0 + k].crc;
			run_adler = adler_join(run_adler, M->h_res[j0 + k].adler, len);
		}
		*out_len = total;
		if (crc) *crc = run_crc;
		if (adler) *adler = run_adler;
	}
	lk.lock();
	if (--M->left == 0) { M->state = Merge::FREE; c->mcv.notify_all(); }
	lk.unlock();
	return rc;
}

extern "C" int nxz_deflate_host(nxz_ctx_t *c, int fc, const uint8_t *src, size_t src_len, int final,
				uint8_t *dst, size_t dst_cap, size_t *out_len, uint32_t *crc, uint32_t *adler)
{
	return nxz_deflate_host_hist(c, fc, src, src_len, final, 0, nullptr, 0, dst, dst_cap, out_len, crc, adler);
}

// The same with a window: every block sees the hist_max bytes of the INPUT in front of it (the levels that carry
// history from job to job, lib/nx_deflate.c:654-680,845-862: the history of a job is just the bytes in front of
// it, known up front, so the jobs do not depend on each other); the first block's window is the tail of `prev`
// (what the stream kept of earlier calls).  Blocks are 64 KiB - hist_max long (window + block <= 64 KiB).
extern "C" int nxz_deflate_host_hist(nxz_ctx_t *c, int fc, const uint8_t *src, size_t src_len, int final, uint32_t hist_max,
				     const uint8_t *prev, size_t prev_len, uint8_t *dst, size_t dst_cap, size_t *out_len, uint32_t *crc, uint32_t *adler)
{
	if (!c || !src || !dst || !out_len || !src_len) return -EINVAL;
	if (fc != NXZ_FC_COMPRESS_FHT && fc != NXZ_FC_COMPRESS_DHTGEN) return -EINVAL;
	if (forked_child()) return -ENODEV;
	if (dst_cap < nxz_deflate_host_bound_hist(src_len, hist_max)) return -E2BIG;
	const uint32_t H = (uint32_t)(SUBBLOCK - host_block_bytes(hist_max));      // window bytes per block
	const size_t B = SUBBLOCK - H;
	if (H) fc |= 0x08;                                                  // the RESUME forms take hist_len
	if (!prev) prev_len = 0;
	(void)hipSetDevice(c->device);
	// (a call of more than 64 blocks that is alone takes its own pair of lanes, whose groups overlap copies and kernels: 16 MiB
	// on one thread 8.1 against 6.8 GiB/s merged; with others about, merged: sixteen threads of 8 MiB calls 12.4 -> 28-29 GiB/s.
	// Not beyond 128 blocks: two members of 16 MiB fill a merge, 17 GiB/s either way.)
	struct InCall { std::atomic<int> &n; int mine; InCall(std::atomic<int> &a) : n(a), mine(a.fetch_add(1) + 1) {} ~InCall() { n.fetch_sub(1); } } in_call(c->host_callers);
	const size_t nblk_all = (src_len + B - 1) / B;
	const uint32_t mmax = merge_max_blocks();
	if (nblk_all <= mmax && (nblk_all <= 64 || in_call.mine > 1)) {
		const int r = merged_deflate(c, fc, src, src_len, final, H, B, prev, prev_len, dst, out_len, crc, adler);
		if (r != -EAGAIN) return r;
	}
	// A call beyond the merge's limit while other callers are about goes through the merges in slices of that many blocks, one
	// after the other (every block of a stream starts on a byte boundary and sees the input in front of it as its window, so the
	// slices' streams laid end to end ARE the call's stream, byte for byte): sixteen threads of 16 MiB calls on four pairs of
	// lanes of their own ran at half the rate of 8 MiB calls (14 against 30 GiB/s).  NXZ_MERGE_SLICES=0: own lanes as before.
	const char *sle = getenv("NXZ_MERGE_SLICES");                       // (read at every call: the tests switch it)
	if (!(sle && atoi(sle) == 0) && nblk_all > mmax && mmax >= 64 && in_call.mine > 1) {
		const size_t S = (size_t)mmax * B;
		size_t off = 0, pos = 0;
		uint32_t run_crc = 0, run_adler = 1;
		while (off < src_len) {
			const size_t len = std::min<size_t>(S, src_len - off);
			size_t got = 0;
			uint32_t ck = 0, ak = 1;
			const int r = merged_deflate(c, fc, src + off, len, final && off + len == src_len, H, B, off ? src : prev, off ? off : prev_len, dst + pos, &got, &ck, &ak);
			if (r == -EAGAIN && !off) break;                            // (no merges to be had: the lanes below, nothing is done yet)
			if (r) return r == -EAGAIN ? -EIO : r;
			run_crc = gf2_mul32(run_crc, crc_shift_op(len)) ^ ck;
			run_adler = adler_join(run_adler, ak, len);
			pos += got; off += len;
		}
		if (off == src_len) {
			*out_len = pos;
			if (crc) *crc = run_crc;
			if (adler) *adler = run_adler;
			return 0;
		}
	}
	int pair = -1;
	for (int k = 0; k < HOST_PAIRS && pair < 0; k++) if (c->lanes_mtx[k].try_lock()) pair = k;
	if (pair < 0) { pair = (int)(c->lanes_turn.fetch_add(1) % HOST_PAIRS); c->lanes_mtx[pair].lock(); }
	std::lock_guard<std::mutex> g(c->lanes_mtx[pair], std::adopt_lock);
	nxz_ctx::HostLane *const lanes = c->lanes + 2 * pair;
	const size_t nblk = (src_len + B - 1) / B;
	// groups: at least four when the input allows it, so that copies and kernels overlap
	size_t group = std::min<size_t>(HOST_GROUP - 1, std::max<size_t>(31, (nblk + 3) / 4));   // (- 1: the window in front of a group's first block)
	const size_t ngroups = (nblk + group - 1) / group;
	group = (nblk + ngroups - 1) / ngroups;
	for (int k = 0; k < 2; k++)
		if (!lane_need(lanes[k], k == 1, group + 1)) return -ENOMEM;
	const uint32_t op_block = crc_shift_op(B);
	uint32_t run_crc = 0, run_adler = 1;
	size_t pos = 0;
	int rc = 0;

	auto queue = [&](size_t gi) -> int {
		nxz_ctx::HostLane &l = lanes[gi & 1];
		const size_t b0 = gi * group, n = std::min(group, nblk - b0);
		const uint64_t first = (uint64_t)b0 * B;                      // offset of the group's first block in src
		const uint64_t bytes = std::min<uint64_t>((uint64_t)n * B, src_len - first);
		// the window in front of the group: from src itself, for the call's first block from `prev`
		const uint32_t h0 = !H ? 0 : first ? (uint32_t)std::min<uint64_t>(H, first) & ~15u : (uint32_t)std::min<size_t>(H, prev_len) & ~15u;
		for (size_t k = 0; k < n; k++) {
			nxz_batch_job_t &j = l.h_jobs[k];
			memset(&j, 0, sizeof(j));
			const uint32_t hk = (uint32_t)std::min<uint64_t>(H, h0 + (uint64_t)k * B);   // (a multiple of 16: h0, B and H are)
			j.src = l.d_src + h0 + k * B - hk; j.dst = l.d_dst + k * HOST_SLOT;
			j.hist_len = hk;
			j.src_len = hk + (uint32_t)std::min<uint64_t>(B, bytes - (uint64_t)k * B);
			j.dst_cap = HOST_SLOT; j.in_crc = 0; j.in_adler = 1;
		}
		l.n = n; l.bytes = bytes;
		HIPCHK(hipMemcpyAsync(l.d_jobs, l.h_jobs, n * sizeof(nxz_batch_job_t), hipMemcpyHostToDevice, l.stream), return -EIO);
		const uint8_t *from = src + first - (first ? h0 : 0);
		const size_t from_bytes = bytes + (first ? h0 : 0), at = first ? 0 : h0;
		if (l.h_src) {                                                // the window and the blocks through the lane's pinned staging: one copy
			if (at) memcpy(l.h_src, prev + prev_len - h0, h0);
			memcpy(l.h_src + at, from, from_bytes);
			HIPCHK(hipMemcpyAsync(l.d_src, l.h_src, at + from_bytes, hipMemcpyHostToDevice, l.stream), return -EIO);
		} else {
			if (at) { HIPCHK(hipMemcpyAsync(l.d_src, prev + prev_len - h0, h0, hipMemcpyHostToDevice, l.stream), return -EIO); }
			HIPCHK(hipMemcpyAsync(l.d_src + at, from, from_bytes, hipMemcpyHostToDevice, l.stream), return -EIO);
		}
		int r = nxz_batch_compress(c, fc, l.d_jobs, n, nullptr, 0, l.d_res, nullptr, l.stream);
		if (r) return r;
		const uint32_t fin = final && gi == ngroups - 1 ? (uint32_t)(n - 1) : 0xffffffffu;
		if (nxz_launch_pack_stream(l.d_jobs, l.d_res, n, fin, l.d_off, l.d_packed, l.stream)) return -EIO;
		HIPCHK(hipMemcpyAsync(l.h_res, l.d_res, n * sizeof(nxz_batch_result_t), hipMemcpyDeviceToHost, l.stream), return -EIO);
		HIPCHK(hipMemcpyAsync(l.h_total, l.d_off + n, sizeof(uint64_t), hipMemcpyDeviceToHost, l.stream), return -EIO);
		return 0;
	};
	auto collect = [&](size_t gi) -> int {
		nxz_ctx::HostLane &l = lanes[gi & 1];
		HIPCHK(hipStreamSynchronize(l.stream), return -EIO);
		const uint64_t total = *l.h_total;
		if (pos + total > dst_cap) return -E2BIG;                   // cannot happen: the bound was checked
		HIPCHK(hipMemcpyAsync(l.h_packed ? l.h_packed : dst + pos, l.d_packed, total, hipMemcpyDeviceToHost, l.stream), return -EIO);
		for (size_t k = 0; k < l.n; k++) {                           // meanwhile: checksums of the run
			const uint32_t len = l.h_jobs[k].src_len - l.h_jobs[k].hist_len;
			const uint32_t op = len == B ? op_block : crc_shift_op(len);
			run_crc = gf2_mul32(run_crc, op) ^ l.h_res[k].crc;
			run_adler = adler_join(run_adler, l.h_res[k].adler, len);
		}
		HIPCHK(hipStreamSynchronize(l.stream), return -EIO);
		if (l.h_packed) memcpy(dst + pos, l.h_packed, total);
		pos += total;
		return 0;
	};
	size_t queued = 0, done = 0;
	static const bool htrace = getenv("NXZ_API_TRACE") != nullptr;
	uint64_t tq = 0, tc = 0, t_ = 0;
	auto tick = [&]() { return htrace ? trace_ns() : 0; };
	while (!rc && queued < ngroups && queued < 2) { t_ = tick(); rc = queue(queued++); tq += tick() - t_; }
	while (!rc && done < queued) {
		t_ = tick(); rc = collect(done++); tc += tick() - t_;
		if (!rc && queued < ngroups) { t_ = tick(); rc = queue(queued++); tq += tick() - t_; }
	}
	if (htrace && src_len >= (64u << 20))
		fprintf(stderr, "nxz_deflate_host: %zu bytes in %zu groups on lanes %d/%d: %.2f ms queueing (copies in, launches), %.2f ms collecting (waits, copies out)\n",
			src_len, ngroups, 2 * pair, 2 * pair + 1, tq * 1e-6, tc * 1e-6);
	if (rc) {
		for (int k = 0; k < 2; k++) (void)hipStreamSynchronize(lanes[k].stream);
		return rc;
	}
	*out_len = pos;
	if (crc) *crc = run_crc;
	if (adler) *adler = run_adler;
	return 0;
}
