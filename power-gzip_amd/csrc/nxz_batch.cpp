// nxz_batch.cpp -- the batched, device-resident interface of include/nxz_engine.h: the compress and inflate batches and which
// kernels they get, their dictionary, framed and BGZF forms, table generation, wrap and the pack forms, and the diagnostics.
#include "nxz_ctx.h"
#include "nxz_streams.h"

// ---------------------------------------------------------------------------
// batched, device-resident interface
// ---------------------------------------------------------------------------
// Jobs per launch of the three compress kernels: bounds the token scratch (104 KiB per job: 832 MiB for 8192
// jobs, 6.6 GiB for 65536).  Larger chunks cost memory, smaller ones time: the LZ77 kernel is one persistent
// workgroup per CU, at the end of a launch CUs idle until the last job is done, and every chunk is three launches
// (the corpus, 262144 jobs: 92.8 GiB/s at 8192 jobs per launch, 94.7 at 16384, 95.8 at 32768, 96.4 at 65536).  So the
// chunk grows with the batch -- a quarter to an eighth of it, 8192 at least and 65536 at most: a caller with a few thousand jobs
// never pays gigabytes for them -- and falls back to 8192 when the device has no room for more.
// NXZ_COMPRESS_CHUNK fixes it.
static size_t compress_chunk(size_t n)
{
	static const size_t v = [] { const char *e = getenv("NXZ_COMPRESS_CHUNK"); size_t x = e ? (size_t)strtoull(e, nullptr, 0) : 0; return x >= 256 ? x : (size_t)0; }();
	if (v) return v;
	size_t c = 8192;
	while (c < 65536 && n >= 8 * c) c *= 2;
	return c;
}

static constexpr unsigned JOB_COUNTERS = 256;
// Which inflate kernel a batch gets (profiles/r01c_inflate_by_batch_size.txt, 64 KiB streams):
//   up to NXZ_WINDOW_LDS_MAX streams   a stream per wave, window in LDS (4 per CU): 3.7-4.4 ms a round
//   below NXZ_LANES_MIN streams        a stream per wave, the target as window (20 per CU): 7.5 ms for
//                                      4096 streams, 40 GiB/s at 65 536
//   from NXZ_LANES_MIN streams on      a stream per lane: 55-60 ms however few streams, 51 GiB/s at 65 536,
//                                      110 at 262 144
// The wave kernels need 16-byte aligned sources, as the batch interface demands.
// Round 3 (profiles/r03_inflate_by_batch_size.txt): the lane kernel wins only on streams of fixed-Huffman (or stored)
// blocks -- one table for all lanes -- from about 100 000 streams on (91 against 44 GiB/s at 262 144); streams that
// bring a table each (zlib's, the engine's own exact-table output) run twice as fast a stream per wave at every batch
// size (81 against 40).  So a batch of NXZ_LANES_MIN streams or more is sampled first: 256 of its streams, the type
// of their first block.
// Round 4 (profiles/r04c_inflate_by_batch_size.txt): with its memory instructions issued where all lanes pass together
// the lane kernel does fixed-code streams at 36 GiB/s at 16 384 streams, 62 at 32 768, 105 at 65 536, 154 at 131 072
// (a stream per wave: 38, 42, 43, 44); streams with tables of their own are still the wave kernel's at every size.
// ... on the bench's synthetic blocks (ratio 1.75, a token every 2.3 bytes).  The corpus' blocks as fixed-code streams (ratio
// 2.9) go through the wave kernel at 73 GiB/s from 32 768 streams on and through the lane kernel at 51 / 88 / 164 at 32 768 /
// 65 536 / 262 144: the switch-over lies between the two kinds' break-evens.
#define NXZ_LANES_MIN 49152
#define NXZ_LANES_TABLES_MIN 163840   /* streams that bring tables: the lane kernel from here on */
#define NXZ_WINDOW_LDS_MAX 1024
#define NXZ_DICT_WG_MIN_DEFAULT 4096    /* nxz_batch_decompress_dict: source bytes from which a stream goes a workgroup each (profiles/r08_dict.txt: the two routes break even at about 4 KiB of source, 10 KiB of output) */

extern "C" int nxz_dict_create(nxz_ctx_t *c, const uint8_t *bytes, size_t len, nxz_dict_t **out)
{
	if (!c || !out || (len && !bytes)) return -EINVAL;
	if (forked_child()) return -ENODEV;
	(void)hipSetDevice(c->device);
	nxz_dict *d = new (std::nothrow) nxz_dict;
	if (!d) return -ENOMEM;
	d->device = c->device; d->len = len;
	d->id = nxz_dict_adler32(bytes, len);
	d->win = nxz_dict_inflate_window(len); d->W = nxz_dict_deflate_window(len);
	std::vector<uint8_t> img(NXZ_DICT_WINDOW, 0);
	if (d->win) memcpy(img.data() + NXZ_DICT_WINDOW - d->win, bytes + nxz_dict_inflate_start(len), d->win);
	if (hipMalloc((void **)&d->d_win, NXZ_DICT_WINDOW) != hipSuccess) { (void)hipGetLastError(); delete d; return -ENOMEM; }
	hipError_t e = hipMemcpy(d->d_win, img.data(), NXZ_DICT_WINDOW, hipMemcpyHostToDevice);
	if (e != hipSuccess) { set_err("dictionary copy", e); (void)hipFree(d->d_win); delete d; return -EIO; }
	*out = d;
	return 0;
}
extern "C" void nxz_dict_destroy(nxz_ctx_t *c, nxz_dict_t *d)
{
	if (!d) return;
	if (!forked_child()) { (void)hipSetDevice(d->device); (void)hipFree(d->d_win); }
	delete d;
}
extern "C" uint32_t nxz_dict_id(const nxz_dict_t *d) { return d ? d->id : 1; }

// The compress function codes: LZ77 kernel (tokens, counts, checksums) -> [table generator] ->
// entropy kernel, chunk after chunk on the caller's stream.
static int batch_compress(nxz_ctx_t *c, int fc, const nxz_batch_job_t *jobs, size_t n,
			  const nxz_batch_dht_t *dht, size_t ntables, nxz_batch_result_t *results,
			  uint32_t *counts, void *stream, const nxz_dict *dict);
extern "C" int nxz_batch_compress(nxz_ctx_t *c, int fc, const nxz_batch_job_t *jobs, size_t n,
				  const nxz_batch_dht_t *dht, size_t ntables, nxz_batch_result_t *results,
				  uint32_t *counts, void *stream)
{
	return batch_compress(c, fc, jobs, n, dht, ntables, results, counts, stream, nullptr);
}
// ... with one dictionary as every job's window: the kernels get the caller's jobs rewritten on the device (nxz_launch_dict_jobs:
// 48 bytes a job of per-stream scratch, no copy of the window), the LZ77 kernel's load phase takes the window from the dictionary
extern "C" int nxz_batch_compress_dict(nxz_ctx_t *c, int fc, const nxz_dict_t *dict, const nxz_batch_job_t *jobs, size_t n,
				       const nxz_batch_dht_t *dht, size_t ntables, nxz_batch_result_t *results,
				       uint32_t *counts, void *stream)
{
	if (!c || !dict || dict->device != c->device || n >= (1u << 31) || (n && (!jobs || !results))) return -EINVAL;
	return batch_compress(c, fc, jobs, n, dht, ntables, results, counts, stream, dict);
}
static int batch_compress(nxz_ctx_t *c, int fc, const nxz_batch_job_t *ujobs, size_t n,
			  const nxz_batch_dht_t *dht, size_t ntables, nxz_batch_result_t *results,
			  uint32_t *counts, void *stream, const nxz_dict *dict)
{
	const nxz_batch_job_t *jobs = ujobs;
	if (!c || !nxz_fc_is_compress((uint32_t)fc) || (fc & 1) || (fc & ~0x2e)) return -EINVAL;
	if (forked_child()) return -ENODEV;
	const bool gen = nxz_fc_is_dhtgen((uint32_t)fc);
	const bool isdht = nxz_fc_is_dht((uint32_t)fc), count = nxz_fc_has_count((uint32_t)fc);
	if (gen && !isdht) return -EINVAL;
	if (count && !counts) return -EINVAL;
	if (isdht && !gen && (!dht || !ntables)) return -EINVAL;
	if (n == 0) return 0;
	hipStream_t s = (hipStream_t)stream;   // NULL = the HIP default stream
	(void)hipSetDevice(c->device);
	nxz_dht_prepared_t *prepared = nullptr;
	// equal chunks (a last chunk of a few jobs would cost three launches for nothing)
	// the fixed code without counts: the LZ77 kernel writes the finished block itself (no tokens in device scratch,
	// no entropy launch, and so no reason to cut the batch into chunks: one launch, one tail)
	// ... and so it can for the additive DHTGEN function codes (round 5, NXZ_FUSED_GEN=1): the table of a block is made, and the block
	// encoded, inside the LZ77 kernel, a job behind the parse (nxz_lz77.hip gen::) -- one launch, 110 MB of scratch whatever the batch
	// instead of 104 KiB a job of a chunk.  Not the default: 75.7 against 103.1 GiB/s on the corpus (profiles/r05_fused_dhtgen.txt) -- the
	// table generator is a chain of dependent steps that ONE wavefront works through while fifteen wait at their barriers, where the
	// kernel of nxz_dhtgen.hip has thirty tables in flight on a CU and hides every one's latency behind the others'.
	const char *fge = getenv("NXZ_FUSED_GEN");                        // (read at every call: the tests switch it)
	const bool fused_gen_on = fge && atoi(fge) != 0;
	const bool fused_gen = gen && fused_gen_on;
	const bool fused = (!isdht && !count) || fused_gen;
	size_t want = compress_chunk(n);
	size_t nchunks = fused ? 1 : (n + want - 1) / want;
	size_t chunk = (n + nchunks - 1) / nchunks;
	nxz_ctx::Scratch sc;
	// One call at a time per stream from sizing to the last launch (lease_scratch; round 2's advisor finding)
	const auto use = lease_scratch(c, s);
	const int sized = with_scratch(c, s, [&](nxz_ctx::Scratch &r) -> int {
		if (!fused && r.chunk_limit && want > r.chunk_limit) {
			// a larger chunk could not be had on this device a call ago: not tried again before nxz_trim()
			want = r.chunk_limit; nchunks = (n + want - 1) / want; chunk = (n + nchunks - 1) / nchunks;
		}
		if (!fused && r.chunk_cap < chunk) {
			// grows only: warm up once with the largest batch before timing a loop.  The scratch of a chunk (104 KiB of
			// tokens + a table + the counts per job) takes no more than a quarter of what the device has free right now.
			if (r.d_tokens) { (void)hipStreamSynchronize(s); r.release_chunk(); }
			const size_t per_job = (size_t)NXZ_TOK_STRIDE + sizeof(nxz_dht_prepared_t) + 316 * sizeof(uint32_t);
			size_t free_b = 0, total_b = 0;
			if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && want > 8192 && chunk * per_job > free_b / 4) {
				while (want > 8192 && want * per_job > free_b / 4) want /= 2;
				nchunks = (n + want - 1) / want; chunk = (n + nchunks - 1) / nchunks;
				r.chunk_limit = want;
			}
			while (!r.alloc_chunk(chunk)) {
				if (want <= 1024) return -ENOMEM;
				want = want > 8192 ? 8192 : want / 2;          // no room for the large chunk: the small one, then halves of it
				nchunks = (n + want - 1) / want; chunk = (n + nchunks - 1) / nchunks;
				r.chunk_limit = want;
			}
		}
		if (!r.d_cand2) HIPCHK(hipMalloc((void **)&r.d_cand2, nxz_lz77_cand2_bytes()), return -ENOMEM);
		if (fused_gen && !r.d_fuse) HIPCHK(hipMalloc((void **)&r.d_fuse, nxz_lz77_gen_scratch_bytes()), return -ENOMEM);
		if (isdht && !gen && r.buf[BUF_PREPARED].grow(s, ntables * sizeof(nxz_dht_prepared_t)) == DevBuf::FAILED) return -ENOMEM;
		if (!c->d_job_counters && hipMalloc((void **)&c->d_job_counters, JOB_COUNTERS * sizeof(uint32_t)) != hipSuccess) c->d_job_counters = nullptr;
		if (dict && r.buf[BUF_DICT_JOBS].grow(s, n * sizeof(nxz_batch_job_t)) == DevBuf::FAILED) return -ENOMEM;
		sc = r;
		return 0;
	});
	if (sized) return sized;
	if (dict) {
		nxz_batch_job_t *djobs = sc.buf[BUF_DICT_JOBS].as<nxz_batch_job_t>();
		int rc = nxz_launch_dict_jobs(ujobs, n, dict->W, djobs, s);
		if (rc) { set_err("dictionary jobs launch", (hipError_t)rc); return -EIO; }
		jobs = djobs;
	}
	if (isdht && !gen) {
		prepared = sc.buf[BUF_PREPARED].as<nxz_dht_prepared_t>();
		int rc = nxz_launch_dht_prepare(dht, ntables, prepared, s);
		if (rc) { set_err("dht prepare launch", (hipError_t)rc); return -EIO; }
	}
	for (size_t off = 0; off < n; off += chunk) {
		const size_t m = n - off < chunk ? n - off : chunk;
		uint32_t *jc = nullptr;
		{
			std::lock_guard<std::mutex> g(c->mtx);
			if (c->d_job_counters) jc = c->d_job_counters + (c->next_counter++ % JOB_COUNTERS);
		}
		uint32_t *cnt = count ? counts + off * 316 : gen ? sc.d_counts : nullptr;
		auto stamp = [&]() {
			if (!c->timing) return;
			hipEvent_t e;
			if (hipEventCreate(&e) != hipSuccess) return;
			(void)hipEventRecord(e, s);
			std::lock_guard<std::mutex> g(c->mtx);
			c->tev.push_back(e);
		};
		stamp();
		// (the fused dynamic form makes its table inside the kernel: its own scratch, and counts only for the caller who asked)
		const int mode = fused_gen ? NXZ_LZ77_FUSED_GEN : fused ? NXZ_LZ77_FUSED_FHT : cnt != nullptr;
		uint8_t *const lz_scratch = fused_gen ? sc.d_fuse : sc.d_tokens;
		uint32_t *const lz_counts = fused_gen && !count ? nullptr : cnt;
		int rc = dict ? nxz_launch_lz77_dict(mode, jobs + off, m, lz_scratch, sc.d_cand2, results + off, lz_counts, jc, dict->deflate_window(), s)
			      : nxz_launch_lz77(mode, jobs + off, m, lz_scratch, sc.d_cand2, results + off, lz_counts, jc, s);
		if (rc) { set_err("lz77 launch", (hipError_t)rc); return -EIO; }
		stamp();
		if (fused) { stamp(); stamp(); continue; }
		if (gen) {
			rc = nxz_launch_dhtgen(cnt, m, sc.d_gen, nullptr, s);
			if (rc) { set_err("dhtgen launch", (hipError_t)rc); return -EIO; }
		}
		stamp();
		rc = nxz_launch_encode(isdht, gen, jobs + off, m, sc.d_tokens, gen ? sc.d_gen : prepared, results + off, s);
		if (rc) { set_err("encode launch", (hipError_t)rc); return -EIO; }
		stamp();
	}
	if (dict) {
		int rc = nxz_launch_dict_finish(ujobs, n, dict->W, results, s);
		if (rc) { set_err("dictionary finish launch", (hipError_t)rc); return -EIO; }
	}
	return 0;
}

// nxz_trim(): the token scratch of every stream no batch call is working on goes back to the device (a chunk of 65536 jobs
// is 6.6 GiB), and a remembered "no room for more than N jobs a chunk" is forgotten.  Returns the bytes freed.
size_t trim_compress_scratch()
{
	size_t freed = 0;
	std::lock_guard<std::mutex> g(g_mtx);
	for (nxz_ctx *c : g_ctx) {
		if (!c) continue;
		(void)hipSetDevice(c->device);
		std::vector<std::pair<hipStream_t, std::mutex *>> streams;
		{
			std::lock_guard<std::mutex> g2(c->mtx);
			for (auto &kv : c->scratch) streams.emplace_back(kv.first, &c->scratch_use[kv.first]);
		}
		for (auto &sm : streams) {
			if (!sm.second->try_lock()) continue;              // a call is sizing or launching on that stream
			// (a stream the caller has destroyed meanwhile -- nxz_stream_destroy drops its entry, a stream of the caller's own may be gone
			// without a word: a failed wait means "leave it alone")
			bool there;
			{
				std::lock_guard<std::mutex> g2(c->mtx);
				there = c->scratch.find(sm.first) != c->scratch.end();
			}
			if (there && hipStreamSynchronize(sm.first) != hipSuccess) { (void)hipGetLastError(); there = false; }
			if (there) {
				std::lock_guard<std::mutex> g2(c->mtx);
				auto it = c->scratch.find(sm.first);               // (find, not []: an entry that went away in between stays away)
				if (it != c->scratch.end()) {
					nxz_ctx::Scratch &r = it->second;
					if (r.d_tokens) freed += r.chunk_cap * ((size_t)NXZ_TOK_STRIDE + sizeof(nxz_dht_prepared_t) + 316 * sizeof(uint32_t));
					r.release_chunk();
					r.chunk_limit = 0;
				}
			}
			sm.second->unlock();
		}
	}
	return freed;
}

// Measurement aid: with timing on, every compress batch records events around its kernels;
// nxz_ctx_stage_ms waits for them and returns the milliseconds spent in the LZ77, dhtgen and
// entropy kernels since the last call (and the number of launches of each).
extern "C" void nxz_ctx_stage_timing(nxz_ctx_t *c, int on)
{
	if (!c) return;
	std::lock_guard<std::mutex> g(c->mtx);
	c->timing = on != 0;
}

extern "C" int nxz_ctx_stage_ms(nxz_ctx_t *c, double ms[3], unsigned *launches)
{
	if (!c || !ms) return -EINVAL;
	std::vector<hipEvent_t> ev;
	{
		std::lock_guard<std::mutex> g(c->mtx);
		ev.swap(c->tev);
	}
	ms[0] = ms[1] = ms[2] = 0;
	if (launches) *launches = (unsigned)(ev.size() / 4);
	for (size_t i = 0; i + 3 < ev.size(); i += 4) {
		(void)hipEventSynchronize(ev[i + 3]);
		for (int k = 0; k < 3; k++) {
			float f = 0;
			if (hipEventElapsedTime(&f, ev[i + k], ev[i + k + 1]) == hipSuccess) ms[k] += f;
		}
	}
	for (auto e : ev) (void)hipEventDestroy(e);
	return 0;
}

// The reference's dhtgen() (lib/nx_dhtgen.c:945-1034) for a batch of count arrays on the device.
extern "C" int nxz_batch_dhtgen(nxz_ctx_t *c, const uint32_t *counts, size_t n, nxz_batch_dht_t *tables, void *stream)
{
	if (!c || !counts || !tables) return -EINVAL;
	if (forked_child()) return -ENODEV;
	(void)hipSetDevice(c->device);
	int rc = nxz_launch_dhtgen(counts, n, nullptr, tables, (hipStream_t)stream);
	if (rc) { set_err("dhtgen launch", (hipError_t)rc); return -EIO; }
	return 0;
}

// force: 0 -- the kernel by the batch's size and kind; 1 -- a stream per lane, any block type; 2 -- a stream per wavefront
static int batch_decompress(nxz_ctx_t *c, const nxz_batch_job_t *jobs, size_t n, nxz_batch_result_t *results, nxz_batch_dht_t *dht_io, void *stream, int force);
extern "C" int nxz_batch_decompress(nxz_ctx_t *c, const nxz_batch_job_t *jobs, size_t n,
				    nxz_batch_result_t *results, nxz_batch_dht_t *dht_io, void *stream)
{
	return batch_decompress(c, jobs, n, results, dht_io, stream, 0);
}
// The block-type sample of a large inflate batch (nxz_launch_sample_btype on 256 of its streams; one small launch and a wait for
// it: nothing next to the tens of milliseconds such a batch takes).  true: h[0] the sampled streams whose first block brings a
// table, h[1] and h[2] the shortest and the longest source among the sampled; false: no sample to be had.
static bool sample_btype(nxz_ctx *c, const nxz_batch_job_t *jobs, size_t n, hipStream_t s, uint32_t h[3])
{
	uint32_t *w = nullptr;
	{
		std::lock_guard<std::mutex> g(c->mtx);
		if (!c->h_sample) (void)hipHostMalloc((void **)&c->h_sample, 64 * sizeof(uint32_t));
		w = c->h_sample ? c->h_sample + 4 * (c->sample_turn++ & 15) : nullptr;
	}
	if (!w) return false;
	w[0] = 0; w[1] = 0; w[2] = 0;
	if (nxz_launch_sample_btype(jobs, n, w, s) != 0 || hipStreamSynchronize(s) != hipSuccess) return false;
	h[0] = w[0]; h[1] = w[1]; h[2] = w[2];
	return true;
}

// The workspace of the workgroup-per-stream kernels for n streams on `s`, and from 128 streams on the order workspace (NULL: none
// to be had, the streams go as they come).  The caller holds the lease.
static int wg_workspaces(nxz_ctx *c, hipStream_t s, size_t n, uint8_t **wws, uint8_t **ows)
{
	return with_scratch(c, s, [&](nxz_ctx::Scratch &sc) -> int {
		const size_t oneed = n >= 128 ? nxz_order_workspace(n) : 0;
		if (sc.buf[BUF_WG].grow(s, nxz_inflate_wg_workspace(n)) == DevBuf::FAILED) return -ENOMEM;
		*wws = sc.buf[BUF_WG].p;
		*ows = oneed && sc.buf[BUF_ORDER].grow(s, oneed) != DevBuf::FAILED ? sc.buf[BUF_ORDER].p : nullptr;
		return 0;
	});
}

static int batch_decompress(nxz_ctx_t *c, const nxz_batch_job_t *jobs, size_t n, nxz_batch_result_t *results, nxz_batch_dht_t *dht_io, void *stream, int force)
{
	if (!c) return -EINVAL;
	if (forked_child()) return -ENODEV;
	(void)hipSetDevice(c->device);         // scratch is allocated on, and kernels go to, the context's device
	hipStream_t s = (hipStream_t)stream;   // NULL = the HIP default stream
	int rc;
	const char *lm = getenv("NXZ_INFLATE_LANES_MIN");                    // tuning / test knob
	const size_t lanes_min = lm ? (size_t)strtoull(lm, nullptr, 0) : (size_t)NXZ_LANES_MIN;
	bool lanes = force ? (force & 3) == 1 : n >= lanes_min, by_len = (force & 4) != 0, no_tables = false;
	bool split = false;
	// A stream per WORKGROUP, source, output and tables in LDS (nxz_inflate_wg.hip): every batch, unless one of the older routes' knobs
	// is set (the tests' way to name a route) -- except, from 98 304 streams on, the batches whose sampled streams begin with fixed-code
	// or stored blocks (the fixed-code lane kernel's: 158-177 GiB/s against 151).  That kernel runs at one rate from a few thousand
	// streams on (a CU a stream; profiles/r06_inflate_by_batch_size.txt: zlib -6 streams of the corpus 96-99 GiB/s from 4096 streams on,
	// own exact-table streams 115-120, fixed-code synthetic blocks 144-151), where a stream per wavefront needs 16 384 streams for 56
	// and levels off at 66, and a stream per lane needs 100 000 (zlib -6 streams at 262 144, both older kernels side by side: 87).
	// Streams of any length are its own (in spans, the output flushed in halves); what it does not do -- streams that resume or bring
	// a history, end early or are damaged -- it hands back, and those go a stream per wavefront behind it.
	// NXZ_INFLATE_WG=0 / 1: never / always; NXZ_INFLATE_WG_MAX: batches up to that size only.
	const char *wge = getenv("NXZ_INFLATE_WG");                         // (read at every call: the tests switch it)
	const char *wgm = getenv("NXZ_INFLATE_WG_MAX");
	const size_t wg_max = wgm ? (size_t)strtoull(wgm, nullptr, 0) : ~(size_t)0;
	bool wg = !force && (wge ? atoi(wge) != 0 : (!lm && !getenv("NXZ_INFLATE_CUT") && n <= wg_max));
	if (wg && !wge && n >= 98304) {
		// (the sample the older routes take below: here only "do these streams bring tables?")
		uint32_t h[3];
		if (sample_btype(c, jobs, n, s, h) && h[0] <= 16) wg = false;
	}
	if (wg) {
		const auto use = lease_scratch(c, s);
		uint8_t *wws = nullptr, *ows = nullptr;
		if ((rc = wg_workspaces(c, s, n, &wws, &ows)) != 0) return rc;
		const uint32_t *order = ows ? nxz_launch_order_by_length(jobs, n, ows, s) : nullptr;   // (a workgroup draws stream after stream: the long ones first)
		rc = nxz_launch_inflate_wg(jobs, n, results, dht_io, wws, order, nullptr, s);
		if (rc) { set_err("inflate launch", (hipError_t)rc); return -EIO; }
		return 0;
	}
	if (lanes && !lm && !force) {
		// what kind of streams?
		uint32_t h[3];
		if (sample_btype(c, jobs, n, s, h)) {
			// a quarter or more with tables: the wave kernel's, unless the batch is so large that the general lane kernel
			// overtakes it (zlib -6 streams of the corpus: 75 against 86 GiB/s at 131 072 streams, 95 against 86 at 196 608, 102 at
			// 262 144, 117 at 524 288; profiles/r04c_inflate_by_batch_size.txt)
			if (h[0] > 64 && n < NXZ_LANES_TABLES_MIN) lanes = false;
			// ... and from there on BOTH, side by side on two HIP streams, each on its share of the batch (NXZ_INFLATE_SPLIT_PCT: the
			// wavefront kernel's share, 40; 0: the lane kernel alone, as up to round 5): the lane kernel waits for memory three quarters
			// of its time, the wavefront kernel is bound by what it issues -- 262 548 zlib -6 streams of the corpus 81.6 -> 84.4 GiB/s,
			// of the round-4 classes 97.4 -> 110
			else if (h[0] > 64 && n >= NXZ_LANES_TABLES_MIN) split = true;
			// streams of very different lengths (zeros beside text: BASELINE configs[4]): a wavefront takes as long as its
			// longest stream, so the lane kernel gets them ordered by length; much of a size they stay as they come
			// (neighbours in memory: ordering the bench's synthetic blocks cost 5 %)
			by_len = h[2] > 8 * (uint64_t)h[1] + 4096;
			// few of the sampled streams begin with a dynamic block: the fixed-code-only lane kernel first, which hands the
			// streams it cannot do -- those, and any with a dynamic block further in -- to the general one, stream by stream
			no_tables = h[0] <= 16;
		}
	}
	static const int split_pct = getenv("NXZ_INFLATE_SPLIT_PCT") ? atoi(getenv("NXZ_INFLATE_SPLIT_PCT")) : 40;
	if (split && split_pct > 0 && split_pct < 100) {
		{
			std::lock_guard<std::mutex> g(c->mtx);
			if (!c->split_stream) {
				if (stream_create_spread(&c->split_stream, 1) != hipSuccess || hipEventCreateWithFlags(&c->split_ev[0], hipEventDisableTiming) != hipSuccess ||
				    hipEventCreateWithFlags(&c->split_ev[1], hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); c->split_stream = nullptr; }
			}
		}
		if (c->split_stream) {
			std::lock_guard<std::mutex> one(c->split_mtx);              // (one split batch at a time: the second stream and the events are the context's)
			const size_t k = ((n * (size_t)(100 - split_pct) / 100) + 63) & ~(size_t)63;
			if (k > 0 && k < n) {
				HIPCHK(hipEventRecord(c->split_ev[0], s), return -EIO);
				HIPCHK(hipStreamWaitEvent(c->split_stream, c->split_ev[0], 0), return -EIO);
				const int r2 = batch_decompress(c, jobs + k, n - k, results + k, dht_io ? dht_io + k : nullptr, c->split_stream, 2);
				const int r1 = batch_decompress(c, jobs, k, results, dht_io, s, 1 | (by_len ? 4 : 0));
				HIPCHK(hipEventRecord(c->split_ev[1], c->split_stream), return -EIO);
				HIPCHK(hipStreamWaitEvent(s, c->split_ev[1], 0), return -EIO);
				return r1 ? r1 : r2;
			}
		}
	}
	if (lanes) {
		// many streams: one stream per lane (nxz_inflate_lanes.hip); the table workspace is made once
		const auto use = lease_scratch(c, s);
		uint8_t *ws = nullptr;
		// grows only (3.6 KiB per lane in flight, 0.9 GiB for the largest grid); a new workspace has its tables made again
		const DevBuf::Grown grown = with_scratch(c, s, [&](nxz_ctx::Scratch &sc) {
			const DevBuf::Grown g = sc.buf[BUF_LANES].grow(s, nxz_inflate_lanes_workspace(n));
			ws = sc.buf[BUF_LANES].p;
			return g;
		});
		if (grown == DevBuf::FAILED) return -ENOMEM;
		const int init = grown == DevBuf::NEW;
		rc = nxz_launch_inflate_lanes(jobs, n, results, dht_io, ws, init | (by_len ? 2 : 0) | (no_tables ? 4 : 0), s);
	} else if ([&]() -> bool {
		// A batch that does not fill the device a stream per wavefront (5120 at a time, each as slow as 20-100 MB/s): every stream
		// is cut inside its first block and the pieces go side by side (nxz_inflate_cut.hip; zlib -6 streams of the corpus, 4096
		// of them: 28.6 GiB/s a stream per wavefront).  NXZ_INFLATE_CUT=0 / 1: never / whenever two pieces a stream are allowed.
		const char *ce = getenv("NXZ_INFLATE_CUT");
		const int cut_env = ce ? atoi(ce) : -1;
		if (cut_env == 0) return false;
		unsigned P = nxz_inflate_cut_pieces(n);
		// (left to itself: batches of 64 streams at most, where a call takes as long as its slowest stream and
		// the pieces of all of them are resident at once; larger ones lose more to the rounds -- each as long as ITS
		// slowest piece -- than the cuts win: profiles/r05_inflate_cut_by_batch_size.txt)
		static const size_t auto_max = getenv("NXZ_INFLATE_CUT_MAX") ? (size_t)strtoull(getenv("NXZ_INFLATE_CUT_MAX"), nullptr, 0) : 64;
		if (cut_env < 0 && (P < 4 || n > auto_max)) return false;
		if (P < 2) { if (cut_env <= 0) return false; P = 2; }
		// room for the pieces' 16-bit elements: half a megabyte a stream, a quarter of what the device has free at most
		size_t arena = n * ((size_t)512 << 10), free_b = 0, total_b = 0;
		if (arena < ((size_t)256 << 20)) arena = (size_t)256 << 20;
		if (arena > ((size_t)8 << 30)) arena = (size_t)8 << 30;
		const auto use = lease_scratch(c, s);
		uint8_t *ws = nullptr;
		if (!with_scratch(c, s, [&](nxz_ctx::Scratch &sc) {
			DevBuf &b = sc.buf[BUF_CUT];
			size_t need = nxz_inflate_cut_workspace(n, P, arena);
			if (b.cap < need) {
				b.drop(s);                                                 // (first: what it held counts as free below)
				if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && arena > free_b / 4) { arena = free_b / 4; need = nxz_inflate_cut_workspace(n, P, arena); }
				if (arena < ((size_t)16 << 20) || b.grow(s, need) == DevBuf::FAILED) return false;
			} else arena += b.cap - need;                                  // (what a larger batch left: the arena takes it)
			ws = b.p;
			return true;
		})) return false;
		rc = nxz_launch_inflate_cut(jobs, n, results, dht_io, P, ws, arena, s);
		return true;
	}()) {
	} else {
		const char *wm = getenv("NXZ_INFLATE_LDS_MAX");                 // tuning / test knob
		const size_t lds_max = wm ? (size_t)strtoull(wm, nullptr, 0) : (size_t)NXZ_WINDOW_LDS_MAX;
		// A launch ends with its slowest stream, and the corpus' slowest block takes a wavefront 8 ms where the average takes 4:
		// the long ones start first -- the jobs' indices by falling source length (zlib -6 streams of the corpus: 53.9 -> 77.1
		// GiB/s at 16 384 streams, 67.4 -> 85.0 at 32 768, 83.1 -> 86.5 at 262 144, 26.1 -> 28.5 at 4096 where all are resident
		// at once; profiles/r04c_inflate_by_batch_size.txt).  Not for the few streams that get the window in LDS.
		// (NXZ_INFLATE_ORDER=0 / 1: never / always)
		const uint32_t *order = nullptr;
		const char *oe = getenv("NXZ_INFLATE_ORDER");
		const int order_env = oe ? atoi(oe) : -1;
		if (order_env < 0 ? n > lds_max : order_env != 0) {
			const auto use = lease_scratch(c, s);                          // (the kernel reads the order)
			uint8_t *const ows = with_scratch(c, s, [&](nxz_ctx::Scratch &sc) {
				return sc.buf[BUF_ORDER].grow(s, nxz_order_workspace(n)) != DevBuf::FAILED ? sc.buf[BUF_ORDER].p : nullptr;
			});
			order = nxz_launch_order_by_length(jobs, n, ows, s);              // (NULL: in the caller's order)
			rc = nxz_launch_inflate(jobs, n, results, dht_io, n <= lds_max, order, s);
		} else rc = nxz_launch_inflate(jobs, n, results, dht_io, n <= lds_max, nullptr, s);
	}
	if (rc) { set_err("inflate launch", (hipError_t)rc); return -EIO; }
	return 0;
}

// Streams that share a preset dictionary: a workgroup each with the window preloaded (nxzw::inflate_wg_dict_kernel), the hand-backs a
// wavefront each behind it (nxzi::inflate_dict_kernel), checksums -- all on `s`, nothing waits.  The caller holds no lock.
static int batch_decompress_dict(nxz_ctx_t *c, const nxz_dict *dict, const nxz_batch_job_t *jobs, size_t n, nxz_batch_result_t *results, hipStream_t s)
{
	const auto use = lease_scratch(c, s);
	uint8_t *wws = nullptr, *ows = nullptr;
	int rc = wg_workspaces(c, s, n, &wws, &ows);
	if (rc) return rc;
	const uint32_t *order = ows ? nxz_launch_order_by_length(jobs, n, ows, s) : nullptr;
	// Streams of fewer than NXZ_DICT_WG_MIN source bytes go a wavefront each from the start: the workgroup kernel costs a stream 84 000 -
	// 95 000 cycles whatever its size and has one stream a CU in flight, the wavefront kernel twenty (profiles/r08_dict.txt).  0: all a workgroup each.
	const char *wm = getenv("NXZ_DICT_WG_MIN");                         // (read at every call: the tests switch it)
	const uint32_t src_min = wm ? (uint32_t)strtoul(wm, nullptr, 0) : (uint32_t)NXZ_DICT_WG_MIN_DEFAULT;
	rc = nxz_launch_inflate_wg_dict(jobs, n, results, wws, order, dict->d_win, dict->win, src_min, s);
	if (rc) { set_err("inflate launch", (hipError_t)rc); return -EIO; }
	return 0;
}
extern "C" int nxz_batch_decompress_dict(nxz_ctx_t *c, const nxz_dict_t *dict, const nxz_batch_job_t *jobs, size_t n,
					 nxz_batch_result_t *results, void *stream)
{
	if (!c || !dict || dict->device != c->device || n >= (1u << 31) || (n && (!jobs || !results))) return -EINVAL;
	if (forked_child()) return -ENODEV;
	if (!n) return 0;
	(void)hipSetDevice(c->device);
	return batch_decompress_dict(c, dict, jobs, n, results, (hipStream_t)stream);
}

// (diagnostic / tests: how many streams of the last batch of n that `stream` ran through the lane kernels the fixed-code-only
// kernel handed back to the general one; waits for the stream)
extern "C" int nxz_inflate_lanes_handed_back(const uint8_t *workspace, size_t n, uint32_t *count);
extern "C" int nxz_ctx_lanes_handed_back(nxz_ctx_t *c, void *stream, size_t n, uint32_t *count)
{
	if (!c || !count) return -EINVAL;
	(void)hipSetDevice(c->device);
	hipStream_t s = (hipStream_t)stream;
	if (hipStreamSynchronize(s) != hipSuccess) return -EIO;
	const uint8_t *ws = nullptr;
	{
		std::lock_guard<std::mutex> g(c->mtx);
		auto it = c->scratch.find(s);
		if (it != c->scratch.end()) ws = it->second.buf[BUF_LANES].p;
	}
	if (!ws) return -ENOENT;
	return nxz_inflate_lanes_handed_back(ws, n, count) ? -EIO : 0;
}

// (diagnostic / tests: why the workgroup-per-stream kernel handed streams of the last batch on `stream` back: out16[1..14] by reason
// (nxz_inflate_wg.hip R_*), out16[15] the streams handed back; waits for the stream)
extern "C" int nxz_ctx_wg_reasons(nxz_ctx_t *c, void *stream, uint32_t *out16)
{
	if (!c || !out16) return -EINVAL;
	(void)hipSetDevice(c->device);
	hipStream_t s = (hipStream_t)stream;
	if (hipStreamSynchronize(s) != hipSuccess) return -EIO;
	const uint8_t *ws = nullptr;
	{
		std::lock_guard<std::mutex> g(c->mtx);
		auto it = c->scratch.find(s);
		if (it != c->scratch.end()) ws = it->second.buf[BUF_WG].p;
	}
	if (!ws) return -ENOENT;
	return nxz_inflate_wg_reasons(ws, out16) ? -EIO : 0;
}
extern "C" int nxz_ctx_wg_prof(nxz_ctx_t *c, void *stream, unsigned long long *out12)
{
	if (!c || !out12) return -EINVAL;
	(void)hipSetDevice(c->device);
	hipStream_t s = (hipStream_t)stream;
	if (hipStreamSynchronize(s) != hipSuccess) return -EIO;
	const uint8_t *ws = nullptr;
	{
		std::lock_guard<std::mutex> g(c->mtx);
		auto it = c->scratch.find(s);
		if (it != c->scratch.end()) ws = it->second.buf[BUF_WG].p;
	}
	if (!ws) return -ENOENT;
	return nxz_inflate_wg_prof(ws, out12) ? -EIO : 0;
}

extern "C" int nxz_batch_wrap(nxz_ctx_t *c, const nxz_batch_job_t *jobs, size_t n,
			      nxz_batch_result_t *results, void *stream)
{
	if (!c) return -EINVAL;
	(void)hipSetDevice(c->device);
	hipStream_t s = (hipStream_t)stream;   // NULL = the HIP default stream
	static const bool old_wrap = getenv("NXZ_WRAP_OLD") && atoi(getenv("NXZ_WRAP_OLD")) != 0;
	int rc = old_wrap ? nxz_launch_wrap(jobs, n, results, s) : nxz_launch_wrap_sliced(jobs, n, results, s);
	if (rc) { set_err("wrap launch", (hipError_t)rc); return -EIO; }
	return 0;
}

// Gzip members from the results of a compress batch (nxz_misc.hip): offsets[n + 1] and `packed`
// are device memory; offsets[n] is the number of bytes written to `packed`.
extern "C" int nxz_batch_pack_gzip(nxz_ctx_t *c, const nxz_batch_job_t *jobs, const nxz_batch_result_t *results, size_t n,
				   uint64_t *offsets, uint8_t *packed, void *stream)
{
	if (!c || !jobs || !results || !offsets || !packed || n > 0xffffffffu) return -EINVAL;
	(void)hipSetDevice(c->device);
	int rc = nxz_launch_pack_members(jobs, results, n, offsets, packed, (hipStream_t)stream);
	if (rc) { set_err("pack launch", (hipError_t)rc); return -EIO; }
	return 0;
}

extern "C" int nxz_batch_pack_zlib(nxz_ctx_t *c, int level, const nxz_batch_job_t *jobs, const nxz_batch_result_t *results, size_t n,
				   uint64_t *offsets, uint8_t *packed, void *stream)
{
	if (!c || !jobs || !results || !offsets || !packed || n > 0xffffffffu || level < -1 || level > 9) return -EINVAL;
	(void)hipSetDevice(c->device);
	// FLEVEL as zlib's deflate.c writes it: 0 for levels 0-1, 1 for 2-5, 2 for 6 (and the default), 3 for 7-9
	const uint32_t flevel = level < 0 || level == 6 ? 2 : level < 2 ? 0 : level < 6 ? 1 : 3;
	uint32_t hdr = 0x78u << 8 | flevel << 6;
	hdr += 31 - hdr % 31;
	int rc = nxz_launch_pack_zlib(jobs, results, n, hdr & 0xff, offsets, packed, (hipStream_t)stream);
	if (rc) { set_err("pack launch", (hipError_t)rc); return -EIO; }
	return 0;
}

extern "C" int nxz_batch_pack_zlib_dict(nxz_ctx_t *c, int level, const nxz_dict_t *dict, const nxz_batch_job_t *jobs, const nxz_batch_result_t *results,
					size_t n, uint64_t *offsets, uint8_t *packed, void *stream)
{
	if (!c || !dict || dict->device != c->device || !jobs || !results || !offsets || !packed || n > 0xffffffffu || level < -1 || level > 9) return -EINVAL;
	(void)hipSetDevice(c->device);
	int rc = nxz_launch_pack_zlib_dict(jobs, results, n, nxz_zlib_cmf_flg(level, 1) & 0xff, dict->id, offsets, packed, (hipStream_t)stream);
	if (rc) { set_err("pack launch", (hipError_t)rc); return -EIO; }
	return 0;
}

// ---------------------------------------------------------------------------
// Framed streams (nxz_frame.hip): header kernel -> the raw batch on the derived jobs -> trailer kernel, all on `s`.
// The caller holds c->frame_use[s].
// ---------------------------------------------------------------------------
static int framed_locked(nxz_ctx_t *c, int fmt, const nxz_batch_job_t *jobs, size_t n, nxz_batch_result_t *results,
			 nxz_batch_frame_t *frames, hipStream_t s, const nxz_dict *dict = nullptr)
{
	// (the caller's frame_use[s] guards the derived jobs: no lease here, batch_decompress takes its own)
	nxz_batch_job_t *const derived = with_scratch(c, s, [&](nxz_ctx::Scratch &sc) {
		(void)sc.buf[BUF_FRAME_JOBS].grow(s, n * sizeof(nxz_batch_job_t));
		return sc.buf[BUF_FRAME_JOBS].as<nxz_batch_job_t>();
	});
	if (!derived) return -ENOMEM;
	int rc = dict ? nxz_launch_frame_header_dict(fmt, jobs, n, frames, derived, dict->id, s) : nxz_launch_frame_header(fmt, jobs, n, frames, derived, s);
	if (rc) { set_err("frame header launch", (hipError_t)rc); return -EIO; }
	rc = dict ? batch_decompress_dict(c, dict, derived, n, results, s) : batch_decompress(c, derived, n, results, nullptr, s, 0);
	if (rc) return rc;
	rc = nxz_launch_frame_trailer(jobs, n, results, frames, s);
	if (rc) { set_err("frame trailer launch", (hipError_t)rc); return -EIO; }
	return 0;
}

static std::mutex *frame_mutex(nxz_ctx_t *c, hipStream_t s)
{
	std::lock_guard<std::mutex> g(c->mtx);
	return &c->frame_use[s];
}

extern "C" int nxz_batch_decompress_framed(nxz_ctx_t *c, int fmt, const nxz_batch_job_t *jobs, size_t n,
					   nxz_batch_result_t *results, nxz_batch_frame_t *frames, void *stream)
{
	if (!c || fmt < NXZ_FMT_ZLIB || fmt > NXZ_FMT_AUTO || n >= (1u << 31) || (n && (!jobs || !results || !frames))) return -EINVAL;
	if (forked_child()) return -ENODEV;
	if (!n) return 0;
	(void)hipSetDevice(c->device);
	hipStream_t s = (hipStream_t)stream;
	std::lock_guard<std::mutex> use(*frame_mutex(c, s));
	return framed_locked(c, fmt, jobs, n, results, frames, s);
}

extern "C" int nxz_batch_decompress_framed_dict(nxz_ctx_t *c, int fmt, const nxz_dict_t *dict, const nxz_batch_job_t *jobs, size_t n,
						nxz_batch_result_t *results, nxz_batch_frame_t *frames, void *stream)
{
	if (!c || !dict || dict->device != c->device || fmt < NXZ_FMT_ZLIB || fmt > NXZ_FMT_AUTO || n >= (1u << 31) || (n && (!jobs || !results || !frames))) return -EINVAL;
	if (forked_child()) return -ENODEV;
	if (!n) return 0;
	(void)hipSetDevice(c->device);
	hipStream_t s = (hipStream_t)stream;
	std::lock_guard<std::mutex> use(*frame_mutex(c, s));
	return framed_locked(c, fmt, jobs, n, results, frames, s, dict);
}

// ---------------------------------------------------------------------------
// Output sizes (nxz_inflate_size.hip): what the streams would produce, a wavefront each, all on `s`, nothing waits.  From 128
// streams on the long ones start first (the order is this stream's scratch, as for the decode routes).  The caller holds no lease.
// ---------------------------------------------------------------------------
static int batch_size(nxz_ctx_t *c, const nxz_batch_job_t *jobs, size_t n, nxz_batch_result_t *results, uint32_t dict_window, hipStream_t s)
{
	const auto use = lease_scratch(c, s);                                // (the kernel reads the order)
	uint8_t *const ows = n >= 128 ? with_scratch(c, s, [&](nxz_ctx::Scratch &sc) {
		return sc.buf[BUF_ORDER].grow(s, nxz_order_workspace(n)) != DevBuf::FAILED ? sc.buf[BUF_ORDER].p : nullptr;
	}) : nullptr;
	const uint32_t *order = ows ? nxz_launch_order_by_length(jobs, n, ows, s) : nullptr;   // (NULL: in the caller's order)
	const int rc = nxz_launch_inflate_size(jobs, n, results, order, dict_window, s);
	if (rc) { set_err("inflate size launch", (hipError_t)rc); return -EIO; }
	return 0;
}

extern "C" int nxz_batch_decompress_size(nxz_ctx_t *c, const nxz_batch_job_t *jobs, size_t n, nxz_batch_result_t *results, void *stream)
{
	if (!c || n >= (1u << 31) || (n && (!jobs || !results))) return -EINVAL;
	if (forked_child()) return -ENODEV;
	if (!n) return 0;
	(void)hipSetDevice(c->device);
	return batch_size(c, jobs, n, results, 0, (hipStream_t)stream);
}

// header kernel (the framed decode's own, with the dictionary's DICTID when there is one) -> the size walk on the derived jobs ->
// the trailer step without the checksum comparison.  frame_use[s] guards the derived jobs, as in framed_locked.
extern "C" int nxz_batch_decompress_size_framed(nxz_ctx_t *c, int fmt, const nxz_dict_t *dict, const nxz_batch_job_t *jobs, size_t n,
						nxz_batch_result_t *results, nxz_batch_frame_t *frames, void *stream)
{
	if (!c || (dict && dict->device != c->device) || fmt < NXZ_FMT_ZLIB || fmt > NXZ_FMT_AUTO || n >= (1u << 31) || (n && (!jobs || !results || !frames))) return -EINVAL;
	if (forked_child()) return -ENODEV;
	if (!n) return 0;
	(void)hipSetDevice(c->device);
	hipStream_t s = (hipStream_t)stream;
	std::lock_guard<std::mutex> use(*frame_mutex(c, s));
	nxz_batch_job_t *const derived = with_scratch(c, s, [&](nxz_ctx::Scratch &sc) {
		(void)sc.buf[BUF_FRAME_JOBS].grow(s, n * sizeof(nxz_batch_job_t));
		return sc.buf[BUF_FRAME_JOBS].as<nxz_batch_job_t>();
	});
	if (!derived) return -ENOMEM;
	int rc = dict ? nxz_launch_frame_header_dict(fmt, jobs, n, frames, derived, dict->id, s) : nxz_launch_frame_header(fmt, jobs, n, frames, derived, s);
	if (rc) { set_err("frame header launch", (hipError_t)rc); return -EIO; }
	// (without a dictionary the header kernel sets no NXZ_JOB_NO_DICT, and there is no window to withhold: 0)
	if ((rc = batch_size(c, derived, n, results, dict ? dict->win : 0, s)) != 0) return rc;
	rc = nxz_launch_size_trailer(jobs, n, results, frames, s);
	if (rc) { set_err("frame trailer launch", (hipError_t)rc); return -EIO; }
	return 0;
}

// ---------------------------------------------------------------------------
// Multi-member gzip jobs (nxz_gzip_members.hip, the rules in nxz_gzip_members.h).  The index is the size query's shape: a wavefront
// a job, from 128 jobs on the long ones first, the order in this stream's scratch under the lease.  The decode holds frame_use[s]
// from its first kernel to its last -- BUF_GZIP_MEMBERS is the framed batch framed_locked works on -- and never waits for the host.
// ---------------------------------------------------------------------------
extern "C" int nxz_batch_gzip_members_size(nxz_ctx_t *c, const nxz_batch_job_t *jobs, size_t n, uint32_t member_cap,
					   nxz_gzip_member_t *members, nxz_gzip_stream_t *streams, void *stream)
{
	if (!c || member_cap == 0 || n >= (1u << 31) || (n && (!jobs || !members || !streams))) return -EINVAL;
	if (forked_child()) return -ENODEV;
	if (!n) return 0;
	(void)hipSetDevice(c->device);
	hipStream_t s = (hipStream_t)stream;
	const auto use = lease_scratch(c, s);                                // (the kernel reads the order)
	uint8_t *const ows = n >= 128 ? with_scratch(c, s, [&](nxz_ctx::Scratch &sc) {
		return sc.buf[BUF_ORDER].grow(s, nxz_order_workspace(n)) != DevBuf::FAILED ? sc.buf[BUF_ORDER].p : nullptr;
	}) : nullptr;
	const uint32_t *order = ows ? nxz_launch_order_by_length(jobs, n, ows, s) : nullptr;   // (NULL: in the caller's order)
	const int rc = nxz_launch_gzip_members_index(jobs, n, member_cap, members, streams, order, s);
	if (rc) { set_err("gzip members index launch", (hipError_t)rc); return -EIO; }
	return 0;
}

extern "C" int nxz_batch_gzip_members_decode(nxz_ctx_t *c, const nxz_batch_job_t *jobs, size_t n, uint32_t member_cap,
					     nxz_gzip_member_t *members, nxz_gzip_stream_t *streams, size_t total_members, void *stream)
{
	if (!c || member_cap == 0 || total_members < n || n >= (1u << 31) || (n && (!jobs || !members || !streams))) return -EINVAL;
	if (forked_child()) return -ENODEV;
	if (!n) return 0;
	const uint64_t slots = (uint64_t)n * member_cap;                     // (n < 2^31, member_cap < 2^32: no overflow)
	const size_t total = (size_t)std::min<uint64_t>(total_members, slots);
	if (total >= (1u << 31) || slots >= (1ull << 39)) return -E2BIG;     // (the framed batch; a thread a record slot in one grid)
	(void)hipSetDevice(c->device);
	hipStream_t s = (hipStream_t)stream;
	std::lock_guard<std::mutex> use(*frame_mutex(c, s));
	uint8_t *const ws = with_scratch(c, s, [&](nxz_ctx::Scratch &sc) {
		(void)sc.buf[BUF_GZIP_MEMBERS].grow(s, nxz_gzip_members_workspace(n, total));
		return sc.buf[BUF_GZIP_MEMBERS].p;
	});
	if (!ws) return -ENOMEM;
	nxz_batch_job_t *xjobs = nullptr;
	nxz_batch_result_t *xresults = nullptr;
	nxz_batch_frame_t *xframes = nullptr;
	int rc = nxz_launch_gzip_members_expand(jobs, n, member_cap, members, streams, total, ws, &xjobs, &xresults, &xframes, s);
	if (rc) { set_err("gzip members expand launch", (hipError_t)rc); return -EIO; }
	if ((rc = framed_locked(c, NXZ_FMT_GZIP, xjobs, total, xresults, xframes, s)) != 0) return rc;
	rc = nxz_launch_gzip_members_join(n, member_cap, members, streams, total, ws, s);
	if (rc) { set_err("gzip members join launch", (hipError_t)rc); return -EIO; }
	return 0;
}

// ---------------------------------------------------------------------------
// One stream per device buffer (nxz_streams.hip, the rules in nxz_streams.h).  The host makes one pass over the streams -- the
// refusals and the block prefix first[n + 1] -- into pinned staging, uploads it with the descriptors, and queues per chunk of
// NXZ_STREAMS_CHUNK blocks: expand -> nxz_batch_compress on the device jobs -> layout and checksum joins -> pack; a prologue in
// front (headers, state) and an epilogue behind (empty streams, trailers, results).  Everything goes on `s`.
// No host wait: once the stream's scratch holds a batch of this size there is no hipStreamSynchronize, hipMalloc or hipFree on
// this path (DevBuf::grow and nxz_batch_compress's chunk only act when they must grow).  The one wait there can be is for the
// UPLOAD of the call before the last on this stream, whose pinned staging this call fills again (Scratch::h_up: two in turn, an
// event behind each upload); a caller who queues three calls faster than the device takes two uploads meets it, no other.
// frame_use[s] guards BUF_STREAMS and the staging, as it guards the derived jobs of the framed calls: nxz_batch_compress takes
// the scratch lease itself.
// ---------------------------------------------------------------------------
static uint32_t streams_chunk()
{
	const char *e = getenv("NXZ_STREAMS_CHUNK");                        // (read at every call: the tests switch it)
	const uint64_t v = e ? strtoull(e, nullptr, 0) : 0;
	return v ? (uint32_t)std::min<uint64_t>(v, 65536) : NXZ_STREAMS_CHUNK_DEFAULT;
}

extern "C" size_t nxz_deflate_stream_bound(uint64_t src_len, uint32_t hist_max, int fmt)
{
	return (size_t)nxz_streams_bound(src_len, hist_max, fmt);
}

extern "C" int nxz_batch_deflate_streams(nxz_ctx_t *c, int fc, int fmt, int level, uint32_t hist_max, const nxz_stream_job_t *jobs, size_t n,
					 nxz_stream_result_t *results, void *stream)
{
	if (!c || (fc != NXZ_FC_COMPRESS_FHT && fc != NXZ_FC_COMPRESS_DHTGEN) || !nxz_streams_fmt_ok(fmt) || level < -1 || level > 9 ||
	    (n && (!jobs || !results))) return -EINVAL;
	if (forked_child()) return -ENODEV;
	if (!n) return 0;
	if (n >= (1u << 31)) return -E2BIG;
	(void)hipSetDevice(c->device);
	hipStream_t s = (hipStream_t)stream;
	std::lock_guard<std::mutex> use(*frame_mutex(c, s));
	const uint32_t H = nxz_streams_window(hist_max), B = nxz_streams_block_bytes(hist_max), ns = (uint32_t)n;
	auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
	// what is uploaded: [descriptors][first], the same layout in the staging and in the device buffer
	const size_t o_first = up(n * sizeof(nxz_stream_job_t)), up_bytes = o_first + (n + 1) * sizeof(uint32_t);
	// this call's staging: the upload that read it last must have run
	struct Staging { uint8_t *h; size_t cap; hipEvent_t ev; unsigned k; };
	Staging st = with_scratch(c, s, [](nxz_ctx::Scratch &r) { const unsigned k = r.up_turn & 1; return Staging{r.h_up[k], r.h_up_cap[k], r.up_ev[k], k}; });
	if (!st.ev) HIPCHK(hipEventCreateWithFlags(&st.ev, hipEventDisableTiming), return -ENOMEM);
	else HIPCHK(hipEventSynchronize(st.ev), return -EIO);
	if (st.cap < up_bytes) {
		if (st.h) (void)hipHostFree(st.h);
		st.h = nullptr; st.cap = 0;
		if (hipHostMalloc((void **)&st.h, up_bytes) == hipSuccess) st.cap = up_bytes;
		else { (void)hipGetLastError(); st.h = nullptr; }
	}
	with_scratch(c, s, [&](nxz_ctx::Scratch &r) { r.h_up[st.k] = st.h; r.h_up_cap[st.k] = st.cap; r.up_ev[st.k] = st.ev; return 0; });
	if (!st.h) return -ENOMEM;
	// one pass over the streams: a refused stream gets no blocks
	nxz_stream_job_t *const h_desc = (nxz_stream_job_t *)st.h;
	uint32_t *const h_first = (uint32_t *)(st.h + o_first);
	memcpy(h_desc, jobs, n * sizeof(nxz_stream_job_t));
	uint64_t total = 0;
	for (size_t i = 0; i < n; i++) {
		h_first[i] = (uint32_t)total;
		if (!nxz_streams_refusal(&jobs[i], hist_max, fmt)) total += nxz_streams_blocks(jobs[i].src_len, B);
		if (total >= (1ull << 31)) return -E2BIG;
	}
	h_first[n] = (uint32_t)total;
	const uint32_t nblk = (uint32_t)total, C = std::min(streams_chunk(), nblk);
	const size_t o_state = up(up_bytes), o_jobs = o_state + up(n * sizeof(nxz_stream_state_t)), o_res = o_jobs + up((size_t)C * sizeof(nxz_batch_job_t)),
		     o_owner = o_res + up((size_t)C * sizeof(nxz_batch_result_t)), o_off = o_owner + up((size_t)C * sizeof(uint32_t)),
		     o_slots = o_off + up((size_t)C * sizeof(uint64_t)), d_bytes = o_slots + (size_t)C * NXZ_STREAMS_SLOT;
	uint8_t *const d = with_scratch(c, s, [&](nxz_ctx::Scratch &r) {
		(void)r.buf[BUF_STREAMS].grow(s, d_bytes);
		return r.buf[BUF_STREAMS].p;
	});
	if (!d) return -ENOMEM;
	const nxz_stream_job_t *const d_desc = (const nxz_stream_job_t *)d;
	const uint32_t *const d_first = (const uint32_t *)(d + o_first);
	nxz_stream_state_t *const d_state = (nxz_stream_state_t *)(d + o_state);
	nxz_batch_job_t *const d_jobs = (nxz_batch_job_t *)(d + o_jobs);
	nxz_batch_result_t *const d_res = (nxz_batch_result_t *)(d + o_res);
	uint32_t *const d_owner = (uint32_t *)(d + o_owner);
	uint64_t *const d_off = (uint64_t *)(d + o_off);
	uint8_t *const d_slots = d + o_slots;
	HIPCHK(hipMemcpyAsync(d, st.h, up_bytes, hipMemcpyHostToDevice, s), return -EIO);
	HIPCHK(hipEventRecord(st.ev, s), return -EIO);
	with_scratch(c, s, [](nxz_ctx::Scratch &r) { r.up_turn++; return 0; });
	int rc = nxz_launch_streams_prologue(d_desc, ns, hist_max, fmt, level, d_state, s);
	if (rc) { set_err("streams prologue launch", (hipError_t)rc); return -EIO; }
	const uint32_t op_block = nxz_crc_shift_op(B);
	uint32_t i_lo = 0;                                                  // the stream of the chunk's first block (the chunks go in order)
	for (uint32_t b0 = 0; b0 < nblk; b0 += C) {
		const uint32_t m = std::min(C, nblk - b0);
		while (h_first[i_lo + 1] <= b0) i_lo++;
		uint32_t i_hi = i_lo;
		while (h_first[i_hi + 1] < b0 + m) i_hi++;
		rc = nxz_launch_streams_expand(d_desc, d_first, ns, b0, m, hist_max, d_slots, d_jobs, d_owner, s);
		if (rc) { set_err("streams expand launch", (hipError_t)rc); return -EIO; }
		if ((rc = nxz_batch_compress(c, fc | (H ? 0x08 : 0), d_jobs, m, nullptr, 0, d_res, nullptr, s)) != 0) return rc;
		rc = nxz_launch_streams_layout(d_first, i_lo, i_hi - i_lo + 1, b0, m, d_jobs, d_res, hist_max, op_block, d_state, d_off, s);
		if (!rc) rc = nxz_launch_streams_pack(d_desc, d_first, d_owner, b0, m, d_jobs, d_res, d_off, s);
		if (rc) { set_err("streams pack launch", (hipError_t)rc); return -EIO; }
		i_lo = i_hi;
	}
	rc = nxz_launch_streams_epilogue(d_desc, d_first, ns, hist_max, fmt, d_state, results, s);
	if (rc) { set_err("streams epilogue launch", (hipError_t)rc); return -EIO; }
	return 0;
}

// The members of a BGZF image in device memory (nxz_launch_bgzf_discover; with coff: nxz_launch_bgzf_coff behind it), then
// ONE wait for ctl = candidates, members, bytes covered, sum of ISIZE.  The caller holds c->frame_use[s].
static int bgzf_discover_locked(nxz_ctx_t *c, const uint8_t *packed, uint64_t len, uint8_t *dst, uint64_t *offsets, size_t max_members,
				uint64_t *coff, hipStream_t s, uint64_t ctl[4], nxz_batch_job_t **jobs)
{
	// room for the candidates: twice the members the caller allows, and one every 32 KiB (a true member has at most
	// 64 KiB); an image with more -- false candidates in the payloads -- is run again with room for all of them
	const uint64_t most = len / 4 + 1;                                   // (1f 8b 08 04 cannot overlap itself)
	uint64_t cap = std::min<uint64_t>(most, std::max<uint64_t>((uint64_t)max_members * 2 + 1024, len / 32768 + 1024));
	for (int pass = 0; pass < 2; pass++) {
		uint8_t *const ws = with_scratch(c, s, [&](nxz_ctx::Scratch &sc) -> uint8_t * {
			cap = std::max(cap, sc.bgzf_cap);
			const DevBuf::Grown g = sc.buf[BUF_BGZF].grow(s, nxz_bgzf_workspace(len, cap));
			if (g != DevBuf::KEPT) sc.bgzf_cap = 0;                        // (another buffer, or none: what the old one had room for is history)
			if (g == DevBuf::FAILED) return nullptr;
			sc.bgzf_cap = std::max(sc.bgzf_cap, cap);
			return sc.buf[BUF_BGZF].p;
		});
		if (!ws) return -ENOMEM;
		int rc = nxz_launch_bgzf_discover(packed, len, dst, offsets, max_members, ws, cap, jobs, s);
		if (!rc && coff) rc = nxz_launch_bgzf_coff(packed, len, ws, cap, max_members, coff, s);
		if (rc) { set_err("bgzf discovery launch", (hipError_t)rc); return -EIO; }
		HIPCHK(hipMemcpyAsync(ctl, ws, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, s), return -EIO);
		HIPCHK(hipStreamSynchronize(s), return -EIO);
		if (ctl[0] <= cap) break;
		cap = ctl[0];                                                    // (every candidate, the second time)
	}
	return 0;
}

// A BGZF image in device memory: the members found on the device (nxz_launch_bgzf_discover), then ONE wait for their count,
// then the framed gzip path on them.
extern "C" int nxz_batch_unpack_gzip(nxz_ctx_t *c, const uint8_t *packed, uint64_t len, uint8_t *dst, uint64_t dst_cap,
				     uint64_t *offsets, nxz_batch_frame_t *frames, nxz_batch_result_t *results,
				     size_t max_members, uint64_t *members, uint64_t *consumed, uint64_t *out_len, void *stream)
{
	if (members) *members = 0;
	if (consumed) *consumed = 0;
	if (out_len) *out_len = 0;
	if (!c || (len && !packed) || !offsets || (max_members && (!frames || !results))) return -EINVAL;
	if (forked_child()) return -ENODEV;
	if (len < 26) return -EILSEQ;
	(void)hipSetDevice(c->device);
	hipStream_t s = (hipStream_t)stream;
	std::lock_guard<std::mutex> use(*frame_mutex(c, s));
	uint64_t ctl[4] = {0, 0, 0, 0};
	nxz_batch_job_t *jobs = nullptr;
	int rc = bgzf_discover_locked(c, packed, len, dst, offsets, max_members, nullptr, s, ctl, &jobs);
	if (rc) return rc;
	const uint64_t L = ctl[1];
	if (L == 0) return -EILSEQ;
	if (members) *members = L;
	if (consumed) *consumed = ctl[2];
	if (L > max_members) return -E2BIG;
	if (out_len) *out_len = ctl[3];
	if (ctl[3] > dst_cap) return -E2BIG;
	if (L >= (1u << 31)) return -E2BIG;
	rc = framed_locked(c, NXZ_FMT_GZIP, jobs, (size_t)L, results, frames, s);
	if (rc) return rc;
	HIPCHK(hipStreamSynchronize(s), return -EIO);
	return 0;
}

// The member index of a BGZF image: the discovery of nxz_batch_unpack_gzip (its layout's offsets are uoff) and coff.
extern "C" int nxz_bgzf_index(nxz_ctx_t *c, const uint8_t *packed, uint64_t len, uint64_t *coff, uint64_t *uoff, size_t max_members,
			      uint64_t *members, void *stream)
{
	if (members) *members = 0;
	if (!c || (len && !packed) || !coff || !uoff) return -EINVAL;
	if (forked_child()) return -ENODEV;
	if (len < 26) return -EILSEQ;
	(void)hipSetDevice(c->device);
	hipStream_t s = (hipStream_t)stream;
	std::lock_guard<std::mutex> use(*frame_mutex(c, s));
	uint64_t ctl[4] = {0, 0, 0, 0};
	nxz_batch_job_t *jobs = nullptr;
	int rc = bgzf_discover_locked(c, packed, len, nullptr, uoff, max_members, coff, s, ctl, &jobs);
	if (rc) return rc;
	if (ctl[1] == 0) return -EILSEQ;
	if (members) *members = ctl[1];
	return ctl[1] > max_members ? -E2BIG : 0;
}

// Members a chunk of nxz_bgzf_read_ranges decodes at most: NXZ_BGZF_CHUNK (read at every call: the tests lower it), 16 384
static uint64_t bgzf_chunk_members()
{
	const char *e = getenv("NXZ_BGZF_CHUNK");
	const uint64_t v = e ? strtoull(e, nullptr, 0) : 0;
	return v && v < 16384 ? v : 16384;
}

// Ranges of a BGZF image: the map (nxz_bgzf.hip) and ONE wait for its totals, then per chunk of needed members their
// framed decode into slots and the gather of the pieces, then the zeros of damaged ranges and a last wait.
extern "C" int nxz_bgzf_read_ranges(nxz_ctx_t *c, const uint8_t *packed, uint64_t packed_len, const uint64_t *coff, const uint64_t *uoff,
				    uint64_t nidx, int kind, const nxz_bgzf_range_t *ranges, size_t n, uint8_t *dst, uint64_t dst_cap,
				    uint64_t *offsets, uint32_t *status, uint64_t *out_len, uint64_t *decoded, void *stream)
{
	if (out_len) *out_len = 0;
	if (decoded) *decoded = 0;
	if (!c || !coff || !uoff || !offsets || nidx == 0 || nidx > 0xffffffffull || (packed_len && !packed) || (n && (!ranges || !status)) ||
	    (kind != NXZ_RANGE_UOFF && kind != NXZ_RANGE_VOFF) || n >= (1ull << 31))
		return -EINVAL;
	if (forked_child()) return -ENODEV;
	(void)hipSetDevice(c->device);
	hipStream_t s = (hipStream_t)stream;
	std::lock_guard<std::mutex> use(*frame_mutex(c, s));
	const uint64_t L = nidx - 1;
	uint8_t *const ws = with_scratch(c, s, [&](nxz_ctx::Scratch &sc) {
		(void)sc.buf[BUF_RNG].grow(s, nxz_bgzf_ranges_workspace(n, L));
		return sc.buf[BUF_RNG].p;
	});
	if (!ws) return -ENOMEM;
	int rc = nxz_launch_bgzf_map(packed, packed_len, coff, uoff, L, kind, ranges, n, offsets, status, ws, s);
	if (rc) { set_err("bgzf map launch", (hipError_t)rc); return -EIO; }
	uint64_t ctl[5];
	HIPCHK(hipMemcpyAsync(ctl, ws, sizeof(ctl), hipMemcpyDeviceToHost, s), return -EIO);
	HIPCHK(hipStreamSynchronize(s), return -EIO);
	if (ctl[0]) return -EILSEQ;
	if (out_len) *out_len = ctl[2];
	if (ctl[2] > dst_cap || (ctl[2] && !dst)) return -E2BIG;
	const uint64_t needed = ctl[1], pieces = ctl[3];
	if (!needed) return 0;
	// a slot per member of the chunk, all of the largest needed member's size (65 536 for BGZF): at most 1 GiB of them
	const uint64_t stride = (std::max<uint64_t>(ctl[4], 16) + 15) & ~(uint64_t)15;
	const uint64_t per = std::min(needed, std::min(bgzf_chunk_members(), std::max<uint64_t>(1, (1ull << 30) / stride)));
	const size_t sb = (per * stride + 255) & ~(size_t)255, jb = (per * sizeof(nxz_batch_job_t) + 255) & ~(size_t)255,
		     fb = (per * sizeof(nxz_batch_frame_t) + 255) & ~(size_t)255;
	uint8_t *const slots = with_scratch(c, s, [&](nxz_ctx::Scratch &sc) {
		(void)sc.buf[BUF_RNG_SLOTS].grow(s, sb + jb + fb + per * sizeof(nxz_batch_result_t));
		return sc.buf[BUF_RNG_SLOTS].p;
	});
	if (!slots) return -ENOMEM;
	nxz_batch_job_t *jobs = (nxz_batch_job_t *)(slots + sb);
	nxz_batch_frame_t *frames = (nxz_batch_frame_t *)(slots + sb + jb);
	nxz_batch_result_t *results = (nxz_batch_result_t *)(slots + sb + jb + fb);
	for (uint64_t k0 = 0; k0 < needed; k0 += per) {
		const uint64_t cnt = std::min(per, needed - k0);
		rc = nxz_launch_bgzf_jobs(packed, coff, uoff, n, L, ws, k0, cnt, slots, stride, jobs, s);
		if (rc) { set_err("bgzf jobs launch", (hipError_t)rc); return -EIO; }
		rc = framed_locked(c, NXZ_FMT_GZIP, jobs, (size_t)cnt, results, frames, s);
		if (rc) return rc;
		rc = nxz_launch_bgzf_gather(uoff, n, L, pieces, ws, offsets, slots, stride, k0, cnt, frames, results, dst, status, s);
		if (rc) { set_err("bgzf gather launch", (hipError_t)rc); return -EIO; }
	}
	rc = nxz_launch_bgzf_zero(n, offsets, status, dst, s);
	if (rc) { set_err("bgzf zero launch", (hipError_t)rc); return -EIO; }
	HIPCHK(hipStreamSynchronize(s), return -EIO);
	if (decoded) *decoded = needed;
	return 0;
}

// ---------------------------------------------------------------------------
// Checkpoints (nxz_checkpoint.hip, the rules in nxz_checkpoint.h).  The index is the size query's shape: a wavefront a job, from 128
// jobs on the long ones first, the order in this stream's scratch under the lease; the windows' copies go behind it on `s`, and
// nothing waits for the host.
// ---------------------------------------------------------------------------
extern "C" int nxz_batch_checkpoint_index(nxz_ctx_t *c, int fmt, const nxz_batch_job_t *jobs, size_t n, uint64_t span, uint32_t cp_cap,
					  uint64_t *cbit, uint64_t *uoff, uint8_t *windows, nxz_checkpoint_stream_t *streams, void *stream)
{
	if (!c || fmt < NXZ_FMT_RAW || fmt > NXZ_FMT_AUTO || span == 0 || cp_cap == 0 || n >= (1u << 31) || (n && (!jobs || !cbit || !uoff || !streams)))
		return -EINVAL;
	if (forked_child()) return -ENODEV;
	if (!n) return 0;
	(void)hipSetDevice(c->device);
	hipStream_t s = (hipStream_t)stream;
	const auto use = lease_scratch(c, s);                                // (the kernel reads the order)
	uint8_t *const ows = n >= 128 ? with_scratch(c, s, [&](nxz_ctx::Scratch &sc) {
		return sc.buf[BUF_ORDER].grow(s, nxz_order_workspace(n)) != DevBuf::FAILED ? sc.buf[BUF_ORDER].p : nullptr;
	}) : nullptr;
	const uint32_t *order = ows ? nxz_launch_order_by_length(jobs, n, ows, s) : nullptr;   // (NULL: in the caller's order)
	const int rc = nxz_launch_checkpoint_index(fmt, jobs, n, span, cp_cap, cbit, uoff, windows, streams, order, s);
	if (rc) { set_err("checkpoint index launch", (hipError_t)rc); return -EIO; }
	return 0;
}

// Ranges of one stream through its checkpoint index: nxz_bgzf_read_ranges with segments for members.  The map (the index check of
// nxz_checkpoint.hip inside nxz_bgzf.hip's) and ONE wait for its totals, then per chunk of needed segments their inputs staged,
// nxz_batch_decompress on them, the verdicts and nxz_bgzf.hip's gather, then the zeros of damaged ranges and a last wait.
// BUF_RNG and BUF_RNG_SLOTS are the BGZF call's: both calls hold frame_use[s] from the first kernel to the last wait.
extern "C" int nxz_checkpoint_read_ranges(nxz_ctx_t *c, const uint8_t *src, uint64_t src_len, const uint64_t *cbit, const uint64_t *uoff,
					  const uint8_t *windows, uint64_t nidx, const nxz_bgzf_range_t *ranges, size_t n, uint8_t *dst,
					  uint64_t dst_cap, uint64_t *offsets, uint32_t *status, uint64_t *out_len, uint64_t *decoded, void *stream)
{
	if (out_len) *out_len = 0;
	if (decoded) *decoded = 0;
	if (!c || !src || !cbit || !uoff || !offsets || nidx < 2 || nidx > 0xffffffffull || (!windows && nidx > 2) || (n && (!ranges || !status)) ||
	    n >= (1ull << 31))
		return -EINVAL;
	if (forked_child()) return -ENODEV;
	(void)hipSetDevice(c->device);
	hipStream_t s = (hipStream_t)stream;
	std::lock_guard<std::mutex> use(*frame_mutex(c, s));
	const uint64_t L = nidx - 1;
	uint8_t *const ws = with_scratch(c, s, [&](nxz_ctx::Scratch &sc) {
		(void)sc.buf[BUF_RNG].grow(s, nxz_bgzf_ranges_workspace(n, L));
		return sc.buf[BUF_RNG].p;
	});
	if (!ws) return -ENOMEM;
	int rc = nxz_launch_range_map_clear(ws, n, L, s);
	if (!rc) rc = nxz_launch_checkpoint_check(src_len, cbit, uoff, L, ws, s);
	if (!rc) rc = nxz_launch_range_map_ranges(uoff, L, ranges, n, offsets, status, ws, s);
	if (!rc) rc = nxz_launch_checkpoint_inmax(cbit, uoff, n, L, ws, s);
	if (rc) { set_err("checkpoint map launch", (hipError_t)rc); return -EIO; }
	uint64_t ctl[6];
	HIPCHK(hipMemcpyAsync(ctl, ws, sizeof(ctl), hipMemcpyDeviceToHost, s), return -EIO);
	HIPCHK(hipStreamSynchronize(s), return -EIO);
	if (ctl[0]) return -EILSEQ;
	if (out_len) *out_len = ctl[2];
	if (ctl[2] > dst_cap || (ctl[2] && !dst)) return -E2BIG;
	const uint64_t needed = ctl[1], pieces = ctl[3];
	if (!needed) return 0;
	// an input and an output slot per segment of the chunk, all of the largest needed segment's size: at most 1 GiB of either (a
	// segment larger than that goes alone)
	const uint64_t ostride = (std::max<uint64_t>(ctl[4], 16) + 15) & ~(uint64_t)15, istride = (std::max<uint64_t>(ctl[5], 16) + 15) & ~(uint64_t)15;
	const uint64_t per = std::min(needed, std::min(bgzf_chunk_members(), std::max<uint64_t>(1, (1ull << 30) / std::max(istride, ostride))));
	const size_t ib = (per * istride + 255) & ~(size_t)255, ob = (per * ostride + 255) & ~(size_t)255,
		     jb = (per * sizeof(nxz_batch_job_t) + 255) & ~(size_t)255, fb = (per * sizeof(nxz_batch_frame_t) + 255) & ~(size_t)255;
	uint8_t *const slots = with_scratch(c, s, [&](nxz_ctx::Scratch &sc) {
		(void)sc.buf[BUF_RNG_SLOTS].grow(s, ib + ob + jb + fb + per * sizeof(nxz_batch_result_t));
		return sc.buf[BUF_RNG_SLOTS].p;
	});
	if (!slots) return -ENOMEM;
	uint8_t *const oslots = slots + ib;
	nxz_batch_job_t *jobs = (nxz_batch_job_t *)(slots + ib + ob);
	nxz_batch_frame_t *frames = (nxz_batch_frame_t *)(slots + ib + ob + jb);
	nxz_batch_result_t *results = (nxz_batch_result_t *)(slots + ib + ob + jb + fb);
	for (uint64_t k0 = 0; k0 < needed; k0 += per) {
		const uint64_t cnt = std::min(per, needed - k0);
		rc = nxz_launch_checkpoint_stage(src, cbit, uoff, windows, n, L, ws, k0, cnt, slots, istride, oslots, ostride, jobs, s);
		if (rc) { set_err("checkpoint stage launch", (hipError_t)rc); return -EIO; }
		rc = batch_decompress(c, jobs, (size_t)cnt, results, nullptr, s, 0);
		if (rc) return rc;
		rc = nxz_launch_checkpoint_verdict(uoff, n, L, ws, k0, cnt, results, frames, s);
		if (rc) { set_err("checkpoint verdict launch", (hipError_t)rc); return -EIO; }
		rc = nxz_launch_bgzf_gather(uoff, n, L, pieces, ws, offsets, oslots, ostride, k0, cnt, frames, results, dst, status, s);
		if (rc) { set_err("checkpoint gather launch", (hipError_t)rc); return -EIO; }
	}
	rc = nxz_launch_bgzf_zero(n, offsets, status, dst, s);
	if (rc) { set_err("checkpoint zero launch", (hipError_t)rc); return -EIO; }
	HIPCHK(hipStreamSynchronize(s), return -EIO);
	if (decoded) *decoded = needed;
	return 0;
}
