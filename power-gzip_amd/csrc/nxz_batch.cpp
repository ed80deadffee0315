// nxz_batch.cpp -- the raw batches of include/nxz_engine.h's device-resident interface: the compress and inflate batches and which
// kernels they get, their dictionary forms, table generation, wrap and the pack forms, nxz_trim, stage timing and the diagnostics.
// (The calls around them are nxz_batch_framed.cpp's -- framed streams, sizes, members --, nxz_batch_streams.cpp's -- one-stream deflate and inflate -- and nxz_batch_ranges.cpp's -- BGZF and checkpoints.)
#include "nxz_ctx.h"
#include "nxz_inflate_part.h"

// ---------------------------------------------------------------------------
// batched, device-resident interface
// ---------------------------------------------------------------------------
// Jobs per launch of the compress kernels: bounds the token scratch (104 KiB per job: 832 MiB for 8192
// jobs, 6.6 GiB for 65536).  Larger chunks cost memory, smaller ones time: the LZ77 kernel is one persistent
// workgroup per CU, at the end of a launch CUs idle until the last job is done, and every chunk is four launches
// (LZ77, symbol counts, table, entropy; three for a caller's table or the fixed code with counts)
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
static_assert(NXZ_INFLATE_PART_CHUNK_STREAMS < NXZ_LANES_MIN, "a chunk of nxz_batch_inflate_streams_part must stay below the batches that are sampled or go a stream per lane");
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

// The compress function codes: LZ77 kernel (tokens) -> [symbol counts -> table generator] ->
// entropy kernel (the block, its checksums), chunk after chunk on the caller's stream.  (The symbol-count kernel is
// nxz_launch_lz77's own second launch: the stage stamps count it as "lz77".)
static int batch_compress(nxz_ctx_t *c, int fc, const nxz_batch_job_t *jobs, size_t n,
			  const nxz_batch_dht_t *dht, size_t ntables, nxz_batch_result_t *results,
			  uint32_t *counts, void *stream, const nxz_dict *dict, const uint8_t *win = nullptr, size_t nwin = 0);
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
// ... with a window of the caller's choosing for the first nwin jobs and none but their own for the rest (nxz_batch_deflate_streams_dict:
// the first blocks of a chunk's streams, then its other blocks).  The DEVICE jobs are as the kernels take them already -- the first
// nwin as nxz_launch_dict_jobs would write them, hist_len = the window's length -- so nothing is rewritten and no job is refused.
int batch_compress_windowed(nxz_ctx_t *c, int fc, const uint8_t *win, size_t nwin, const nxz_batch_job_t *jobs, size_t n,
			    nxz_batch_result_t *results, void *stream)
{
	if (!win || nwin > n) return -EINVAL;
	return batch_compress(c, fc, jobs, n, nullptr, 0, results, nullptr, stream, nullptr, win, nwin);
}
// dict: every job gets the dictionary's deflate window (the caller's jobs are rewritten first).  win: jobs [0, nwin) get `win`.
static int batch_compress(nxz_ctx_t *c, int fc, const nxz_batch_job_t *ujobs, size_t n,
			  const nxz_batch_dht_t *dht, size_t ntables, nxz_batch_result_t *results,
			  uint32_t *counts, void *stream, const nxz_dict *dict, const uint8_t *win, size_t nwin)
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
	// equal chunks (a last chunk of a few jobs would cost four launches for nothing)
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
		if (int rc = launched("dictionary jobs launch", nxz_launch_dict_jobs(ujobs, n, dict->W, djobs, s))) return rc;
		jobs = djobs;
	}
	if (isdht && !gen) {
		prepared = sc.buf[BUF_PREPARED].as<nxz_dht_prepared_t>();
		if (int rc = launched("dht prepare launch", nxz_launch_dht_prepare(dht, ntables, prepared, s))) return rc;
	}
	if (dict) { win = dict->deflate_window(); nwin = n; }
	for (size_t off = 0; off < n; off += chunk) {
		const size_t m = n - off < chunk ? n - off : chunk;
		const size_t mw = off < nwin ? std::min(m, nwin - off) : 0;      // the chunk's jobs that take `win`: its first mw
		auto draw = [&]() {
			std::lock_guard<std::mutex> g(c->mtx);
			return c->d_job_counters ? c->d_job_counters + (c->next_counter++ % JOB_COUNTERS) : nullptr;
		};
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
		// (a launch indexes tokens and counts by the job's place in it; the fused forms' scratch is a workgroup's, not a job's)
		int rc = mw ? nxz_launch_lz77_dict(mode, jobs + off, mw, lz_scratch, sc.d_cand2, results + off, lz_counts, draw(), win, s) : 0;
		if (!rc && mw < m)
			rc = nxz_launch_lz77(mode, jobs + off + mw, m - mw, fused ? lz_scratch : lz_scratch + mw * (size_t)NXZ_TOK_STRIDE, sc.d_cand2,
					     results + off + mw, lz_counts ? lz_counts + mw * 316 : nullptr, draw(), s);
		if ((rc = launched("lz77 launch", rc)) != 0) return rc;
		stamp();
		if (fused) { stamp(); stamp(); continue; }
		if (gen) {
			if ((rc = launched("dhtgen launch", nxz_launch_dhtgen(cnt, m, sc.d_gen, nullptr, s))) != 0) return rc;
		}
		stamp();
		rc = launched("encode launch", nxz_launch_encode(isdht, gen, jobs + off, m, sc.d_tokens, gen ? sc.d_gen : prepared, results + off, s));
		if (rc) return rc;
		stamp();
	}
	return dict ? launched("dictionary finish launch", nxz_launch_dict_finish(ujobs, n, dict->W, results, s)) : 0;
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
	return launched("dhtgen launch", nxz_launch_dhtgen(counts, n, nullptr, tables, (hipStream_t)stream));
}

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

const uint32_t *order_by_length_for(nxz_ctx *c, hipStream_t s, const nxz_batch_job_t *jobs, size_t n)
{
	uint8_t *const ows = with_scratch(c, s, [&](nxz_ctx::Scratch &sc) {
		return sc.buf[BUF_ORDER].grow(s, nxz_order_workspace(n)) != DevBuf::FAILED ? sc.buf[BUF_ORDER].p : nullptr;
	});
	return nxz_launch_order_by_length(jobs, n, ows, s);                  // (NULL without a workspace)
}

// The workspace of the workgroup-per-stream kernels for n streams on `s` (NULL: none to be had).  The caller holds the lease.
static uint8_t *wg_workspace(nxz_ctx *c, hipStream_t s, size_t n)
{
	return with_scratch(c, s, [&](nxz_ctx::Scratch &sc) {
		(void)sc.buf[BUF_WG].grow(s, nxz_inflate_wg_workspace(n));
		return sc.buf[BUF_WG].p;
	});
}

int batch_decompress(nxz_ctx_t *c, const nxz_batch_job_t *jobs, size_t n, nxz_batch_result_t *results, nxz_batch_dht_t *dht_io, void *stream, int force)
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
		uint8_t *const wws = wg_workspace(c, s, n);
		if (!wws) return -ENOMEM;
		const uint32_t *order = n >= 128 ? order_by_length_for(c, s, jobs, n) : nullptr;   // (a workgroup draws stream after stream: the long ones first)
		return launched("inflate launch", nxz_launch_inflate_wg(jobs, n, results, dht_io, wws, order, nullptr, s));
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
			order = order_by_length_for(c, s, jobs, n);                       // (NULL: in the caller's order)
			rc = nxz_launch_inflate(jobs, n, results, dht_io, n <= lds_max, order, s);
		} else rc = nxz_launch_inflate(jobs, n, results, dht_io, n <= lds_max, nullptr, s);
	}
	return launched("inflate launch", rc);
}

// Streams that share a preset dictionary: a workgroup each with the window preloaded (nxzw::inflate_wg_dict_kernel), the hand-backs a
// wavefront each behind it (nxzi::inflate_dict_kernel), checksums -- all on `s`, nothing waits.  The caller holds no lock.
int batch_decompress_dict(nxz_ctx_t *c, const nxz_dict *dict, const nxz_batch_job_t *jobs, size_t n, nxz_batch_result_t *results, hipStream_t s)
{
	const auto use = lease_scratch(c, s);
	uint8_t *const wws = wg_workspace(c, s, n);
	if (!wws) return -ENOMEM;
	const uint32_t *order = n >= 128 ? order_by_length_for(c, s, jobs, n) : nullptr;
	// Streams of fewer than NXZ_DICT_WG_MIN source bytes go a wavefront each from the start: the workgroup kernel costs a stream 84 000 -
	// 95 000 cycles whatever its size and has one stream a CU in flight, the wavefront kernel twenty (profiles/r08_dict.txt).  0: all a workgroup each.
	const char *wm = getenv("NXZ_DICT_WG_MIN");                         // (read at every call: the tests switch it)
	const uint32_t src_min = wm ? (uint32_t)strtoul(wm, nullptr, 0) : (uint32_t)NXZ_DICT_WG_MIN_DEFAULT;
	return launched("inflate launch", nxz_launch_inflate_wg_dict(jobs, n, results, wws, order, dict->d_win, dict->win, src_min, s));
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

// The diagnostics below look at what the last batch on `stream` left in that stream's scratch: waits for the stream, then *p = its
// buffer `which` as it stands (find, not []: a stream without scratch gets none made).  -EIO: the wait failed; -ENOENT: no such buffer.
static int settled_buffer(nxz_ctx_t *c, void *stream, ScratchBuf which, const uint8_t **p)
{
	(void)hipSetDevice(c->device);
	hipStream_t s = (hipStream_t)stream;
	if (hipStreamSynchronize(s) != hipSuccess) return -EIO;
	std::lock_guard<std::mutex> g(c->mtx);
	auto it = c->scratch.find(s);
	*p = it != c->scratch.end() ? it->second.buf[which].p : nullptr;
	return *p ? 0 : -ENOENT;
}

// (diagnostic / tests: how many streams of the last batch of n that `stream` ran through the lane kernels the fixed-code-only
// kernel handed back to the general one; waits for the stream)
extern "C" int nxz_inflate_lanes_handed_back(const uint8_t *workspace, size_t n, uint32_t *count);
extern "C" int nxz_ctx_lanes_handed_back(nxz_ctx_t *c, void *stream, size_t n, uint32_t *count)
{
	if (!c || !count) return -EINVAL;
	const uint8_t *ws = nullptr;
	if (int rc = settled_buffer(c, stream, BUF_LANES, &ws)) return rc;
	return nxz_inflate_lanes_handed_back(ws, n, count) ? -EIO : 0;
}

// (diagnostic / tests: why the workgroup-per-stream kernel handed streams of the last batch on `stream` back: out16[1..14] by reason
// (nxz_inflate_wg.hip R_*), out16[15] the streams handed back; waits for the stream)
extern "C" int nxz_ctx_wg_reasons(nxz_ctx_t *c, void *stream, uint32_t *out16)
{
	if (!c || !out16) return -EINVAL;
	const uint8_t *ws = nullptr;
	if (int rc = settled_buffer(c, stream, BUF_WG, &ws)) return rc;
	return nxz_inflate_wg_reasons(ws, out16) ? -EIO : 0;
}
extern "C" int nxz_ctx_wg_prof(nxz_ctx_t *c, void *stream, unsigned long long *out12)
{
	if (!c || !out12) return -EINVAL;
	const uint8_t *ws = nullptr;
	if (int rc = settled_buffer(c, stream, BUF_WG, &ws)) return rc;
	return nxz_inflate_wg_prof(ws, out12) ? -EIO : 0;
}

extern "C" int nxz_batch_wrap(nxz_ctx_t *c, const nxz_batch_job_t *jobs, size_t n,
			      nxz_batch_result_t *results, void *stream)
{
	if (!c) return -EINVAL;
	(void)hipSetDevice(c->device);
	hipStream_t s = (hipStream_t)stream;   // NULL = the HIP default stream
	static const bool old_wrap = getenv("NXZ_WRAP_OLD") && atoi(getenv("NXZ_WRAP_OLD")) != 0;
	return launched("wrap launch", old_wrap ? nxz_launch_wrap(jobs, n, results, s) : nxz_launch_wrap_sliced(jobs, n, results, s));
}

// Gzip members from the results of a compress batch (nxz_misc.hip): offsets[n + 1] and `packed`
// are device memory; offsets[n] is the number of bytes written to `packed`.
extern "C" int nxz_batch_pack_gzip(nxz_ctx_t *c, const nxz_batch_job_t *jobs, const nxz_batch_result_t *results, size_t n,
				   uint64_t *offsets, uint8_t *packed, void *stream)
{
	if (!c || !jobs || !results || !offsets || !packed || n > 0xffffffffu) return -EINVAL;
	(void)hipSetDevice(c->device);
	return launched("pack launch", nxz_launch_pack_members(jobs, results, n, offsets, packed, (hipStream_t)stream));
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
	return launched("pack launch", nxz_launch_pack_zlib(jobs, results, n, hdr & 0xff, offsets, packed, (hipStream_t)stream));
}

extern "C" int nxz_batch_pack_zlib_dict(nxz_ctx_t *c, int level, const nxz_dict_t *dict, const nxz_batch_job_t *jobs, const nxz_batch_result_t *results,
					size_t n, uint64_t *offsets, uint8_t *packed, void *stream)
{
	if (!c || !dict || dict->device != c->device || !jobs || !results || !offsets || !packed || n > 0xffffffffu || level < -1 || level > 9) return -EINVAL;
	(void)hipSetDevice(c->device);
	return launched("pack launch", nxz_launch_pack_zlib_dict(jobs, results, n, nxz_zlib_cmf_flg(level, 1) & 0xff, dict->id, offsets, packed, (hipStream_t)stream));
}
