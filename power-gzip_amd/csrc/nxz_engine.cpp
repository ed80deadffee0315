// nxz_engine.cpp -- host side of libnxz_engine.so: the C ABI of include/nxz_engine.h
// on top of the HIP kernels (nxz_lz77.hip, nxz_dhtgen.hip, nxz_encode.hip, nxz_inflate*.hip, nxz_misc.hip).
//
// What it replaces in the reference (paths relative to the libnxz tree):
//   lib/gzip_vas.c  -- open /dev/crypto/nx-gzip, VAS window, copy/paste of the
//                      CRB, CSB polling (:94-417).  Here: a HIP stream per job
//                      slot, pinned staging of the DDE gather/scatter lists,
//                      kernel launch, and completion written to the CSB.
//   lib/crc32_power.c -- __crc32_vpmsum (vector CRC on POWER).  Here: slice-by-8.
// There is NO CPU fallback for the engine ops: without a gfx950 device
// nx_function_begin fails with ENODEV and nxu_run_job completes jobs with
// CC = NXZ_CC_NO_HW.
#include "nxz_ctx.h"

#define NXZ_VERSION "nxz-engine 0.1 (gfx950)"

static thread_local char g_err[256];
void set_err(const char *what, hipError_t e)
{
	snprintf(g_err, sizeof(g_err), "%s: %s", what, e == hipSuccess ? "error" : hipGetErrorString(e));
}

extern "C" const char *nxz_last_error(void) { return g_err; }
extern "C" size_t nxz_pinflate_trim(void);
extern "C" size_t nxz_trim(void) { return nxz_pinflate_trim() + trim_compress_scratch(); }
extern "C" const char *nxz_engine_version(void) { return NXZ_VERSION; }
extern "C" size_t nxz_compress_bound(size_t n) { return ((n * 9 + 7) / 8 + 16 + 15) & ~(size_t)15; }

#define OUT_CAP (SUBBLOCK * 2 + 4096)    /* staging for one job's target */
#define INF_SRC_CAP (1u << 20)           /* decompress: source bytes taken per job */
#define INF_OUT_CAP (4u << 20)

std::mutex g_mtx;
nxz_ctx *g_ctx[64];
pid_t g_creator_pid = 0;

static bool slot_init(Slot &s)
{
	HIPCHK(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking), return false);
	HIPCHK(hipHostMalloc((void **)&s.h_in, INF_SRC_CAP + 64), return false);
	HIPCHK(hipHostMalloc((void **)&s.h_out, INF_OUT_CAP), return false);
	HIPCHK(hipMalloc((void **)&s.d_in, INF_SRC_CAP + 64), return false);
	HIPCHK(hipMalloc((void **)&s.d_out, INF_OUT_CAP), return false);
	HIPCHK(hipHostMalloc((void **)&s.h_job, sizeof(nxz_batch_job_t)), return false);
	HIPCHK(hipMalloc((void **)&s.d_job, sizeof(nxz_batch_job_t)), return false);
	HIPCHK(hipHostMalloc((void **)&s.h_res, sizeof(nxz_batch_result_t)), return false);
	HIPCHK(hipMalloc((void **)&s.d_res, sizeof(nxz_batch_result_t)), return false);
	HIPCHK(hipHostMalloc((void **)&s.h_dht, sizeof(nxz_batch_dht_t)), return false);
	HIPCHK(hipMalloc((void **)&s.d_dht, sizeof(nxz_batch_dht_t)), return false);
	HIPCHK(hipMalloc((void **)&s.d_prep, sizeof(nxz_dht_prepared_t)), return false);
	HIPCHK(hipHostMalloc((void **)&s.h_cnt, 316 * 4), return false);
	HIPCHK(hipMalloc((void **)&s.d_cnt, 316 * 4), return false);
	return true;
}

static void slot_free(Slot &s)
{
	if (s.stream) (void)hipStreamDestroy(s.stream);
	(void)hipHostFree(s.h_in); (void)hipHostFree(s.h_out); (void)hipFree(s.d_in); (void)hipFree(s.d_out);
	(void)hipHostFree(s.h_job); (void)hipFree(s.d_job); (void)hipHostFree(s.h_res); (void)hipFree(s.d_res);
	(void)hipHostFree(s.h_dht); (void)hipFree(s.d_dht); (void)hipFree(s.d_prep);
	(void)hipHostFree(s.h_cnt); (void)hipFree(s.d_cnt);
	s = Slot();
}

extern "C" int nxz_engine_usable(void) { return forked_child() ? 0 : 1; }

// Which device a caller that names none (NX_GZIP_DEV_NUM = -1, the default) gets.  The reference opens the
// NX unit nearest the calling CPU, or the one NX_GZIP_DEV_NUM names (lib/nx_zlib.c:568-576,1081,1281-1287), so a
// process with many threads uses every engine of the machine.  Here: NXZ_DEVICE names one; else the calling
// THREAD keeps one device for all its streams -- the first thread of the process the current HIP device (what a
// single-threaded caller has always got), every further thread the next visible device in turn -- so that T
// threads spread over min(T, ndev) GPUs.  NXZ_DEVICE_POLICY=current: every thread the current device.
// Pure function of its arguments (tests/test_config.py calls it with made-up device counts).
extern "C" int nxz_pick_device(int requested, int ndev, int current, unsigned thread_index, int spread)
{
	if (ndev <= 0) return -1;
	if (requested >= 0) return requested < ndev ? requested : -1;      // an explicit ordinal pins (out of range: no such device)
	if (current < 0 || current >= ndev) current = 0;
	if (!spread) return current;
	return (int)(((unsigned)current + thread_index) % (unsigned)ndev);
}

static unsigned calling_thread_index()
{
	static std::atomic<unsigned> next{0};
	static thread_local unsigned mine = ~0u;
	if (mine == ~0u) mine = next.fetch_add(1);
	return mine;
}

extern "C" nxz_ctx_t *nxz_ctx_create(int device)
{
	if (forked_child()) {
		snprintf(g_err, sizeof(g_err), "this process was forked after the engine was opened: the HIP runtime does not survive fork()");
		errno = ENODEV;
		return nullptr;
	}
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
		snprintf(g_err, sizeof(g_err), "no HIP device: the DEFLATE engine needs a gfx950 GPU (no CPU fallback)");
		errno = ENODEV;
		return nullptr;
	}
	if (device < 0) {
		const char *e = getenv("NXZ_DEVICE");
		if (e) device = atoi(e);
		else {
			static const bool spread = !(getenv("NXZ_DEVICE_POLICY") && !strcmp(getenv("NXZ_DEVICE_POLICY"), "current"));
			int cur = 0;
			(void)hipGetDevice(&cur);
			device = nxz_pick_device(-1, ndev < 64 ? ndev : 64, cur, calling_thread_index(), spread);
		}
	}
	if (device < 0 || device >= ndev || device >= 64) { errno = ENODEV; snprintf(g_err, sizeof(g_err), "device %d out of range", device); return nullptr; }
	std::lock_guard<std::mutex> g(g_mtx);
	if (g_ctx[device]) { g_ctx[device]->refs++; (void)hipSetDevice(device); return g_ctx[device]; }
	hipDeviceProp_t prop;
	HIPCHK(hipGetDeviceProperties(&prop, device), { errno = ENODEV; return nullptr; });
	if (!strstr(prop.gcnArchName, "gfx950")) {
		snprintf(g_err, sizeof(g_err), "device %d is %s: this engine is built for gfx950 only", device, prop.gcnArchName);
		errno = ENODEV;
		return nullptr;
	}
	HIPCHK(hipSetDevice(device), { errno = ENODEV; return nullptr; });
	nxz_ctx *c = new nxz_ctx();
	c->device = device;
	c->refs = 1;
	g_creator_pid = getpid();
	HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking), { delete c; errno = ENODEV; return nullptr; });
	g_ctx[device] = c;
	return c;
}

// (for the engine's other translation units: the HIP device of a context)
extern "C" int nxz_ctx_device(nxz_ctx_t *c) { return c ? c->device : -1; }

// the scratch of a stream that is about to be destroyed (its work is done) goes back to the device, and its entry away
static void drop_scratch(nxz_ctx *c, hipStream_t s)
{
	std::lock_guard<std::mutex> g(c->mtx);
	auto it = c->scratch.find(s);
	if (it != c->scratch.end()) { it->second.release(); c->scratch.erase(it); }
}

extern "C" void nxz_ctx_destroy(nxz_ctx_t *c)
{
	if (!c || forked_child()) return;                     // the parent owns the device objects
	std::lock_guard<std::mutex> g(g_mtx);
	if (--c->refs > 0) return;
	(void)hipSetDevice(c->device);
	for (auto &s : c->slots) if (s.stream) slot_free(s);
	for (auto &kv : c->scratch) kv.second.release();
	if (c->d_job_counters) (void)hipFree(c->d_job_counters);
	if (c->h_sample) (void)hipHostFree(c->h_sample);
	for (auto &l : c->lanes) {
		if (!l.stream) continue;
		(void)hipStreamSynchronize(l.stream);
		drop_scratch(c, l.stream);
		(void)hipFree(l.d_base); (void)hipHostFree(l.h_base);
		(void)hipStreamDestroy(l.stream);
		l = nxz_ctx::HostLane();
	}
	for (auto &m : c->merges) {
		if (!m.stream) continue;
		(void)hipStreamSynchronize(m.stream);
		drop_scratch(c, m.stream);
		(void)hipFree(m.d_base); (void)hipHostFree(m.h_base);
		(void)hipStreamDestroy(m.stream);
		m = nxz_ctx::Merge();
	}
	for (auto &r : c->rounds) {
		if (r.stream) { (void)hipStreamSynchronize(r.stream); (void)hipStreamDestroy(r.stream); }
		(void)hipHostFree(r.h_jobs); (void)hipHostFree(r.h_res); (void)hipHostFree(r.h_dht); (void)hipHostFree(r.h_cnt);
		(void)hipFree(r.d_prep); (void)hipFree(r.d_tok); (void)hipFree(r.d_cand2); (void)hipFree(r.d_src); (void)hipHostFree(r.h_items);
		r = nxz_ctx::Round();
	}
	if (c->split_stream) {
		(void)hipStreamSynchronize(c->split_stream); (void)hipStreamDestroy(c->split_stream);
		if (c->split_ev[0]) (void)hipEventDestroy(c->split_ev[0]);
		if (c->split_ev[1]) (void)hipEventDestroy(c->split_ev[1]);
	}
	if (c->stream) (void)hipStreamDestroy(c->stream);
	g_ctx[c->device] = nullptr;
	delete c;
}

extern "C" int nxz_ctx_sync(nxz_ctx_t *c, void *stream)
{
	hipStream_t s = (hipStream_t)stream;   // NULL = the HIP default stream
	HIPCHK(hipStreamSynchronize(s), return -EIO);
	return 0;
}

// a non-blocking stream whose priority goes round (low, normal, high) with `turn`: streams that are to run side by
// side -- rounds, the callers' streams of nxz_stream_create -- spread over the hardware queues of all three levels
hipError_t stream_create_spread(hipStream_t *s, unsigned turn)
{
	static const bool spread = !(getenv("NXZ_STREAM_PRIORITIES") && atoi(getenv("NXZ_STREAM_PRIORITIES")) == 0);
	int least = 0, greatest = 0;
	(void)hipDeviceGetStreamPriorityRange(&least, &greatest);
	const int prio = !spread ? 0 : turn % 3 == 0 ? 0 : turn % 3 == 1 ? greatest : least;
	return hipStreamCreateWithPriority(s, hipStreamNonBlocking, prio);
}

// Device memory, pinned host memory, streams and copies for callers that hold HOST buffers and do
// not link the HIP runtime themselves (cgo / JNI / ctypes hosts; libnxz_amd.so's blocked-gzip layer).
extern "C" void *nxz_dev_malloc(nxz_ctx_t *c, size_t bytes)
{
	void *p = nullptr;
	if (!c || hipSetDevice(c->device) != hipSuccess) return nullptr;
	HIPCHK(hipMalloc(&p, bytes ? bytes : 16), return nullptr);
	return p;
}
extern "C" void nxz_dev_free(nxz_ctx_t *c, void *p) { if (c && p) { (void)hipSetDevice(c->device); (void)hipFree(p); } }
extern "C" void *nxz_pinned_malloc(nxz_ctx_t *c, size_t bytes)
{
	void *p = nullptr;
	if (!c || hipSetDevice(c->device) != hipSuccess) return nullptr;
	HIPCHK(hipHostMalloc(&p, bytes ? bytes : 16), return nullptr);
	return p;
}
extern "C" void nxz_pinned_free(nxz_ctx_t *c, void *p) { if (c && p) { (void)hipSetDevice(c->device); (void)hipHostFree(p); } }
extern "C" void *nxz_stream_create(nxz_ctx_t *c)
{
	hipStream_t s = nullptr;
	if (!c || hipSetDevice(c->device) != hipSuccess) return nullptr;
	static std::atomic<unsigned> turn{0};
	HIPCHK(stream_create_spread(&s, turn.fetch_add(1)), return nullptr);
	return (void *)s;
}
extern "C" void nxz_stream_destroy(nxz_ctx_t *c, void *stream)
{
	if (!c || !stream) return;
	(void)hipSetDevice(c->device);
	(void)hipStreamSynchronize((hipStream_t)stream);
	drop_scratch(c, (hipStream_t)stream);
	(void)hipStreamDestroy((hipStream_t)stream);
}
extern "C" int nxz_copy_to_device(nxz_ctx_t *c, void *dst_dev, const void *src_host, size_t bytes, void *stream)
{
	if (!c) return -EINVAL;
	if (!bytes) return 0;
	HIPCHK(hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, (hipStream_t)stream), return -EIO);
	return 0;
}
// Measurement aid (bench.py's peak_measured): one device-to-device copy of `bytes` (a multiple of 16, both 16-byte aligned) by a
// 16-bytes-a-lane kernel, asynchronous on `stream`
extern "C" int nxz_copy_device(nxz_ctx_t *c, void *dst_dev, const void *src_dev, size_t bytes, void *stream)
{
	if (!c) return -EINVAL;
	(void)hipSetDevice(c->device);
	return nxz_launch_copy16(src_dev, dst_dev, bytes, (hipStream_t)stream) ? -EIO : 0;
}

extern "C" int nxz_copy_to_host(nxz_ctx_t *c, void *dst_host, const void *src_dev, size_t bytes, void *stream)
{
	if (!c) return -EINVAL;
	if (!bytes) return 0;
	HIPCHK(hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream), return -EIO);
	return 0;
}

// ---------------------------------------------------------------------------
// the reference's transport symbols
// ---------------------------------------------------------------------------
extern "C" uint64_t tb_freq = 512000000ull;

static uint64_t tb_now(void)
{
	struct timespec ts;
	clock_gettime(CLOCK_MONOTONIC, &ts);
	return (uint64_t)ts.tv_sec * 512000000ull + (uint64_t)ts.tv_nsec * 512ull / 1000ull;
}

extern "C" uint64_t nx_wait_ticks(uint64_t ticks, uint64_t accumulated, int do_sleep)
{
	uint64_t t0 = tb_now(), t1 = t0;
	if (do_sleep && accumulated > 110000) {
		uint64_t us = accumulated / 512;
		usleep(us > 1000 ? 1000 : (useconds_t)us);
		t1 = tb_now();
	} else {
		while (t1 - t0 <= ticks) t1 = tb_now();
	}
	return accumulated + (t1 - t0);
}

extern "C" int nx_function_begin(int function, int pri, void *handle)
{
	nxz_dev_t *h = (nxz_dev_t *)handle;
	if (function != NXZ_FUNC_COMP_GZIP || !h) { errno = EINVAL; return -1; }
	nxz_ctx_t *c = nxz_ctx_create(pri);
	if (!c) { if (!errno) errno = ENODEV; fprintf(stderr, "nxz: %s\n", g_err); return -1; }
	h->function = function;
	h->paste_addr = c;
	h->fd = c->device + 1;
	return 0;
}

extern "C" int nx_function_end(void *handle)
{
	nxz_dev_t *h = (nxz_dev_t *)handle;
	if (!h) return -1;
	if (h->paste_addr) nxz_ctx_destroy((nxz_ctx_t *)h->paste_addr);
	h->paste_addr = nullptr;
	h->fd = 0;
	return 0;
}

static Slot *slot_acquire(nxz_ctx *c)
{
	std::unique_lock<std::mutex> g(c->mtx);
	for (;;) {
		for (auto &s : c->slots) {
			if (!s.busy) {
				s.busy = true;
				if (!s.stream) {
					g.unlock();
					(void)hipSetDevice(c->device);
					bool ok = slot_init(s);
					if (!ok) slot_free(s);                        // nothing half built stays behind (the next caller starts over)
					g.lock();
					if (!ok) { s.busy = false; return nullptr; }
				}
				return &s;
			}
		}
		c->cv.wait(g);
	}
}

static void slot_release(nxz_ctx *c, Slot *s)
{
	{ std::lock_guard<std::mutex> g(c->mtx); s->busy = false; }
	c->cv.notify_one();
}

// gather `want` bytes starting `skip` bytes into the DDE list
static uint32_t dde_gather(const nxz_dde_t *d, uint32_t skip, uint8_t *dst, uint32_t want)
{
	uint32_t total = nxz_dde_bytes(d), cnt = nxz_dde_count(d), got = 0;
	if (cnt == 0) {
		if (skip >= total) return 0;
		uint32_t k = total - skip < want ? total - skip : want;
		memcpy(dst, (const uint8_t *)nxz_dde_addr(d) + skip, k);
		return k;
	}
	const nxz_dde_t *l = (const nxz_dde_t *)nxz_dde_addr(d);
	uint32_t off = 0;
	for (uint32_t i = 0; i < cnt && off < total && got < want; i++) {
		uint32_t k = nxz_dde_bytes(&l[i]);
		if (k > total - off) k = total - off;
		uint32_t lo = off, hi = off + k;
		if (hi > skip) {
			uint32_t from = lo > skip ? 0 : skip - lo;
			uint32_t take = k - from < want - got ? k - from : want - got;
			memcpy(dst + got, (const uint8_t *)nxz_dde_addr(&l[i]) + from, take);
			got += take;
		}
		off += k;
	}
	return got;
}

static uint32_t dde_capacity(const nxz_dde_t *d)
{
	uint32_t total = nxz_dde_bytes(d), cnt = nxz_dde_count(d), sum = 0;
	if (cnt == 0) return total;
	const nxz_dde_t *l = (const nxz_dde_t *)nxz_dde_addr(d);
	for (uint32_t i = 0; i < cnt; i++) sum += nxz_dde_bytes(&l[i]);
	return sum < total ? sum : total;
}

static void dde_scatter(const nxz_dde_t *d, const uint8_t *src, uint32_t n)
{
	uint32_t cnt = nxz_dde_count(d), off = 0;
	if (cnt == 0) { if (n) memcpy(nxz_dde_addr(d), src, n); return; }
	const nxz_dde_t *l = (const nxz_dde_t *)nxz_dde_addr(d);
	for (uint32_t i = 0; i < cnt && off < n; i++) {
		uint32_t k = nxz_dde_bytes(&l[i]);
		if (k > n - off) k = n - off;
		memcpy(nxz_dde_addr(&l[i]), src + off, k);
		off += k;
	}
}

static void put_cksums(nxz_crb_cpb_t *j, uint32_t crc, uint32_t adler)
{
	nxz_wr32(&j->cpb.out_adler_be, adler);
	j->cpb.out_crc_le = htole32(crc);
}

// NXZ_JOB_TRACE=1: where the time of the single-job interface goes, printed when the process ends
static struct JobTrace {
	std::atomic<uint64_t> jobs{0}, rounds{0}, ns_acquire{0}, ns_gather{0}, ns_wait{0}, ns_finish{0}, ns_issue{0}, ns_sync{0};
	bool on = false;
	JobTrace() { on = getenv("NXZ_JOB_TRACE") != nullptr; }
	~JobTrace()
	{
		if (!on || !jobs) return;
		const double j = (double)jobs, r = (double)(rounds ? rounds.load() : 1);
		fprintf(stderr, "nxz job trace: %llu compress jobs in %llu rounds (%.1f per round); per job: slot %.1f us, gather %.1f us, in the round %.1f us, "
			"scatter %.1f us; per round: launch calls %.1f us, synchronise %.1f us\n", (unsigned long long)jobs, (unsigned long long)rounds, j / r,
			ns_acquire / j * 1e-3, ns_gather / j * 1e-3, ns_wait / j * 1e-3, ns_finish / j * 1e-3, ns_issue / r * 1e-3, ns_sync / r * 1e-3);
	}
} g_trace;

// One caller's compress job on its way through a round.
struct CompressReq {
	uint32_t fc = 0;
	nxz_batch_job_t job;                  // src / dst: the caller's slot, pinned host memory the kernels work on in place
	const nxz_cpb_t *cpb = nullptr;       // the caller's table (DHT function codes)
	nxz_batch_result_t res;
	uint32_t cnt[316];
	int rc = 0;
	bool taken = false, done = false;
};
#define ROUND_MAX 32u

static void round_free(nxz_ctx::Round &r)
{
	if (r.stream) (void)hipStreamDestroy(r.stream);
	if (r.h_jobs) (void)hipHostFree(r.h_jobs);
	if (r.h_res) (void)hipHostFree(r.h_res);
	if (r.h_dht) (void)hipHostFree(r.h_dht);
	if (r.h_cnt) (void)hipHostFree(r.h_cnt);
	if (r.h_items) (void)hipHostFree(r.h_items);
	if (r.d_prep) (void)hipFree(r.d_prep);
	if (r.d_tok) (void)hipFree(r.d_tok);
	if (r.d_cand2) (void)hipFree(r.d_cand2);
	if (r.d_src) (void)hipFree(r.d_src);
	if (r.d_cut) (void)hipFree(r.d_cut);
	if (r.d_wg) (void)hipFree(r.d_wg);
	if (r.h_targets) (void)hipHostFree(r.h_targets);
	const bool busy = r.busy;                    // (the caller's claim on the round stands)
	r = nxz_ctx::Round();
	r.busy = busy;
}

static bool round_init(nxz_ctx::Round &r)
{
	if (r.ready) return true;
	static std::atomic<unsigned> round_turn{0};
	// (what a failed attempt got so far goes back: the next attempt would write over the pointers -- advisor, round 2)
	auto fail = [&]() { round_free(r); return false; };
	HIPCHK(stream_create_spread(&r.stream, round_turn.fetch_add(1)), return fail());
	HIPCHK(hipHostMalloc((void **)&r.h_jobs, ROUND_MAX * sizeof(nxz_batch_job_t)), return fail());
	HIPCHK(hipHostMalloc((void **)&r.h_res, ROUND_MAX * sizeof(nxz_batch_result_t)), return fail());
	HIPCHK(hipHostMalloc((void **)&r.h_dht, ROUND_MAX * sizeof(nxz_batch_dht_t)), return fail());
	HIPCHK(hipHostMalloc((void **)&r.h_cnt, ROUND_MAX * 316 * sizeof(uint32_t)), return fail());
	HIPCHK(hipMalloc((void **)&r.d_prep, ROUND_MAX * sizeof(nxz_dht_prepared_t)), return fail());
	HIPCHK(hipMalloc((void **)&r.d_tok, (size_t)ROUND_MAX * NXZ_TOK_STRIDE), return fail());
	HIPCHK(hipMalloc((void **)&r.d_cand2, nxz_lz77_cand2_bytes() / NXZ_LZ77_MAX_GRID * ROUND_MAX), return fail());
	HIPCHK(hipMalloc((void **)&r.d_src, (size_t)ROUND_MAX * SUBBLOCK), return fail());
	HIPCHK(hipHostMalloc((void **)&r.h_items, ROUND_MAX * sizeof(nxz_ctx::Round::Item)), return fail());
	r.ready = true;
	return true;
}

// The jobs of one round: a launch of each kernel for all of them.  Targets, job, table and result
// records are pinned host memory that the kernels read and write in place; the sources, which two
// kernels read (the second one in small pieces), are first brought over by a copy kernel (one
// workgroup per job, 16 bytes per lane straight from the callers' pinned staging).  No copy to
// queue, one synchronisation per round.
static int round_run(nxz_ctx *c, nxz_ctx::Round &R, std::vector<CompressReq *> &v)
{
	const uint32_t fc = v[0]->fc;
	const size_t n = v.size();
	const bool dht = nxz_fc_is_dht(fc), count = nxz_fc_has_count(fc), gen = nxz_fc_is_dhtgen(fc);
	(void)hipSetDevice(c->device);
	const uint64_t t0 = g_trace.on ? trace_ns() : 0;
	for (size_t k = 0; k < n; k++) {
		R.h_jobs[k] = v[k]->job;
		R.h_jobs[k].dht_index = (uint32_t)k;
		R.h_items[k].src = v[k]->job.src; R.h_items[k].dst = R.d_src + k * (size_t)SUBBLOCK; R.h_items[k].bytes = v[k]->job.src_len;
		R.h_jobs[k].src = R.h_items[k].dst;
		if (dht && !gen) {
			R.h_dht[k].dhtlen = nxz_in_dhtlen(v[k]->cpb);
			memcpy(R.h_dht[k].dht, v[k]->cpb->in_dht, NXZ_DHT_MAXSZ);
		}
	}
	static const bool each = getenv("NXZ_JOB_TRACE") && atoi(getenv("NXZ_JOB_TRACE")) > 1;   // 2: time every kernel on its own
	static std::atomic<uint64_t> kns[4];
	auto lap = [&](int i, uint64_t from) { if (each) { (void)hipStreamSynchronize(R.stream); kns[i] += trace_ns() - from; } };
	uint64_t k0 = each ? trace_ns() : 0;
	if (nxz_launch_copy_items(R.h_items, (uint32_t)n, R.stream)) return -EIO;
	if (dht && !gen && nxz_launch_dht_prepare(R.h_dht, n, R.d_prep, R.stream)) return -EIO;
	lap(0, k0); k0 = each ? trace_ns() : 0;
	const bool fused = !dht && !count && !gen;             // the fixed code: the LZ77 kernel writes the block itself
	if (nxz_launch_lz77(fused ? NXZ_LZ77_FUSED_FHT : count || gen, R.h_jobs, n, R.d_tok, R.d_cand2, R.h_res, R.h_cnt, nullptr, R.stream)) return -EIO;
	lap(1, k0); k0 = each ? trace_ns() : 0;
	if (gen && nxz_launch_dhtgen(R.h_cnt, n, R.d_prep, nullptr, R.stream)) return -EIO;
	lap(2, k0); k0 = each ? trace_ns() : 0;
	if (!fused && nxz_launch_encode(dht, gen, R.h_jobs, n, R.d_tok, R.d_prep, R.h_res, R.stream)) return -EIO;
	lap(3, k0);
	if (each && (g_trace.rounds & 255) == 255)
		fprintf(stderr, "nxz round kernels (sum so far, us): dht_prepare %.0f lz77 %.0f dhtgen %.0f encode %.0f over %llu rounds\n",
			kns[0] * 1e-3, kns[1] * 1e-3, kns[2] * 1e-3, kns[3] * 1e-3, (unsigned long long)g_trace.rounds + 1);
	const uint64_t t1 = g_trace.on ? trace_ns() : 0;
	HIPCHK(hipStreamSynchronize(R.stream), return -EIO);
	if (g_trace.on) { g_trace.rounds++; g_trace.ns_issue += t1 - t0; g_trace.ns_sync += trace_ns() - t1; }
	for (size_t k = 0; k < n; k++) {
		v[k]->res = R.h_res[k];
		if (count) memcpy(v[k]->cnt, R.h_cnt + k * 316, sizeof(v[k]->cnt));
	}
	return 0;
}

// A round that is free, as long as fewer than NXZ_ROUNDS (default 6) are in flight: few rounds in flight
// make the callers that arrive meanwhile wait and go out TOGETHER, which is what the device wants (it
// runs only a handful of small launches side by side); c->qm is held.
static nxz_ctx::Round *free_round(nxz_ctx *c, bool inflate = false)
{
	// (decompress rounds are a dozen dependent launches each where a compress round is four: three of them in flight serve
	// sixteen and sixty-four threads of 64 KiB calls best -- 1.07 / 2.0 GiB/s against 0.89 / 1.7 with six; NXZ_ROUNDS_INFLATE)
	static const unsigned limit_c = [] { const char *e = getenv("NXZ_ROUNDS"); unsigned v = e ? (unsigned)atoi(e) : 6; return v < 1 ? 1u : v > 16 ? 16u : v; }();
	static const unsigned limit_i = [] { const char *e = getenv("NXZ_ROUNDS_INFLATE"); unsigned v = e ? (unsigned)atoi(e) : getenv("NXZ_ROUNDS") ? (unsigned)atoi(getenv("NXZ_ROUNDS")) : 3; return v < 1 ? 1u : v > 16 ? 16u : v; }();
	const unsigned limit = inflate ? limit_i : limit_c;
	unsigned busy = 0;
	nxz_ctx::Round *f = nullptr;
	for (auto &r : c->rounds) { if (r.busy) busy++; else if (!f) f = &r; }
	return busy < limit ? f : nullptr;
}

// Queue the job; whoever finds a free round takes the job at the head of the queue and every queued
// job with the same function code, runs them, and wakes their owners.  The first caller goes out
// alone at once; those that arrive while it is in flight form the next round.
static int round_submit(nxz_ctx *c, CompressReq *me)
{
	std::unique_lock<std::mutex> lk(c->qm);
	c->q.push_back(me);
	while (!me->done) {
		nxz_ctx::Round *R = nullptr;
		if (!me->taken) R = free_round(c);
		if (!R) { c->qcv.wait(lk); continue; }
		R->busy = true;
		std::vector<CompressReq *> v;
		const uint32_t fc = c->q.front()->fc;
		for (auto it = c->q.begin(); it != c->q.end() && v.size() < ROUND_MAX; ) {
			if ((*it)->fc == fc) { (*it)->taken = true; v.push_back(*it); it = c->q.erase(it); }
			else ++it;
		}
		lk.unlock();
		(void)hipSetDevice(c->device);
		int rc = round_init(*R) ? round_run(c, *R, v) : -ENOMEM;
		if (rc && R->stream) (void)hipStreamSynchronize(R->stream);   // nothing of a failed round may still be in flight
		lk.lock();
		for (auto *r : v) { r->rc = rc; r->done = true; }
		R->busy = false;
		c->qcv.notify_all();
	}
	return me->rc;
}

static int run_compress(nxz_ctx *c, Slot *s, nxz_crb_cpb_t *j, uint32_t fc)
{
	uint32_t srctotal = nxz_dde_bytes(&j->crb.source);
	uint32_t hist = nxz_fc_is_resume(fc) ? nxz_in_histlen(&j->cpb) * 16 : 0;
	if (hist > srctotal) hist = srctotal;
	// only the last 32 KiB of history can be referenced (inc_nx/nxu.h:303-317)
	uint32_t skip = hist > 32768 ? hist - 32768 : 0;
	uint32_t h = hist - skip;
	uint32_t n = srctotal - hist;
	bool partial = false;
	if (h + n > SUBBLOCK) { n = SUBBLOCK - h; partial = true; }     // byte-count limit -> CC 3 partial
	const uint64_t t0 = g_trace.on ? trace_ns() : 0;
	uint32_t got = dde_gather(&j->crb.source, skip, s->h_in, h + n);
	if (got < h) { h = got; n = 0; } else n = got - h;
	uint32_t cap = dde_capacity(&j->crb.target);
	uint32_t dcap = cap < OUT_CAP ? cap & ~3u : OUT_CAP;
	if (cap < 4) dcap = 0;
	const bool count = nxz_fc_has_count(fc);

	CompressReq req;
	req.fc = fc;
	req.cpb = &j->cpb;
	memset(&req.job, 0, sizeof(req.job));
	req.job.src = s->h_in; req.job.dst = s->h_out; req.job.src_len = h + n; req.job.hist_len = h;
	req.job.dst_cap = dcap; req.job.in_crc = nxz_in_crc(&j->cpb); req.job.in_adler = nxz_in_adler(&j->cpb);
	const uint64_t t1 = g_trace.on ? trace_ns() : 0;
	int rc = round_submit(c, &req);
	if (rc) return rc;
	const uint64_t t2 = g_trace.on ? trace_ns() : 0;

	const nxz_batch_result_t r = req.res;
	uint32_t cc = r.cc, ce = 0, tpbc = 0;
	if (cc == NXZ_CC_TARGET_SPACE || cc == NXZ_CC_MISSING_CODE || cc == NXZ_CC_INVALID_DHT) {
		ce = NXZ_CE_TERMINATE;
	} else {
		tpbc = r.tpbc;
		if (tpbc > cap) { cc = NXZ_CC_TARGET_SPACE; ce = NXZ_CE_TERMINATE; tpbc = 0; }
	}
	if (ce != NXZ_CE_TERMINATE) {
		dde_scatter(&j->crb.target, s->h_out, tpbc);
		nxz_putf(&j->cpb.out_w2_be, 16, 3, r.tebc);
		put_cksums(j, r.crc, r.adler);
		uint32_t spbc = skip + r.spbc;
		if (count) {
			for (int i = 0; i < 316; i++) nxz_wr32(&j->cpb.u.out_lzcount_be[i], req.cnt[i]);
			nxz_wr32(&j->cpb.out_spbc_with_count_be, spbc);
		} else {
			nxz_wr32(&j->cpb.u.out_spbc_be, spbc);
		}
		if (cc == 0 && partial) { cc = NXZ_CC_DATA_LENGTH; ce = NXZ_CE_PARTIAL | NXZ_CE_TPBC_VALID; }
	}
	nxz_csb_complete(j, cc, ce, tpbc);
	if (g_trace.on) { g_trace.jobs++; g_trace.ns_gather += t1 - t0; g_trace.ns_wait += t2 - t1; g_trace.ns_finish += trace_ns() - t2; }
	return 0;
}

static int run_wrap(nxz_ctx *c, Slot *s, nxz_crb_cpb_t *j)
{
	uint32_t n = nxz_dde_bytes(&j->crb.source), cap = dde_capacity(&j->crb.target);
	if (n > INF_SRC_CAP) n = INF_SRC_CAP;
	if (n > cap) { nxz_csb_complete(j, NXZ_CC_TARGET_SPACE, NXZ_CE_TERMINATE, 0); return 0; }
	n = dde_gather(&j->crb.source, 0, s->h_in, n);
	nxz_batch_job_t *bj = s->h_job;
	memset(bj, 0, sizeof(*bj));
	bj->src = s->d_in; bj->dst = s->d_out; bj->src_len = n; bj->dst_cap = INF_OUT_CAP;
	HIPCHK(hipMemcpyAsync(s->d_in, s->h_in, n, hipMemcpyHostToDevice, s->stream), return -EIO);
	HIPCHK(hipMemcpyAsync(s->d_job, bj, sizeof(*bj), hipMemcpyHostToDevice, s->stream), return -EIO);
	if (nxz_launch_wrap_sliced(s->d_job, 1, s->d_res, s->stream)) return -EIO;
	HIPCHK(hipMemcpyAsync(s->h_res, s->d_res, sizeof(nxz_batch_result_t), hipMemcpyDeviceToHost, s->stream), return -EIO);
	HIPCHK(hipMemcpyAsync(s->h_out, s->d_out, n, hipMemcpyDeviceToHost, s->stream), return -EIO);
	HIPCHK(hipStreamSynchronize(s->stream), return -EIO);
	dde_scatter(&j->crb.target, s->h_out, n);
	put_cksums(j, s->h_res->crc, s->h_res->adler);
	nxz_wr32(&j->cpb.u.out_spbc_be, n);
	nxz_csb_complete(j, s->h_res->cc, 0, n);
	return 0;
}

// One caller's decompress job on its way through a round (the rounds of the compress jobs, above: the
// callers that arrive while a launch is in flight go out together -- here as one launch of the
// stream-per-wave inflate kernel with a wavefront per job, instead of a launch per job on a stream of
// its own, of which the device runs only a few at a time).
struct InflateReq {
	uint8_t *d_out = nullptr;             // the slot's device buffer for the output (rounds that cut the streams into pieces decode into it)
	nxz_batch_job_t job;                  // src: the slot's device buffer (filled by the round's copy kernel from h_in); dst: the slot's pinned h_out
	const uint8_t *h_in = nullptr;        // the slot's pinned staging of the source
	nxz_batch_dht_t *dht = nullptr;       // the slot's pinned table: in when the job resumes inside a dynamic block, out when it suspends in one
	nxz_batch_result_t res;
	int rc = 0;
	bool taken = false, done = false;
};

static int round_run_inflate(nxz_ctx *c, nxz_ctx::Round &R, std::vector<InflateReq *> &v)
{
	const size_t n = v.size();
	(void)hipSetDevice(c->device);
	for (size_t k = 0; k < n; k++) {
		R.h_jobs[k] = v[k]->job;
		R.h_items[k].src = v[k]->h_in; R.h_items[k].dst = (uint8_t *)v[k]->job.src; R.h_items[k].bytes = v[k]->job.src_len;
		R.h_dht[k] = *v[k]->dht;
	}
	// A wavefront per job takes 0.6-3 ms for 64 KiB however few jobs there are.  Jobs of a few KiB and more are cut into
	// pieces instead (nxz_inflate_cut.hip: 16 streams of 64 KiB 1.0-1.4 GiB/s against 0.2-0.3); those decode into the slots'
	// device buffers -- the pieces' elements are resolved against what is already there, which pinned host memory is too
	// far away for -- and one more kernel takes the outputs to the callers' pinned targets.  NXZ_ROUND_CUT=0: never.
	static const bool cut_on = !(getenv("NXZ_ROUND_CUT") && atoi(getenv("NXZ_ROUND_CUT")) == 0);
	bool cut = cut_on;
	if (cut) {
		size_t longish = 0;
		for (size_t k = 0; k < n; k++) {
			const nxz_batch_job_t &j = v[k]->job;
			// (long enough, and standing where a stream can be cut: at a block header or inside a dynamic block)
			const uint32_t sfbt = (j.resume >> 16) & 15;
			if (j.src_len - (j.hist_len < j.src_len ? j.hist_len : j.src_len) >= 4096 && v[k]->d_out && (sfbt == 0 || (sfbt & 0xe) == 0xe || (sfbt & 0xe) == 0xc)) longish++;
		}
		cut = longish > 0;
	}
	// A round of fresh streams -- what nx_uncompress / inflate(Z_FINISH) of whole buffers are -- goes a stream per WORKGROUP
	// (nxz_inflate_wg.hip: 0.2-0.4 ms for buffers of 64 KiB whatever the round holds, 0.8 ms for 256 KiB, one launch; what that
	// kernel hands back -- a stream that ends early, a target that is too small -- goes a wavefront each behind it).
	// NXZ_ROUND_WG=0: never; NXZ_ROUND_WG_MAX: source bytes of a job at most.
	static const bool wg_on = !(getenv("NXZ_ROUND_WG") && atoi(getenv("NXZ_ROUND_WG")) == 0);
	static const uint32_t wg_src_max = getenv("NXZ_ROUND_WG_MAX") ? (uint32_t)strtoul(getenv("NXZ_ROUND_WG_MAX"), nullptr, 0) : 400000u;
	bool wg = wg_on;
	for (size_t k = 0; k < n && wg; k++) {
		const nxz_batch_job_t &j = v[k]->job;
		if (j.resume || j.hist_len || j.src_len > wg_src_max || !v[k]->d_out) wg = false;
	}
	if (wg && !R.h_targets && hipHostMalloc((void **)&R.h_targets, ROUND_MAX * sizeof(uint8_t *)) != hipSuccess) { (void)hipGetLastError(); R.h_targets = nullptr; wg = false; }
	if (wg && !R.d_wg && hipMalloc((void **)&R.d_wg, nxz_inflate_wg_workspace(ROUND_MAX)) != hipSuccess) { (void)hipGetLastError(); R.d_wg = nullptr; wg = false; }
	const unsigned P = 32;
	if (wg) cut = false;
	if (cut && !R.d_cut) {
		const size_t arena = (size_t)96 << 20;
		if (hipMalloc((void **)&R.d_cut, nxz_inflate_cut_workspace(ROUND_MAX, P, arena)) != hipSuccess || (!R.h_targets && hipHostMalloc((void **)&R.h_targets, ROUND_MAX * sizeof(uint8_t *)) != hipSuccess)) {
			(void)hipGetLastError();
			if (R.d_cut) (void)hipFree(R.d_cut);
			R.d_cut = nullptr; cut = false;
		} else R.cut_arena = arena;
	}
	// (the sources to the device buffers -- except for a round that goes a stream per workgroup: that kernel reads a stream once,
	// 16 bytes a lane, and does so straight from the callers' pinned staging; and its checksum pass takes the outputs to the
	// pinned targets as it reads them: two launches a round less, 158 -> 145 us for a call of 64 KiB)
	if (!wg && nxz_launch_copy_items(R.h_items, (uint32_t)n, R.stream)) return -EIO;
	if (wg) {
		for (size_t k = 0; k < n; k++) { R.h_targets[k] = R.h_jobs[k].dst; R.h_jobs[k].dst = v[k]->d_out; R.h_jobs[k].src = v[k]->h_in; }
		if (nxz_launch_inflate_wg(R.h_jobs, n, R.h_res, R.h_dht, R.d_wg, nullptr, R.h_targets, R.stream)) return -EIO;
	} else if (cut) {
		for (size_t k = 0; k < n; k++) { R.h_targets[k] = R.h_jobs[k].dst; R.h_jobs[k].dst = v[k]->d_out; }
		if (nxz_launch_inflate_cut(R.h_jobs, n, R.h_res, R.h_dht, P, R.d_cut, R.cut_arena, R.stream)) return -EIO;
		if (nxz_launch_copy_out(R.h_jobs, R.h_res, R.h_targets, n, R.stream)) return -EIO;
	} else if (nxz_launch_inflate(R.h_jobs, n, R.h_res, R.h_dht, 1, nullptr, R.stream)) return -EIO;
	HIPCHK(hipStreamSynchronize(R.stream), return -EIO);
	for (size_t k = 0; k < n; k++) {
		v[k]->res = R.h_res[k];
		if ((R.h_res[k].sfbt & 0xe) == 0xc) *v[k]->dht = R.h_dht[k];
	}
	return 0;
}

static int round_submit_inflate(nxz_ctx *c, InflateReq *me)
{
	std::unique_lock<std::mutex> lk(c->qm);
	c->qi.push_back(me);
	while (!me->done) {
		nxz_ctx::Round *R = nullptr;
		if (!me->taken) R = free_round(c, true);
		if (!R) { c->qcv.wait(lk); continue; }
		R->busy = true;
		std::vector<InflateReq *> v;
		while (!c->qi.empty() && v.size() < ROUND_MAX) { c->qi.front()->taken = true; v.push_back(c->qi.front()); c->qi.pop_front(); }
		lk.unlock();
		(void)hipSetDevice(c->device);
		int rc = round_init(*R) ? round_run_inflate(c, *R, v) : -ENOMEM;
		if (rc && R->stream) (void)hipStreamSynchronize(R->stream);
		lk.lock();
		for (auto *r : v) { r->rc = rc; r->done = true; }
		R->busy = false;
		c->qcv.notify_all();
	}
	return me->rc;
}

static int run_decompress(nxz_ctx *c, Slot *s, nxz_crb_cpb_t *j, uint32_t fc)
{
	uint32_t srctotal = nxz_dde_bytes(&j->crb.source);
	bool resume = nxz_fc_is_resume(fc);
	uint32_t hist = resume ? nxz_in_histlen(&j->cpb) * 16 : 0;
	if (hist > srctotal) hist = srctotal;
	uint32_t take = srctotal > INF_SRC_CAP ? INF_SRC_CAP : srctotal;
	if (take < hist) take = hist;
	uint32_t got = dde_gather(&j->crb.source, 0, s->h_in, take);
	if (got < hist) hist = got;
	uint32_t cap = dde_capacity(&j->crb.target);
	uint32_t dcap = cap < INF_OUT_CAP ? cap : INF_OUT_CAP;
	InflateReq req;
	nxz_batch_job_t *bj = &req.job;
	memset(bj, 0, sizeof(*bj));
	bj->src = s->d_in; bj->dst = s->h_out; bj->src_len = got; bj->hist_len = hist; bj->dst_cap = dcap;
	bj->in_crc = nxz_in_crc(&j->cpb); bj->in_adler = nxz_in_adler(&j->cpb);
	bj->reserved = nxz_rd32(&j->crb.reserved1) & NXZ_JOB_SUSPEND_WHEN_FULL;
	s->h_dht->dhtlen = 0;
	if (resume) {
		uint32_t sfbt = nxz_in_sfbt(&j->cpb);
		bj->resume = (sfbt << 16) | (nxz_in_subc(&j->cpb) << 20);
		if ((sfbt & 0xe) == 0x8) bj->resume |= nxz_in_rembytecnt(&j->cpb);
		if ((sfbt & 0xe) == 0xc) {
			s->h_dht->dhtlen = nxz_in_dhtlen(&j->cpb);
			memcpy(s->h_dht->dht, j->cpb.in_dht, NXZ_DHT_MAXSZ);
		}
	}
	req.h_in = s->h_in; req.dht = s->h_dht; req.d_out = s->d_out;
	const uint64_t td0 = g_trace.on ? trace_ns() : 0;
	{
		const int rrc = round_submit_inflate(c, &req);
		if (rrc) return rrc;
	}
	nxz_batch_result_t r = req.res;
	if (g_trace.on) {
		static std::atomic<uint64_t> dj{0}, dns{0}, din{0}, dout{0};
		dj++; dns += trace_ns() - td0; din += got; dout += r.tpbc;
		if ((dj & 4095) == 0) fprintf(stderr, "nxz decompress jobs: %llu, %.1f us each in the round, %.0f source bytes in, %.0f bytes out each\n",
					      (unsigned long long)dj, dns / (double)dj * 1e-3, din / (double)dj, dout / (double)dj);
	}
	uint32_t cc = r.cc, ce = 0, tpbc = 0;
	if (cc != 0 && cc != NXZ_CC_DATA_LENGTH) {
		ce = NXZ_CE_TERMINATE;
	} else {
		tpbc = r.tpbc;
		uint32_t sfbt = r.sfbt & 0xf;
		dde_scatter(&j->crb.target, s->h_out, tpbc);
		put_cksums(j, r.crc, r.adler);
		nxz_wr32(&j->cpb.out_w2_be, r.subc & 0xffff);
		nxz_wr32(&j->cpb.out_w3_be, 0);
		nxz_putf(&j->cpb.out_w3_be, 16, 4, sfbt);
		if ((sfbt & 0xe) == 0x8) nxz_putf(&j->cpb.out_w3_be, 0, 16, r.tebc);
		else if ((sfbt & 0xe) == 0xc) {
			nxz_putf(&j->cpb.out_w3_be, 0, 12, s->h_dht->dhtlen);
			memset(j->cpb.u.d.out_dht, 0, NXZ_DHT_MAXSZ);
			memcpy(j->cpb.u.d.out_dht, s->h_dht->dht, (s->h_dht->dhtlen + 7) / 8);
		}
		nxz_wr32(&j->cpb.u.d.out_spbc_decomp_be, r.spbc);
		if (cc == NXZ_CC_DATA_LENGTH) ce = NXZ_CE_PARTIAL | NXZ_CE_TPBC_VALID;
	}
	nxz_csb_complete(j, cc, ce, tpbc);
	return 0;
}

extern "C" int nxu_run_job(nxz_crb_cpb_t *j, void *handle)
{
	nxz_dev_t *h = (nxz_dev_t *)handle;
	nxz_ctx *c = h ? (nxz_ctx *)h->paste_addr : nullptr;
	if (!j) return -EINVAL;
	if (!c || forked_child()) { nxz_csb_complete(j, NXZ_CC_NO_HW, NXZ_CE_TERMINATE, 0); return 0; }
	uint32_t fc = nxz_fc(j);
	const uint64_t ta = g_trace.on ? trace_ns() : 0;
	Slot *s = slot_acquire(c);
	if (!s) { nxz_csb_complete(j, NXZ_CC_NO_HW, NXZ_CE_TERMINATE, 0); return 0; }
	if (g_trace.on) g_trace.ns_acquire += trace_ns() - ta;
	if (fc == NXZ_FC_WRAP) (void)hipSetDevice(c->device);     // (compress and decompress jobs: the thread that runs the round does)
	int rc;
	if (fc == NXZ_FC_WRAP) rc = run_wrap(c, s, j);
	else if (nxz_fc_is_compress(fc) && !(fc & 1) && !(fc & ~0x2eu) && (!nxz_fc_is_dhtgen(fc) || nxz_fc_is_dht(fc))) rc = run_compress(c, s, j, fc);
	else if (fc == NXZ_FC_DECOMPRESS || fc == NXZ_FC_DECOMPRESS_RESUME) rc = run_decompress(c, s, j, fc);
	else { nxz_csb_complete(j, NXZ_CC_INVALID_OP, NXZ_CE_TERMINATE, 0); rc = 0; }
	if (rc) (void)hipStreamSynchronize(s->stream);            // nothing of a failed job may still be in flight when the slot is reused
	slot_release(c, s);
	if (rc) { fprintf(stderr, "nxz: job failed: %s\n", g_err); return -EAGAIN; }
	return 0;
}

// ---------------------------------------------------------------------------
// __crc32_vpmsum: raw CRC-32 register update (no pre/post inversion), slice-by-8
// ---------------------------------------------------------------------------
static uint32_t crc_t[8][256];
static std::once_flag crc_once;
static void crc_tables(void)
{
	for (uint32_t i = 0; i < 256; i++) {
		uint32_t c = i;
		for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((c & 1) ? 0xedb88320u : 0);
		crc_t[0][i] = c;
	}
	for (uint32_t i = 0; i < 256; i++)
		for (int k = 1; k < 8; k++) crc_t[k][i] = crc_t[0][crc_t[k - 1][i] & 0xff] ^ (crc_t[k - 1][i] >> 8);
}

extern "C" unsigned int __crc32_vpmsum(unsigned int crc, const unsigned char *p, unsigned long len)
{
	std::call_once(crc_once, crc_tables);
	while (len && ((uintptr_t)p & 7)) { crc = crc_t[0][(crc ^ *p++) & 0xff] ^ (crc >> 8); len--; }
	while (len >= 8) {
		uint64_t v; memcpy(&v, p, 8);
		v = le64toh(v) ^ crc;
		crc = crc_t[7][v & 0xff] ^ crc_t[6][(v >> 8) & 0xff] ^ crc_t[5][(v >> 16) & 0xff] ^ crc_t[4][(v >> 24) & 0xff] ^
		      crc_t[3][(v >> 32) & 0xff] ^ crc_t[2][(v >> 40) & 0xff] ^ crc_t[1][(v >> 48) & 0xff] ^ crc_t[0][v >> 56];
		p += 8; len -= 8;
	}
	while (len--) crc = crc_t[0][(crc ^ *p++) & 0xff] ^ (crc >> 8);
	return crc;
}
