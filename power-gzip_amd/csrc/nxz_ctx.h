// nxz_ctx.h -- what the host sources of libnxz_engine.so share (nxz_engine.cpp, nxz_batch.cpp, nxz_batch_framed.cpp,
// nxz_batch_streams.cpp, nxz_batch_ranges.cpp, nxz_deflate_host.cpp): the context, a stream's scratch with its buffer type and the rules for touching it, and a few helpers.  Private: not installed.
#ifndef NXZ_CTX_H
#define NXZ_CTX_H
#include <hip/hip_runtime.h>
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <map>
#include <deque>
#include <mutex>
#include <new>
#include <type_traits>
#include <vector>
#include "nxz_device.h"
#include "nxz_dict.h"
#include "../../include/nxz_wire.h"

#define SUBBLOCK 65536u
#define SLOTS 32

void set_err(const char *what, hipError_t e);              // the calling thread's nxz_last_error() (nxz_engine.cpp)
#define HIPCHK(x, fail) do { hipError_t e_ = (x); if (e_ != hipSuccess) { set_err(#x, e_); fail; } } while (0)
// what a batched call returns for the status `rc` of one of its launches (nxz_launch_*): 0, or -EIO with `what` in nxz_last_error()
static inline int launched(const char *what, int rc)
{
	if (rc) { set_err(what, (hipError_t)rc); return -EIO; }
	return 0;
}

// one in-flight single job (nxu_run_job)
struct Slot {
	hipStream_t stream = nullptr;
	uint8_t *h_in = nullptr, *h_out = nullptr;      // pinned
	uint8_t *d_in = nullptr, *d_out = nullptr;
	nxz_batch_job_t *h_job = nullptr, *d_job = nullptr;
	nxz_batch_result_t *h_res = nullptr, *d_res = nullptr;
	nxz_batch_dht_t *h_dht = nullptr, *d_dht = nullptr;
	nxz_dht_prepared_t *d_prep = nullptr;
	uint32_t *h_cnt = nullptr, *d_cnt = nullptr;
	bool busy = false;
};

// A grow-only device buffer of a stream's scratch.  Plain data without a destructor: a Scratch is copied by value and lives
// in a std::map; Scratch::release() frees it.
struct DevBuf {
	uint8_t *p = nullptr;
	size_t cap = 0;                               // bytes
	enum Grown { FAILED = -1, KEPT = 0, NEW = 1 };
	// what is there goes back to the device, after the launches on `s` that may still read it
	void drop(hipStream_t s)
	{
		if (p) { (void)hipStreamSynchronize(s); (void)hipFree(p); }
		p = nullptr; cap = 0;
	}
	// Room for `need` bytes.  KEPT: there was (nothing changed).  NEW: a fresh allocation of `need` bytes, its contents
	// undefined -- whoever keeps state in the buffer starts over.  FAILED: no buffer at all (p = nullptr, cap = 0), the
	// reason in nxz_last_error() and HIP's sticky error cleared; for a required buffer the caller returns -ENOMEM, an
	// optional one it does without.
	Grown grow(hipStream_t s, size_t need)
	{
		if (cap >= need) return KEPT;
		drop(s);
		const hipError_t e = hipMalloc((void **)&p, need);
		if (e != hipSuccess) { (void)hipGetLastError(); p = nullptr; set_err("hipMalloc of a stream's scratch", e); return FAILED; }
		cap = need;
		return NEW;
	}
	template <class T> T *as() const { return (T *)p; }
};
// the grow-only buffers of a stream's scratch (nxz_ctx::Scratch::buf)
enum ScratchBuf {
	BUF_PREPARED,       // nxz_batch_compress with the caller's tables: their prepared forms
	BUF_LANES,          // per-lane decode tables of the batched inflate kernel
	BUF_ORDER,          // the jobs' order by length for the stream-per-wave kernel's larger batches
	BUF_CUT,            // small inflate batches cut into pieces (nxz_inflate_cut.hip): control arrays + the pieces' elements
	BUF_WG,             // a stream per workgroup (nxz_inflate_wg.hip): job counter, reasons, hand-back list
	BUF_FRAME_JOBS,     // nxz_batch_decompress_framed: the derived raw jobs (the deflate bytes of each stream)
	BUF_DICT_JOBS,      // nxz_batch_compress_dict: the caller's jobs with the dictionary's window "in front"
	BUF_BGZF,           // nxz_batch_unpack_gzip: the discovery's candidates, jump tables and the members' jobs
	BUF_RNG,            // nxz_bgzf_read_ranges: the map's per-range and per-member arrays
	BUF_RNG_SLOTS,      // ... a chunk of decoded members (16-byte aligned slots), their jobs, frames and results
	BUF_RNG_BATCH,      // nxz_batch_checkpoint_read_ranges: the rows' verdicts and bases, the flat uoff, the ranges mapped onto it
	BUF_STREAMS,        // nxz_batch_streams.cpp (the layouts are carved there, nxz_streams_plan.h's nxz_carve); nxz_batch_deflate_streams and its forms: descriptors, block prefix and state of the streams; jobs, results, owners, offsets and output slots of a chunk; nxz_batch_inflate_streams_part: descriptors and slot offsets; work, jobs, results, table slots and staging slots of a chunk
	BUF_GZIP_MEMBERS,   // nxz_batch_gzip_members_decode: the per-job plan, and the members as framed jobs with their owners, frames and results
	BUF_COUNT
};

constexpr int HOST_PAIRS = 16;
struct nxz_ctx {
	int device = 0;
	int refs = 0;
	hipStream_t stream = nullptr;                 // default stream for batch calls
	std::mutex mtx;
	std::condition_variable cv;
	Slot slots[SLOTS];
	// batch scratch, one set per stream the caller launches on: launches on different streams may
	// run at the same time, so they must not share the prepared tables or the decode workspace
	uint32_t *h_sample = nullptr;                 // pinned words the block-type sample of a large inflate batch lands in
	unsigned sample_turn = 0;
	struct Scratch {
		DevBuf buf[BUF_COUNT];                    // the grow-only buffers (ScratchBuf above)
		uint64_t bgzf_cap = 0;                    // candidates buf[BUF_BGZF] has room for
		// compress: what the LZ77 kernel hands to the entropy kernel, for one chunk of jobs
		uint8_t *d_tokens = nullptr;              // chunk x NXZ_TOK_STRIDE
		nxz_dht_prepared_t *d_gen = nullptr;      // tables the device generated, one per job of the chunk
		uint32_t *d_counts = nullptr;             // symbol counts when the caller did not ask for them
		uint16_t *d_cand2 = nullptr;              // LZ77 kernel: second bucket entries in transit, 32 KiB per workgroup
		uint8_t *d_fuse = nullptr;                // the fused dynamic-Huffman form: two token slots and two table slots per workgroup (nxz_lz77.hip gen::)
		size_t chunk_cap = 0;
		size_t chunk_limit = 0;                   // jobs per chunk the device had room for when a larger chunk could not be had (0: no such failure yet)
		// nxz_batch_deflate_streams: pinned staging for the descriptors and the block prefix, two of them in turn -- a call returns
		// before its upload has run, so the next call fills the other one; up_ev[k] is recorded behind the upload from h_up[k]
		uint8_t *h_up[2] = { nullptr, nullptr };
		size_t h_up_cap[2] = { 0, 0 };
		hipEvent_t up_ev[2] = { nullptr, nullptr };
		unsigned up_turn = 0;
		void release_chunk() {
			if (d_tokens) (void)hipFree(d_tokens);                       // (d_gen and d_counts lie inside it)
			d_tokens = nullptr; d_gen = nullptr; d_counts = nullptr; chunk_cap = 0;
		}
		// the three buffers of a chunk, all or none
		bool alloc_chunk(size_t chunk) {
			// (one allocation: the tokens, then the tables, then the counts)
			const size_t tb = (chunk * (size_t)NXZ_TOK_STRIDE + 255) & ~(size_t)255, gb = (chunk * sizeof(nxz_dht_prepared_t) + 255) & ~(size_t)255;
			if (hipMalloc((void **)&d_tokens, tb + gb + chunk * 316 * sizeof(uint32_t)) == hipSuccess) {
				d_gen = (nxz_dht_prepared_t *)(d_tokens + tb);
				d_counts = (uint32_t *)(d_tokens + tb + gb);
				chunk_cap = chunk;
				return true;
			}
			(void)hipGetLastError();
			d_tokens = nullptr; d_gen = nullptr; d_counts = nullptr;
			return false;
		}
		void release() {
			for (DevBuf &b : buf) if (b.p) (void)hipFree(b.p);
			if (d_tokens) (void)hipFree(d_tokens);                       // (d_gen and d_counts lie inside it)
			if (d_cand2) (void)hipFree(d_cand2);
			if (d_fuse) (void)hipFree(d_fuse);
			for (int k = 0; k < 2; k++) {
				if (h_up[k]) (void)hipHostFree(h_up[k]);
				if (up_ev[k]) (void)hipEventDestroy(up_ev[k]);
			}
			*this = Scratch();
		}
	};
	std::map<hipStream_t, Scratch> scratch;
	std::map<hipStream_t, std::mutex> scratch_use;   // held by a batch call from sizing its stream's scratch to its last launch
	std::map<hipStream_t, std::mutex> frame_use;     // held by a framed call from its header kernel to its trailer kernel (the derived jobs)
	// nxz_deflate_host: a call works on two lanes, each with its own stream, so that the copies of one group of
	// blocks run while the other group is in the kernels; HOST_PAIRS such pairs (made when first used, 100 MiB of device
	// memory each), for callers on different threads (four pairs: 16 threads spent three quarters of a call waiting for one)
	struct HostLane {
		hipStream_t stream = nullptr;
		uint8_t *d_src = nullptr, *d_dst = nullptr, *d_packed = nullptr;
		nxz_batch_job_t *d_jobs = nullptr, *h_jobs = nullptr;
		nxz_batch_result_t *d_res = nullptr, *h_res = nullptr;
		uint64_t *d_off = nullptr, *h_total = nullptr;
		uint8_t *h_src = nullptr, *h_packed = nullptr; // pinned staging for calls of a few MiB (null above STAGE_MAX_BLOCKS per group)
		uint8_t *d_base = nullptr, *h_base = nullptr; // ONE device and ONE pinned allocation hold all of the above (sixteen threads' first calls queue for the runtime's allocator)
		size_t n = 0; uint64_t bytes = 0;
		size_t cap = 0;                           // blocks per group the buffers hold
	} lanes[2 * HOST_PAIRS];
	std::mutex lanes_mtx[HOST_PAIRS];
	std::atomic<unsigned> lanes_turn{0};
	// nxz_deflate_host calls of a few MiB from many threads: the callers that are there at the same time put their blocks into
	// ONE batch (a launch of each kernel for all of them, on one stream), as the rounds below do for single-block jobs --
	// a HIP stream per caller does not get them side by side: the runtime maps the streams onto four hardware queues, and
	// sixteen threads of 1 MiB calls ran at 4 GiB/s, two or three calls at a time (merged_deflate)
	struct Merge {
		enum State { FREE, OPEN, RUNNING, DONE } state = FREE;
		hipStream_t stream = nullptr;
		uint8_t *h_src = nullptr, *h_packed = nullptr;       // pinned: the callers copy their source in and their stream out themselves
		uint8_t *d_src = nullptr, *d_dst = nullptr;
		nxz_batch_job_t *h_jobs = nullptr;                   // pinned, read and written by the kernels in place, as a round's
		nxz_batch_result_t *h_res = nullptr;
		uint64_t *h_off = nullptr;
		nxz_pack_member_t *h_mem = nullptr;
		uint16_t *h_member_of = nullptr;
		uint8_t *h_base = nullptr, *d_base = nullptr;
		int fc = 0; uint32_t H = 0;
		uint32_t slots = 0, jobs = 0, members = 0, filled = 0, left = 0;   // slots: 64 KiB units of staging (windows too); jobs: blocks
		int rc = 0;
		bool ready = false;
	} merges[3];
	std::mutex mm;
	std::condition_variable mcv;
	std::atomic<int> host_callers{0};                 // callers inside nxz_deflate_host at this moment
	hipStream_t split_stream = nullptr;               // nxz_batch_decompress: a large batch of streams that bring tables, shared out between two kernels
	hipEvent_t split_ev[2] = { nullptr, nullptr };
	std::mutex split_mtx;
	// nxu_run_job, compress: callers that arrive while a launch is in flight are gathered and go out
	// together as one launch of each kernel (run_compress / round_run)
	struct Round {
		hipStream_t stream = nullptr;
		nxz_batch_job_t *h_jobs = nullptr;        // pinned, read by the kernels in place
		nxz_batch_result_t *h_res = nullptr;      // pinned, written by the kernels in place
		nxz_batch_dht_t *h_dht = nullptr;
		uint32_t *h_cnt = nullptr;
		nxz_dht_prepared_t *d_prep = nullptr;
		uint8_t *d_tok = nullptr;
		uint16_t *d_cand2 = nullptr;
		uint8_t *d_src = nullptr;                 // the sources, brought over by one copy kernel (two kernels read them)
		uint8_t *d_cut = nullptr;                 // decompress rounds: the workspace of nxz_inflate_cut.hip (made when first used)
		size_t cut_arena = 0;
		uint8_t *d_wg = nullptr;                  // ... or of nxz_inflate_wg.hip (rounds of fresh streams of at most 64 KiB either side)
		uint8_t **h_targets = nullptr;            // ... and where the jobs' outputs go from the device buffers they are decoded into
		struct Item { const uint8_t *src; uint8_t *dst; uint64_t bytes; } *h_items = nullptr;
		bool busy = false, ready = false;
	} rounds[16];
	std::mutex qm;
	std::condition_variable qcv;
	std::deque<struct CompressReq *> q;
	std::deque<struct InflateReq *> qi;           // the same for decompress jobs
	uint32_t *d_job_counters = nullptr;           // job counters of the batched deflate launches (ring)
	unsigned next_counter = 0;
	// measurement aid (nxz_ctx_stage_timing): events around every kernel of the compress batches
	bool timing = false;
	std::vector<hipEvent_t> tev;                  // per chunk: before LZ77, after it, after dhtgen, after the entropy kernel
};
static_assert(std::is_trivially_copyable<nxz_ctx::Scratch>::value, "a Scratch is copied by value under c->mtx");

// A stream's scratch and who may touch it.  Calls on ONE stream share that stream's scratch (tokens, tables, workspaces):
// their launches must not interleave, and a call that needs more room must not free what another has just handed to its
// kernels.  The rules, for every batched entry point:
//   - a Scratch entry is read or written only while c->mtx is held (with_scratch); pointers are copied out of it before
//     anything is launched, never kept as references;
//   - a call holds scratch_use[s] (lease_scratch) from sizing the scratch to its last launch that reads it; the stream's
//     order does the rest;
//   - lock order: frame_use[s], then scratch_use[s], then c->mtx.  So the lease is taken before with_scratch, never inside
//     it, and a framed call (which holds frame_use[s]) touches its own buffers with with_scratch alone: it must not hold
//     scratch_use[s] around nxz_batch_decompress, which takes that lease itself -- inside the route it chooses, because
//     the split route calls itself on the same stream and the mutex is not recursive;
//   - nxz_trim() (trim_compress_scratch) only try_locks scratch_use[s] and looks entries up with find(), never []: a
//     stream's entry that nxz_stream_destroy dropped stays away.
static inline std::unique_lock<std::mutex> lease_scratch(nxz_ctx *c, hipStream_t s)
{
	std::mutex *m;
	{
		std::lock_guard<std::mutex> g(c->mtx);
		m = &c->scratch_use[s];
	}
	return std::unique_lock<std::mutex>(*m);
}
// f(the scratch of `s`, made when first asked for) under c->mtx; returns what f returns
template <class F> static inline auto with_scratch(nxz_ctx *c, hipStream_t s, F &&f)
{
	std::lock_guard<std::mutex> g(c->mtx);
	return f(c->scratch[s]);
}

extern std::mutex g_mtx;                                      // guards g_ctx and the contexts' reference counts (nxz_engine.cpp)
extern nxz_ctx *g_ctx[64];                                    // the context of each device
// The HIP runtime does not survive fork(): a child that inherits contexts must not touch them (the
// reference re-opens its device in the child, lib/nx_zlib.c:529-551; here the child is refused and
// the dispatch layer sends its streams to software zlib).
extern pid_t g_creator_pid;
static inline bool forked_child() { return g_creator_pid != 0 && getpid() != g_creator_pid; }

// A preset dictionary (nxz_dict.h): ONE device buffer of 32 KiB whose last `win` bytes are the inflate window; the deflate
// window is its last W bytes (W a multiple of 16, the buffer's end 16-byte aligned: so is the window).
struct nxz_dict {
	int device = 0;
	size_t len = 0;
	uint32_t id = 1, win = 0, W = 0;
	uint8_t *d_win = nullptr;
	const uint8_t *deflate_window() const { return d_win + NXZ_DICT_WINDOW - W; }
};

hipError_t stream_create_spread(hipStream_t *s, unsigned turn);   // nxz_engine.cpp
size_t trim_compress_scratch();                                    // nxz_batch.cpp (nxz_trim)
// nxz_batch.cpp, for the calls of nxz_batch_framed.cpp, nxz_batch_streams.cpp and nxz_batch_ranges.cpp that run a raw batch or a kernel of its shape.
// force: 0 -- the kernel by the batch's size and kind; 1 -- a stream per lane, any block type; 2 -- a stream per wavefront
int batch_decompress(nxz_ctx_t *c, const nxz_batch_job_t *jobs, size_t n, nxz_batch_result_t *results, nxz_batch_dht_t *dht_io, void *stream, int force);
int batch_decompress_dict(nxz_ctx_t *c, const nxz_dict *dict, const nxz_batch_job_t *jobs, size_t n, nxz_batch_result_t *results, hipStream_t s);
// a compress batch on DEVICE jobs that are as the kernels take them, the first nwin with `win` (16-byte aligned, hist_len bytes) as their window
int batch_compress_windowed(nxz_ctx_t *c, int fc, const uint8_t *win, size_t nwin, const nxz_batch_job_t *jobs, size_t n,
			    nxz_batch_result_t *results, void *stream);
// The jobs' indices by falling source length in BUF_ORDER of `s`, queued on `s` (NULL: none to be had, the jobs go as they come).
// The caller holds the lease until its last launch that reads the order.
const uint32_t *order_by_length_for(nxz_ctx *c, hipStream_t s, const nxz_batch_job_t *jobs, size_t n);

// What the three families of calls around the raw batches share (nxz_batch_framed.cpp, nxz_batch_streams.cpp, nxz_batch_ranges.cpp).
// A framed call holds frame_use[s] from its first kernel to its last:
static inline std::mutex *frame_mutex(nxz_ctx_t *c, hipStream_t s)
{
	std::lock_guard<std::mutex> g(c->mtx);
	return &c->frame_use[s];
}
// How every call goes on once its own arguments are checked.  rc: 1 -- go on, with the device selected, on `s`, frame_use[s] held
// (`frame`) until this goes out of scope; else what the call returns now: -ENODEV in a forked child, 0 when it has no `work`.
struct Entered {
	hipStream_t s;
	int rc;
	std::unique_lock<std::mutex> use;
	Entered(nxz_ctx_t *c, void *stream, bool work, bool frame = true) : s((hipStream_t)stream), rc(forked_child() ? -ENODEV : work ? 1 : 0)
	{
		if (rc != 1) return;
		(void)hipSetDevice(c->device);
		if (frame) use = std::unique_lock<std::mutex>(*frame_mutex(c, s));
	}
};
// A single launch that walks the jobs a wavefront each: launch(order) under the stream's lease (the kernel reads the order), from 128
// jobs on the long ones first, below that order NULL (the caller's order).  Nothing waits.
template <class Launch>
static inline int ordered_launch(nxz_ctx_t *c, hipStream_t s, const nxz_batch_job_t *jobs, size_t n, const char *what, Launch launch)
{
	const auto use = lease_scratch(c, s);
	const uint32_t *order = n >= 128 ? order_by_length_for(c, s, jobs, n) : nullptr;
	return launched(what, launch(order));
}
// nxz_batch_framed.cpp: header kernel -> the raw batch on the derived jobs -> trailer kernel, all on `s`; the caller holds frame_use[s]
int framed_locked(nxz_ctx_t *c, int fmt, const nxz_batch_job_t *jobs, size_t n, nxz_batch_result_t *results, nxz_batch_frame_t *frames, hipStream_t s,
		  const nxz_dict *dict = nullptr);
// nxz_batch_ranges.cpp: the `force` of a raw batch whose jobs bring NXZ_JOB_SUSPEND_WHEN_FULL
int fine_chunk_route();
static inline uint64_t trace_ns() { return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

#endif
