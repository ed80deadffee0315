// nxz_batch_framed.cpp -- the calls of include/nxz_engine.h's device-resident interface that put kernels of their own around a raw
// batch (nxz_batch.cpp) or walk streams without decoding them: framed zlib / gzip streams, output sizes, multi-member gzip jobs,
// one stream per device buffer (written, and read in parts), BGZF discovery, index and range reads, checkpoint index and range reads (one stream's, and a batch's).
#include <functional>
#include "nxz_ctx.h"
#include "nxz_streams_dict.h"
#include "nxz_streams_index.h"
#include "nxz_streams_part.h"
#include "nxz_inflate_part.h"
#include "nxz_checkpoint_fine.h"
#include "nxz_checkpoint_batch.h"

// ---------------------------------------------------------------------------
// Framed streams (nxz_frame.hip): header kernel -> the raw batch on the derived jobs -> trailer kernel, all on `s`.
// The caller holds c->frame_use[s].
// ---------------------------------------------------------------------------
// The header kernel (with the dictionary's DICTID when there is one) into frames and *derived, the raw jobs in BUF_FRAME_JOBS of `s`.
// (the caller's frame_use[s] guards the derived jobs: no lease here, the raw batch takes its own)
static int derive_framed_jobs(nxz_ctx_t *c, int fmt, const nxz_dict *dict, const nxz_batch_job_t *jobs, size_t n, nxz_batch_frame_t *frames,
			      hipStream_t s, nxz_batch_job_t **derived)
{
	nxz_batch_job_t *const d = *derived = with_scratch(c, s, [&](nxz_ctx::Scratch &sc) {
		(void)sc.buf[BUF_FRAME_JOBS].grow(s, n * sizeof(nxz_batch_job_t));
		return sc.buf[BUF_FRAME_JOBS].as<nxz_batch_job_t>();
	});
	if (!d) return -ENOMEM;
	return launched("frame header launch", dict ? nxz_launch_frame_header_dict(fmt, jobs, n, frames, d, dict->id, s)
						    : nxz_launch_frame_header(fmt, jobs, n, frames, d, s));
}

static int framed_locked(nxz_ctx_t *c, int fmt, const nxz_batch_job_t *jobs, size_t n, nxz_batch_result_t *results,
			 nxz_batch_frame_t *frames, hipStream_t s, const nxz_dict *dict = nullptr)
{
	nxz_batch_job_t *derived = nullptr;
	int rc = derive_framed_jobs(c, fmt, dict, jobs, n, frames, s, &derived);
	if (rc) return rc;
	rc = dict ? batch_decompress_dict(c, dict, derived, n, results, s) : batch_decompress(c, derived, n, results, nullptr, s, 0);
	if (rc) return rc;
	return launched("frame trailer launch", nxz_launch_frame_trailer(jobs, n, results, frames, s));
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
	const uint32_t *order = n >= 128 ? order_by_length_for(c, s, jobs, n) : nullptr;   // (NULL: in the caller's order)
	return launched("inflate size launch", nxz_launch_inflate_size(jobs, n, results, order, dict_window, s));
}

extern "C" int nxz_batch_decompress_size(nxz_ctx_t *c, const nxz_batch_job_t *jobs, size_t n, nxz_batch_result_t *results, void *stream)
{
	if (!c || n >= (1u << 31) || (n && (!jobs || !results))) return -EINVAL;
	if (forked_child()) return -ENODEV;
	if (!n) return 0;
	(void)hipSetDevice(c->device);
	return batch_size(c, jobs, n, results, 0, (hipStream_t)stream);
}

// header kernel (the framed decode's own: derive_framed_jobs) -> the size walk on the derived jobs ->
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
	nxz_batch_job_t *derived = nullptr;
	int rc = derive_framed_jobs(c, fmt, dict, jobs, n, frames, s, &derived);
	if (rc) return rc;
	// (without a dictionary the header kernel sets no NXZ_JOB_NO_DICT, and there is no window to withhold: 0)
	if ((rc = batch_size(c, derived, n, results, dict ? dict->win : 0, s)) != 0) return rc;
	return launched("frame trailer launch", nxz_launch_size_trailer(jobs, n, results, frames, s));
}

// ---------------------------------------------------------------------------
// Verify (nxz_inflate_verify.hip, the rules in nxz_verify.h): the size calls with the output passing through a ring in LDS and
// checksummed there -- the same single launch, the same order, the same lease; the framed call ends with the decode's own trailer
// kernel, comparison included.  A dictionary's window is read from its one device copy.
// ---------------------------------------------------------------------------
static int batch_verify(nxz_ctx_t *c, const nxz_batch_job_t *jobs, size_t n, nxz_batch_result_t *results, const nxz_dict *dict, hipStream_t s)
{
	const auto use = lease_scratch(c, s);                                // (the kernel reads the order)
	const uint32_t *order = n >= 128 ? order_by_length_for(c, s, jobs, n) : nullptr;   // (NULL: in the caller's order)
	return launched("inflate verify launch", nxz_launch_inflate_verify(jobs, n, results, order, dict ? dict->d_win : nullptr, dict ? dict->win : 0, s));
}

extern "C" int nxz_batch_decompress_verify(nxz_ctx_t *c, const nxz_batch_job_t *jobs, size_t n, nxz_batch_result_t *results, void *stream)
{
	if (!c || n >= (1u << 31) || (n && (!jobs || !results))) return -EINVAL;
	if (forked_child()) return -ENODEV;
	if (!n) return 0;
	(void)hipSetDevice(c->device);
	return batch_verify(c, jobs, n, results, nullptr, (hipStream_t)stream);
}

extern "C" int nxz_batch_decompress_verify_framed(nxz_ctx_t *c, int fmt, const nxz_dict_t *dict, const nxz_batch_job_t *jobs, size_t n,
						  nxz_batch_result_t *results, nxz_batch_frame_t *frames, void *stream)
{
	if (!c || (dict && dict->device != c->device) || fmt < NXZ_FMT_ZLIB || fmt > NXZ_FMT_AUTO || n >= (1u << 31) || (n && (!jobs || !results || !frames))) return -EINVAL;
	if (forked_child()) return -ENODEV;
	if (!n) return 0;
	(void)hipSetDevice(c->device);
	hipStream_t s = (hipStream_t)stream;
	std::lock_guard<std::mutex> use(*frame_mutex(c, s));
	nxz_batch_job_t *derived = nullptr;
	int rc = derive_framed_jobs(c, fmt, dict, jobs, n, frames, s, &derived);
	if (rc) return rc;
	if ((rc = batch_verify(c, derived, n, results, dict, s)) != 0) return rc;
	return launched("frame trailer launch", nxz_launch_frame_trailer(jobs, n, results, frames, s));
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
	const uint32_t *order = n >= 128 ? order_by_length_for(c, s, jobs, n) : nullptr;   // (NULL: in the caller's order)
	return launched("gzip members index launch", nxz_launch_gzip_members_index(jobs, n, member_cap, members, streams, order, s));
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
	int rc = launched("gzip members expand launch", nxz_launch_gzip_members_expand(jobs, n, member_cap, members, streams, total, ws, &xjobs, &xresults, &xframes, s));
	if (rc) return rc;
	if ((rc = framed_locked(c, NXZ_FMT_GZIP, xjobs, total, xresults, xframes, s)) != 0) return rc;
	return launched("gzip members join launch", nxz_launch_gzip_members_join(n, member_cap, members, streams, total, ws, s));
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
// With a dictionary (nxz_batch_deflate_streams_dict; nxz_streams_dict.hip, the rules in nxz_streams_dict.h) the same function runs: the
// dictionary form's refusals, prologue and epilogue, and -- when block 0 has a window at all, h0 != 0 -- per chunk an expand that
// also writes the jobs in launch order (the chunk's first blocks, then the rest), the compress batch with the dictionary's last h0
// bytes as the window of those first blocks, and a gather of the results back into the batch's order.  How many first blocks a
// chunk holds the host knows from its one pass (nz[]: the streams with blocks in front of each stream): still no host wait.
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

extern "C" size_t nxz_deflate_stream_bound_dict(uint64_t src_len, uint32_t hist_max, int fmt)
{
	return nxz_streams_dict_fmt_ok(fmt) ? (size_t)nxz_streams_dict_bound(src_len, hist_max, fmt) : 0;
}

// This call's pinned staging of `up_bytes` (Scratch::h_up: two in turn): the upload that read it last must have run.  0 and *h, *ev
// (to record behind this call's upload: streams_upload), or -errno.
static int streams_staging(nxz_ctx_t *c, hipStream_t s, size_t up_bytes, uint8_t **h, hipEvent_t *ev)
{
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
	*h = st.h; *ev = st.ev;
	return 0;
}
// ... and its upload to `d`, queued on `s`
static int streams_upload(nxz_ctx_t *c, hipStream_t s, uint8_t *d, const uint8_t *h, size_t up_bytes, hipEvent_t ev)
{
	HIPCHK(hipMemcpyAsync(d, h, up_bytes, hipMemcpyHostToDevice, s), return -EIO);
	HIPCHK(hipEventRecord(ev, s), return -EIO);
	with_scratch(c, s, [](nxz_ctx::Scratch &r) { r.up_turn++; return 0; });
	return 0;
}

// what nxz_batch_deflate_streams_indexed adds to a call: the caller's arrays (its arguments, checked there)
struct StreamsIndex {
	uint64_t span;
	uint32_t cp_cap;
	uint64_t *cbit, *uoff;
	uint8_t *windows;
	nxz_checkpoint_stream_t *streams;
	nxz_batch_job_t *index_jobs;
};

// dict: NULL, or the dictionary form (its device checked by the caller); ix: NULL, or the index to write on the way (never with dict)
static int deflate_streams(nxz_ctx_t *c, int fc, int fmt, int level, uint32_t hist_max, const nxz_dict *dict, const nxz_stream_job_t *jobs, size_t n,
			   nxz_stream_result_t *results, void *stream, const StreamsIndex *ix = nullptr)
{
	if (!c || (fc != NXZ_FC_COMPRESS_FHT && fc != NXZ_FC_COMPRESS_DHTGEN) || !(dict ? nxz_streams_dict_fmt_ok(fmt) : nxz_streams_fmt_ok(fmt)) ||
	    level < -1 || level > 9 || (n && (!jobs || !results))) return -EINVAL;
	if (forked_child()) return -ENODEV;
	if (!n) return 0;
	if (n >= (1u << 31)) return -E2BIG;
	(void)hipSetDevice(c->device);
	hipStream_t s = (hipStream_t)stream;
	std::lock_guard<std::mutex> use(*frame_mutex(c, s));
	const uint32_t H = nxz_streams_window(hist_max), B = nxz_streams_block_bytes(hist_max), ns = (uint32_t)n;
	auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
	// the first block's window, and whether the chunks' first blocks go apart from the rest
	const uint32_t h0 = dict ? nxz_streams_dict_window(dict->len, hist_max) : 0;
	const bool split = h0 != 0;
	// what is uploaded: [descriptors][first]([nz]), the same layout in the staging and in the device buffer
	const size_t o_first = up(n * sizeof(nxz_stream_job_t)), o_nz = o_first + up((n + 1) * sizeof(uint32_t)),
		     up_bytes = split ? o_nz + (n + 1) * sizeof(uint32_t) : o_first + (n + 1) * sizeof(uint32_t);
	uint8_t *st_h = nullptr;
	hipEvent_t st_ev = nullptr;
	int rc = streams_staging(c, s, up_bytes, &st_h, &st_ev);
	if (rc) return rc;
	// one pass over the streams: a refused stream gets no blocks
	nxz_stream_job_t *const h_desc = (nxz_stream_job_t *)st_h;
	uint32_t *const h_first = (uint32_t *)(st_h + o_first);
	uint32_t *const h_nz = split ? (uint32_t *)(st_h + o_nz) : nullptr;   // the streams with blocks in front of each stream
	memcpy(h_desc, jobs, n * sizeof(nxz_stream_job_t));
	uint64_t total = 0;
	uint32_t with_blocks = 0;
	for (size_t i = 0; i < n; i++) {
		h_first[i] = (uint32_t)total;
		if (h_nz) h_nz[i] = with_blocks;
		const uint64_t before = total;
		if (!(dict ? nxz_streams_dict_refusal(&jobs[i], hist_max, fmt) : nxz_streams_refusal(&jobs[i], hist_max, fmt)))
			total += nxz_streams_blocks(jobs[i].src_len, B);
		if (total >= (1ull << 31)) return -E2BIG;
		if (total != before) with_blocks++;
	}
	h_first[n] = (uint32_t)total;
	if (h_nz) h_nz[n] = with_blocks;
	const uint32_t nblk = (uint32_t)total, C = std::min(streams_chunk(), nblk);
	const size_t o_state = up(up_bytes), o_jobs = o_state + up(n * sizeof(nxz_stream_state_t)), o_res = o_jobs + up((size_t)C * sizeof(nxz_batch_job_t)),
		     o_owner = o_res + up((size_t)C * sizeof(nxz_batch_result_t)), o_off = o_owner + up((size_t)C * sizeof(uint32_t)),
		     o_slots = o_off + up((size_t)C * sizeof(uint64_t)), o_ljobs = o_slots + up((size_t)C * NXZ_STREAMS_SLOT),
		     o_lres = o_ljobs + up((size_t)C * sizeof(nxz_batch_job_t)), o_pos = o_lres + up((size_t)C * sizeof(nxz_batch_result_t)),
		     d_plain = split ? o_pos + (size_t)C * sizeof(uint32_t) : o_slots + (size_t)C * NXZ_STREAMS_SLOT,
		     // the index's own, behind everything the plain call lays out: a state a stream, two slot marks a block of a chunk
		     o_ist = up(d_plain), o_marks = o_ist + up(n * sizeof(nxz_stream_index_state_t)),
		     d_bytes = !ix ? d_plain : ix->windows ? o_marks + (size_t)C * 2 * sizeof(uint32_t) : o_marks;
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
	const uint32_t *const d_nz = split ? (const uint32_t *)(d + o_nz) : nullptr;
	nxz_batch_job_t *const d_ljobs = split ? (nxz_batch_job_t *)(d + o_ljobs) : nullptr;
	nxz_batch_result_t *const d_lres = split ? (nxz_batch_result_t *)(d + o_lres) : nullptr;
	uint32_t *const d_pos = split ? (uint32_t *)(d + o_pos) : nullptr;
	nxz_stream_index_state_t *const d_ist = ix ? (nxz_stream_index_state_t *)(d + o_ist) : nullptr;
	uint32_t *const d_marks = ix && ix->windows ? (uint32_t *)(d + o_marks) : nullptr;
	if ((rc = streams_upload(c, s, d, st_h, up_bytes, st_ev)) != 0) return rc;
	rc = launched("streams prologue launch", dict ? nxz_launch_streams_dict_prologue(d_desc, ns, hist_max, fmt, level, dict->id, d_state, s)
							  : nxz_launch_streams_prologue(d_desc, ns, hist_max, fmt, level, d_state, s));
	if (rc) return rc;
	if (ix && (rc = launched("streams index prologue launch", nxz_launch_streams_index_prologue(d_desc, ns, fmt, d_state, ix->cp_cap, ix->cbit, ix->uoff,
												     d_ist, s))) != 0) return rc;
	const uint32_t op_block = nxz_crc_shift_op(B);
	uint32_t i_lo = 0;                                                  // the stream of the chunk's first block (the chunks go in order)
	for (uint32_t b0 = 0; b0 < nblk; b0 += C) {
		const uint32_t m = std::min(C, nblk - b0);
		while (h_first[i_lo + 1] <= b0) i_lo++;
		uint32_t i_hi = i_lo;
		while (h_first[i_hi + 1] < b0 + m) i_hi++;
		if (split) {
			// the first blocks of streams in front of the chunk, and inside it (i_lo and i_hi have blocks: they own b0 and b0 + m - 1)
			const uint32_t nz_b0 = nxz_streams_dict_firsts_before(h_nz[i_lo], b0 - h_first[i_lo]), nf = nxz_streams_dict_firsts_before(h_nz[i_hi], 1) - nz_b0;
			rc = launched("streams expand launch", nxz_launch_streams_dict_expand(d_desc, d_first, d_nz, ns, b0, m, hist_max, h0, nz_b0, nf, d_slots,
											      d_jobs, d_ljobs, d_owner, d_pos, s));
			if (rc) return rc;
			if ((rc = batch_compress_windowed(c, fc | 0x08, dict->d_win + nxz_streams_dict_window_at(h0), nf, d_ljobs, m, d_lres, s)) != 0) return rc;
			if ((rc = launched("streams gather launch", nxz_launch_streams_dict_gather(d_lres, d_pos, m, d_res, s))) != 0) return rc;
		} else {
			rc = launched("streams expand launch", nxz_launch_streams_expand(d_desc, d_first, ns, b0, m, hist_max, d_slots, d_jobs, d_owner, s));
			if (rc) return rc;
			if ((rc = nxz_batch_compress(c, fc | (H ? 0x08 : 0), d_jobs, m, nullptr, 0, d_res, nullptr, s)) != 0) return rc;
		}
		rc = nxz_launch_streams_layout(d_first, i_lo, i_hi - i_lo + 1, b0, m, d_jobs, d_res, hist_max, op_block, d_state, d_off, s);
		if (!rc && ix) rc = nxz_launch_streams_index_sweep(d_first, i_lo, i_hi - i_lo + 1, b0, m, d_jobs, d_res, d_off, hist_max, ix->span, ix->cp_cap,
								    ix->cbit, ix->uoff, d_ist, d_marks, s);
		if (!rc) rc = nxz_launch_streams_pack(d_desc, d_first, d_owner, b0, m, d_jobs, d_res, d_off, s);
		if (!rc && d_marks) rc = nxz_launch_streams_index_windows(d_desc, d_owner, m, d_marks, ix->cp_cap, ix->uoff, ix->windows, s);
		if ((rc = launched("streams pack launch", rc)) != 0) return rc;
		i_lo = i_hi;
	}
	rc = launched("streams epilogue launch", dict ? nxz_launch_streams_dict_epilogue(d_desc, d_first, ns, hist_max, fmt, d_state, results, s)
						      : nxz_launch_streams_epilogue(d_desc, d_first, ns, hist_max, fmt, d_state, results, s));
	if (rc || !ix) return rc;
	return launched("streams index epilogue launch", nxz_launch_streams_index_epilogue(d_desc, ns, fmt, results, d_ist, ix->cp_cap, ix->cbit, ix->uoff,
											   ix->streams, ix->index_jobs, s));
}

extern "C" int nxz_batch_deflate_streams(nxz_ctx_t *c, int fc, int fmt, int level, uint32_t hist_max, const nxz_stream_job_t *jobs, size_t n,
					 nxz_stream_result_t *results, void *stream)
{
	return deflate_streams(c, fc, fmt, level, hist_max, nullptr, jobs, n, results, stream);
}

// The same call with the streams' checkpoint index as a by-product (nxz_streams_index.hip, the rules in nxz_streams_index.h): behind
// the prologue checkpoint 0 and the index's per-stream state, per chunk a sweep over the block headers behind layout and the windows'
// copy beside pack, behind the epilogue the sentinels and the streams' records.  The state and a chunk's slot marks lie behind the
// plain call's part of BUF_STREAMS; still everything on `s`, and no host wait.
extern "C" int nxz_batch_deflate_streams_indexed(nxz_ctx_t *c, int fc, int fmt, int level, uint32_t hist_max, const nxz_stream_job_t *jobs, size_t n,
						 nxz_stream_result_t *results, uint64_t span, uint32_t cp_cap, uint64_t *cbit, uint64_t *uoff,
						 uint8_t *windows, nxz_checkpoint_stream_t *streams, nxz_batch_job_t *index_jobs, void *stream)
{
	if (span == 0 || cp_cap == 0 || (n && (!cbit || !uoff || !streams)) || !nxz_si_shape_ok(n, cp_cap)) return -EINVAL;
	const StreamsIndex ix = {span, cp_cap, cbit, uoff, windows, streams, index_jobs};
	return deflate_streams(c, fc, fmt, level, hist_max, nullptr, jobs, n, results, stream, &ix);
}

extern "C" int nxz_batch_deflate_streams_dict(nxz_ctx_t *c, int fc, int fmt, int level, uint32_t hist_max, const nxz_dict_t *dict,
					      const nxz_stream_job_t *jobs, size_t n, nxz_stream_result_t *results, void *stream)
{
	if (!c || !dict || dict->device != c->device) return -EINVAL;
	return deflate_streams(c, fc, fmt, level, hist_max, dict, jobs, n, results, stream);
}

// ---------------------------------------------------------------------------
// A stream written in parts (nxz_streams_part.hip, the rules in nxz_streams_part.h): deflate_streams' shape with the part's kernels --
// the same pinned staging and upload, the same chunk loop, BUF_STREAMS under frame_use[s], everything on `s` and no host wait.  The
// host's one pass also counts the parts whose first block is STAGED (a window that does not lie in front of the source in memory):
// sg[] goes up beside first[], and per chunk the host knows how many staging slots its first blocks take and how many lie in front
// of it.  The slots (65 536 bytes a staged block of a chunk) and the chunk's staging list lie behind the plain call's layout.
// What the host cannot see is the carry: a part without FIRST on a finished stream is planned like any other and refused on the device.
// ---------------------------------------------------------------------------
extern "C" size_t nxz_deflate_stream_part_bound(uint64_t src_len, uint32_t hist_max, int fmt, uint32_t flags)
{
	return (size_t)nxz_streams_part_bound(src_len, hist_max, fmt, flags);
}

extern "C" int nxz_batch_deflate_streams_part(nxz_ctx_t *c, int fc, int fmt, int level, uint32_t hist_max, const nxz_stream_part_job_t *jobs, size_t n,
					      nxz_stream_carry_t *carry, nxz_stream_result_t *results, void *stream)
{
	if (!c || (fc != NXZ_FC_COMPRESS_FHT && fc != NXZ_FC_COMPRESS_DHTGEN) || !nxz_streams_fmt_ok(fmt) || level < -1 || level > 9 ||
	    (n && (!jobs || !results || !carry))) return -EINVAL;
	if (forked_child()) return -ENODEV;
	if (!n) return 0;
	if (n >= (1u << 31)) return -E2BIG;
	(void)hipSetDevice(c->device);
	hipStream_t s = (hipStream_t)stream;
	std::lock_guard<std::mutex> use(*frame_mutex(c, s));
	const uint32_t H = nxz_streams_window(hist_max), B = nxz_streams_block_bytes(hist_max), ns = (uint32_t)n;
	auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
	// what is uploaded: [descriptors][first][sg], the same layout in the staging and in the device buffer
	const size_t o_first = up(n * sizeof(nxz_stream_part_job_t)), o_sg = o_first + up((n + 1) * sizeof(uint32_t)), up_bytes = o_sg + (n + 1) * sizeof(uint32_t);
	uint8_t *st_h = nullptr;
	hipEvent_t st_ev = nullptr;
	int rc = streams_staging(c, s, up_bytes, &st_h, &st_ev);
	if (rc) return rc;
	// one pass over the streams: a part the host refuses gets no blocks; a part with blocks may have its first one staged
	uint32_t *const h_first = (uint32_t *)(st_h + o_first), *const h_sg = (uint32_t *)(st_h + o_sg);
	memcpy(st_h, jobs, n * sizeof(nxz_stream_part_job_t));
	uint64_t total = 0;
	uint32_t staged = 0;
	for (size_t i = 0; i < n; i++) {
		h_first[i] = (uint32_t)total;
		h_sg[i] = staged;
		if (nxz_streams_part_refusal(&jobs[i], 0, hist_max, fmt)) continue;
		total += nxz_streams_blocks(jobs[i].src_len, B);
		if (total >= (1ull << 31)) return -E2BIG;
		if (nxz_streams_part_staged(&jobs[i], hist_max)) staged++;
	}
	h_first[n] = (uint32_t)total;
	h_sg[n] = staged;
	const uint32_t nblk = (uint32_t)total, C = std::min(streams_chunk(), nblk), S = std::min(C, staged);   // S: the staged blocks a chunk holds at most
	const size_t o_state = up(up_bytes), o_jobs = o_state + up(n * sizeof(nxz_stream_state_t)), o_res = o_jobs + up((size_t)C * sizeof(nxz_batch_job_t)),
		     o_owner = o_res + up((size_t)C * sizeof(nxz_batch_result_t)), o_off = o_owner + up((size_t)C * sizeof(uint32_t)),
		     o_slots = o_off + up((size_t)C * sizeof(uint64_t)), o_list = o_slots + up((size_t)C * NXZ_STREAMS_SLOT),
		     o_stage = o_list + up((size_t)S * sizeof(uint32_t)), d_bytes = o_stage + (size_t)S * NXZ_STREAMS_STAGE_SLOT;
	uint8_t *const d = with_scratch(c, s, [&](nxz_ctx::Scratch &r) {
		(void)r.buf[BUF_STREAMS].grow(s, d_bytes);
		return r.buf[BUF_STREAMS].p;
	});
	if (!d) return -ENOMEM;
	const nxz_stream_part_job_t *const d_desc = (const nxz_stream_part_job_t *)d;
	const uint32_t *const d_first = (const uint32_t *)(d + o_first), *const d_sg = (const uint32_t *)(d + o_sg);
	nxz_stream_state_t *const d_state = (nxz_stream_state_t *)(d + o_state);
	nxz_batch_job_t *const d_jobs = (nxz_batch_job_t *)(d + o_jobs);
	nxz_batch_result_t *const d_res = (nxz_batch_result_t *)(d + o_res);
	uint32_t *const d_owner = (uint32_t *)(d + o_owner), *const d_list = (uint32_t *)(d + o_list);
	uint64_t *const d_off = (uint64_t *)(d + o_off);
	uint8_t *const d_slots = d + o_slots, *const d_stage = d + o_stage;
	if ((rc = streams_upload(c, s, d, st_h, up_bytes, st_ev)) != 0) return rc;
	if ((rc = launched("streams part prologue launch", nxz_launch_streams_part_prologue(d_desc, ns, hist_max, fmt, level, carry, d_state, s))) != 0) return rc;
	const uint32_t op_block = nxz_crc_shift_op(B);
	uint32_t i_lo = 0;                                                  // the stream of the chunk's first block (the chunks go in order)
	for (uint32_t b0 = 0; b0 < nblk; b0 += C) {
		const uint32_t m = std::min(C, nblk - b0);
		while (h_first[i_lo + 1] <= b0) i_lo++;
		uint32_t i_hi = i_lo;
		while (h_first[i_hi + 1] < b0 + m) i_hi++;
		// the staged first blocks in front of the chunk and inside it (i_lo owns b0: its first block lies in front unless it IS b0;
		// i_hi owns b0 + m - 1: its first block is not behind the chunk)
		const uint32_t sg_b0 = h_first[i_lo] < b0 ? h_sg[i_lo + 1] : h_sg[i_lo], nst = h_sg[i_hi + 1] - sg_b0;
		rc = nxz_launch_streams_part_expand(d_desc, d_first, d_sg, ns, b0, m, hist_max, sg_b0, d_slots, d_stage, d_jobs, d_owner, d_list, s);
		if (!rc && nst) rc = nxz_launch_streams_part_stage(d_desc, d_owner, d_list, nst, d_jobs, s);
		if ((rc = launched("streams part expand launch", rc)) != 0) return rc;
		if ((rc = nxz_batch_compress(c, fc | (H ? 0x08 : 0), d_jobs, m, nullptr, 0, d_res, nullptr, s)) != 0) return rc;
		rc = nxz_launch_streams_part_layout(d_desc, d_first, i_lo, i_hi - i_lo + 1, b0, m, d_jobs, d_res, hist_max, op_block, d_state, d_off, s);
		if (!rc) rc = nxz_launch_streams_part_pack(d_desc, d_first, d_owner, b0, m, d_jobs, d_res, d_off, d_state, s);
		if ((rc = launched("streams part pack launch", rc)) != 0) return rc;
		i_lo = i_hi;
	}
	return launched("streams part epilogue launch", nxz_launch_streams_part_epilogue(d_desc, d_first, ns, hist_max, fmt, d_state, carry, results, s));
}

// ---------------------------------------------------------------------------
// A stream READ in parts (nxz_inflate_part.hip, the rules in nxz_inflate_part.h): per chunk open -> stage -> the raw batch on the
// derived jobs with their table slots as dht_io -> close, everything on `s` and no host wait; the same pinned staging and upload,
// BUF_STREAMS under frame_use[s].  What the host cannot see is the carry -- the phase, the window that counts, the tail --, so its
// one pass sets aside the most a part's slot can take (nxz_inflate_part_slot_bound) and cuts the batch into chunks by that: a chunk
// ends in front of the stream that would carry its slots beyond NXZ_INFLATE_PART_SCRATCH bytes (a stream larger than that is a
// chunk of its own) or at NXZ_INFLATE_PART_CHUNK_STREAMS streams.  off[] goes up beside the descriptors: a chunk of m streams has
// m + 1 entries, the first 0, the last its staging bytes.  The decode is kept off the stream-per-lane kernel as the fine range reads
// are (fine_chunk_route below): the jobs bring NXZ_JOB_SUSPEND_WHEN_FULL.
// ---------------------------------------------------------------------------
static int fine_chunk_route();

static uint64_t inflate_part_scratch()
{
	const char *e = getenv("NXZ_INFLATE_PART_SCRATCH");                 // (read at every call: the tests switch it)
	const uint64_t v = e ? strtoull(e, nullptr, 0) : 0;
	return v ? v : NXZ_INFLATE_PART_SCRATCH_DEFAULT;
}

extern "C" int nxz_batch_inflate_streams_part(nxz_ctx_t *c, int fmt, const nxz_inflate_part_job_t *jobs, size_t n, nxz_inflate_carry_t *carry,
					      nxz_inflate_part_result_t *results, void *stream)
{
	if (!c || !nxz_inflate_part_fmt_ok(fmt) || (n && (!jobs || !results || !carry))) return -EINVAL;
	if (forked_child()) return -ENODEV;
	if (!n) return 0;
	if (n >= (1u << 31)) return -E2BIG;
	for (size_t i = 0; i < n; i++)
		if (nxz_inflate_part_slot_bound(&jobs[i]) > 0xffffffffull) return -E2BIG;   // (window + tail + part is a raw job's src_len)
	(void)hipSetDevice(c->device);
	hipStream_t s = (hipStream_t)stream;
	std::lock_guard<std::mutex> use(*frame_mutex(c, s));
	const uint64_t scratch = inflate_part_scratch();
	auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
	// what is uploaded: [descriptors][off], the same layout in the staging and in the device buffer (a chunk a stream at the worst: 2 n entries)
	const size_t o_off = up(n * sizeof(nxz_inflate_part_job_t)), up_bytes = o_off + 2 * n * sizeof(uint64_t);
	uint8_t *st_h = nullptr;
	hipEvent_t st_ev = nullptr;
	int rc = streams_staging(c, s, up_bytes, &st_h, &st_ev);
	if (rc) return rc;
	// one pass over the streams: the chunks and the slots' offsets inside them
	uint64_t *const h_off = (uint64_t *)(st_h + o_off);
	memcpy(st_h, jobs, n * sizeof(nxz_inflate_part_job_t));
	uint64_t cur = 0, max_bytes = 0;
	size_t e = 0;
	uint32_t cnt = 0, max_cnt = 0;
	for (size_t i = 0; i < n; i++) {
		const uint64_t b = nxz_inflate_part_slot_bound(&jobs[i]);
		if (cnt && (cur + b > scratch || cnt == NXZ_INFLATE_PART_CHUNK_STREAMS)) { h_off[e++] = cur; cur = 0; cnt = 0; }
		h_off[e++] = cur;
		cur += b; cnt++;
		max_bytes = std::max(max_bytes, cur); max_cnt = std::max(max_cnt, cnt);
	}
	h_off[e++] = cur;
	const size_t C = max_cnt;
	const size_t o_work = up(up_bytes), o_jobs = o_work + up(C * sizeof(nxz_inflate_part_work_t)), o_res = o_jobs + up(C * sizeof(nxz_batch_job_t)),
		     o_dht = o_res + up(C * sizeof(nxz_batch_result_t)), o_stage = o_dht + up(C * sizeof(nxz_batch_dht_t)), d_bytes = o_stage + (size_t)max_bytes;
	uint8_t *const d = with_scratch(c, s, [&](nxz_ctx::Scratch &r) {
		(void)r.buf[BUF_STREAMS].grow(s, d_bytes);
		return r.buf[BUF_STREAMS].p;
	});
	if (!d) return -ENOMEM;
	const nxz_inflate_part_job_t *const d_desc = (const nxz_inflate_part_job_t *)d;
	const uint64_t *const d_off = (const uint64_t *)(d + o_off);
	nxz_inflate_part_work_t *const d_work = (nxz_inflate_part_work_t *)(d + o_work);
	nxz_batch_job_t *const d_jobs = (nxz_batch_job_t *)(d + o_jobs);
	nxz_batch_result_t *const d_res = (nxz_batch_result_t *)(d + o_res);
	nxz_batch_dht_t *const d_dht = (nxz_batch_dht_t *)(d + o_dht);
	uint8_t *const d_stage = d + o_stage;
	if ((rc = streams_upload(c, s, d, st_h, up_bytes, st_ev)) != 0) return rc;
	size_t e0 = 0;
	for (size_t i0 = 0; i0 < n;) {
		uint32_t m = 1;                                                  // the chunk's entries end in front of the next chunk's 0
		while (e0 + m + 1 < e && h_off[e0 + m + 1] != 0) m++;
		rc = nxz_launch_inflate_part_open(d_desc + i0, m, fmt, carry + i0, d_off + e0, d_stage, d_jobs, d_dht, d_work, results + i0, s);
		if (!rc) rc = nxz_launch_inflate_part_stage(d_desc + i0, carry + i0, d_off + e0, m, h_off[e0 + m], d_work, d_jobs, s);
		if ((rc = launched("inflate part stage launch", rc)) != 0) return rc;
		if ((rc = batch_decompress(c, d_jobs, m, d_res, d_dht, s, fine_chunk_route())) != 0) return rc;
		if ((rc = launched("inflate part close launch", nxz_launch_inflate_part_close(d_desc + i0, m, carry + i0, d_jobs, d_res, d_dht, d_work, results + i0, s))) != 0)
			return rc;
		i0 += m; e0 += m + 1;
	}
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
		if ((rc = launched("bgzf discovery launch", rc)) != 0) return rc;
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

// Members a chunk of a range read decodes at most: NXZ_BGZF_CHUNK (read at every call: the tests lower it), 16 384
static uint64_t bgzf_chunk_members()
{
	const char *e = getenv("NXZ_BGZF_CHUNK");
	const uint64_t v = e ? strtoull(e, nullptr, 0) : 0;
	return v && v < 16384 ? v : 16384;
}

// ---------------------------------------------------------------------------
// Range reads through an index: nxz_bgzf_read_ranges over the members of a BGZF image, nxz_checkpoint_read_ranges over the segments
// between a stream's checkpoints.  One driver: the map and ONE wait for its totals, then per chunk of needed members their decode
// into slots and the gather of the pieces (nxz_bgzf.hip's, for both), then the zeros of damaged ranges and a last wait.  The caller
// holds frame_use[s] from the first kernel to the last wait: BUF_RNG and BUF_RNG_SLOTS are both calls'.
// ---------------------------------------------------------------------------
// a chunk's part of BUF_RNG_SLOTS: an output slot (and, where the call stages its inputs, an input slot) per member, all of the
// largest needed member's size and 16-byte aligned, then the members' jobs, frames and results (and, where the call asks for them,
// a table slot per member)
struct RangeSlots {
	uint8_t *islots, *oslots;
	uint64_t istride, ostride;
	nxz_batch_job_t *jobs;
	nxz_batch_frame_t *frames;
	nxz_batch_result_t *results;
	nxz_batch_dht_t *dht;
};
// what the two calls do differently.  Both callables queue on `s`, report their own failures (launched) and return 0 or the error:
//   map(ws)                 the map kernels into ws (BUF_RNG): ctl = ws[0..5] as nxz_device.h lists them
//   chunk(ws, k0, cnt, sl)  staging, decode and verdict of needed members k0 .. k0 + cnt - 1, so that sl.frames and sl.results are
//                           what nxz_launch_bgzf_gather looks at
struct RangeSteps {
	std::function<int(uint8_t *ws)> map;
	std::function<int(uint8_t *ws, uint64_t k0, uint64_t cnt, const RangeSlots &sl)> chunk;
	bool input_slots;                 // the chunk stages its inputs: slots of ctl[5] bytes (else none, istride 0)
	bool dht_slots = false;           // the chunk's jobs resume inside dynamic blocks: a nxz_batch_dht_t a member (else none, NULL)
	const char *gather_what, *zero_what;
};
static int read_ranges_locked(nxz_ctx_t *c, hipStream_t s, const RangeSteps &steps, const uint64_t *uoff, uint64_t L, size_t n, uint8_t *dst,
			      uint64_t dst_cap, uint64_t *offsets, uint32_t *status, uint64_t *out_len, uint64_t *decoded)
{
	uint8_t *const ws = with_scratch(c, s, [&](nxz_ctx::Scratch &sc) {
		(void)sc.buf[BUF_RNG].grow(s, nxz_bgzf_ranges_workspace(n, L));
		return sc.buf[BUF_RNG].p;
	});
	if (!ws) return -ENOMEM;
	int rc = steps.map(ws);
	if (rc) return rc;
	uint64_t ctl[6];
	HIPCHK(hipMemcpyAsync(ctl, ws, sizeof(ctl), hipMemcpyDeviceToHost, s), return -EIO);
	HIPCHK(hipStreamSynchronize(s), return -EIO);
	if (ctl[0]) return -EILSEQ;
	if (out_len) *out_len = ctl[2];
	if (ctl[2] > dst_cap || (ctl[2] && !dst)) return -E2BIG;
	const uint64_t needed = ctl[1], pieces = ctl[3];
	if (!needed) return 0;
	// at most 1 GiB of output slots, and of input slots (65 536 bytes a slot for BGZF; a member larger than 1 GiB goes alone)
	auto stride_of = [](uint64_t largest) { return (std::max<uint64_t>(largest, 16) + 15) & ~(uint64_t)15; };
	auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
	RangeSlots sl;
	sl.ostride = stride_of(ctl[4]);
	sl.istride = steps.input_slots ? stride_of(ctl[5]) : 0;
	const uint64_t per = std::min(needed, std::min(bgzf_chunk_members(), std::max<uint64_t>(1, (1ull << 30) / std::max(sl.istride, sl.ostride))));
	const size_t ib = up(per * sl.istride), ob = up(per * sl.ostride), jb = up(per * sizeof(nxz_batch_job_t)), fb = up(per * sizeof(nxz_batch_frame_t)),
		     rb = up(per * sizeof(nxz_batch_result_t)), db = steps.dht_slots ? per * sizeof(nxz_batch_dht_t) : 0;
	uint8_t *const slots = with_scratch(c, s, [&](nxz_ctx::Scratch &sc) {
		(void)sc.buf[BUF_RNG_SLOTS].grow(s, ib + ob + jb + fb + rb + db);
		return sc.buf[BUF_RNG_SLOTS].p;
	});
	if (!slots) return -ENOMEM;
	sl.islots = slots; sl.oslots = slots + ib;
	sl.jobs = (nxz_batch_job_t *)(slots + ib + ob);
	sl.frames = (nxz_batch_frame_t *)(slots + ib + ob + jb);
	sl.results = (nxz_batch_result_t *)(slots + ib + ob + jb + fb);
	sl.dht = steps.dht_slots ? (nxz_batch_dht_t *)(slots + ib + ob + jb + fb + rb) : nullptr;
	for (uint64_t k0 = 0; k0 < needed; k0 += per) {
		const uint64_t cnt = std::min(per, needed - k0);
		if ((rc = steps.chunk(ws, k0, cnt, sl)) != 0) return rc;
		rc = launched(steps.gather_what, nxz_launch_bgzf_gather(uoff, n, L, pieces, ws, offsets, sl.oslots, sl.ostride, k0, cnt, sl.frames, sl.results, dst, status, s));
		if (rc) return rc;
	}
	if ((rc = launched(steps.zero_what, nxz_launch_bgzf_zero(n, offsets, status, dst, s))) != 0) return rc;
	HIPCHK(hipStreamSynchronize(s), return -EIO);
	if (decoded) *decoded = needed;
	return 0;
}

// Ranges of a BGZF image: the map is nxz_bgzf.hip's, a chunk is the framed gzip decode of its members into the output slots.
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
	RangeSteps steps;
	steps.map = [&](uint8_t *ws) {
		return launched("bgzf map launch", nxz_launch_bgzf_map(packed, packed_len, coff, uoff, L, kind, ranges, n, offsets, status, ws, s));
	};
	steps.chunk = [&](uint8_t *ws, uint64_t k0, uint64_t cnt, const RangeSlots &sl) {
		const int rc = launched("bgzf jobs launch", nxz_launch_bgzf_jobs(packed, coff, uoff, n, L, ws, k0, cnt, sl.oslots, sl.ostride, sl.jobs, s));
		return rc ? rc : framed_locked(c, NXZ_FMT_GZIP, sl.jobs, (size_t)cnt, sl.results, sl.frames, s);
	};
	steps.input_slots = false;
	steps.gather_what = "bgzf gather launch"; steps.zero_what = "bgzf zero launch";
	return read_ranges_locked(c, s, steps, uoff, L, n, dst, dst_cap, offsets, status, out_len, decoded);
}

// ---------------------------------------------------------------------------
// Checkpoints (nxz_checkpoint.hip, the rules in nxz_checkpoint.h).  The index is the size query's shape: a wavefront a job, from 128
// jobs on the long ones first, the order in this stream's scratch under the lease; the windows' copies go behind it on `s`, and
// nothing waits for the host.
// ---------------------------------------------------------------------------
// what the three index calls refuse alike (each adds the arrays and the span of its own)
static bool index_args_ok(const nxz_ctx_t *c, int fmt, const nxz_batch_job_t *jobs, size_t n, uint64_t span, uint32_t cp_cap, const uint64_t *cbit,
			  const uint64_t *uoff, const nxz_checkpoint_stream_t *streams)
{
	return c && fmt >= NXZ_FMT_RAW && fmt <= NXZ_FMT_AUTO && span != 0 && cp_cap != 0 && n < (1u << 31) && (!n || (jobs && cbit && uoff && streams));
}
// ... and how they launch: launch(order, s) under the stream's lease, order NULL (the caller's order) below 128 jobs
template <class Launch>
static int index_launch(nxz_ctx_t *c, const nxz_batch_job_t *jobs, size_t n, void *stream, const char *what, Launch launch)
{
	if (forked_child()) return -ENODEV;
	if (!n) return 0;
	(void)hipSetDevice(c->device);
	hipStream_t s = (hipStream_t)stream;
	const auto use = lease_scratch(c, s);                                // (the kernel reads the order)
	const uint32_t *order = n >= 128 ? order_by_length_for(c, s, jobs, n) : nullptr;
	return launched(what, launch(order, s));
}

extern "C" int nxz_batch_checkpoint_index(nxz_ctx_t *c, int fmt, const nxz_batch_job_t *jobs, size_t n, uint64_t span, uint32_t cp_cap,
					  uint64_t *cbit, uint64_t *uoff, uint8_t *windows, nxz_checkpoint_stream_t *streams, void *stream)
{
	if (!index_args_ok(c, fmt, jobs, n, span, cp_cap, cbit, uoff, streams)) return -EINVAL;
	return index_launch(c, jobs, n, stream, "checkpoint index launch", [&](const uint32_t *order, hipStream_t s) {
		return nxz_launch_checkpoint_index(fmt, jobs, n, span, cp_cap, cbit, uoff, windows, streams, order, s);
	});
}

// Ranges of one stream through its checkpoint index: nxz_bgzf_read_ranges with segments for members.  The map is the index check of
// nxz_checkpoint.hip inside nxz_bgzf.hip's; a chunk is its segments' inputs staged, nxz_batch_decompress on them and the verdicts.
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
	RangeSteps steps;
	steps.map = [&](uint8_t *ws) {
		int rc = nxz_launch_range_map_clear(ws, n, L, s);
		if (!rc) rc = nxz_launch_checkpoint_check(src_len, cbit, uoff, L, ws, s);
		if (!rc) rc = nxz_launch_range_map_ranges(uoff, L, ranges, n, offsets, status, ws, s);
		if (!rc) rc = nxz_launch_checkpoint_inmax(cbit, uoff, n, L, ws, s);
		return launched("checkpoint map launch", rc);
	};
	steps.chunk = [&](uint8_t *ws, uint64_t k0, uint64_t cnt, const RangeSlots &sl) {
		int rc = launched("checkpoint stage launch", nxz_launch_checkpoint_stage(src, cbit, uoff, windows, n, L, ws, k0, cnt, sl.islots, sl.istride,
											 sl.oslots, sl.ostride, sl.jobs, s));
		if (!rc) rc = batch_decompress(c, sl.jobs, (size_t)cnt, sl.results, nullptr, s, 0);
		return rc ? rc : launched("checkpoint verdict launch", nxz_launch_checkpoint_verdict(uoff, n, L, ws, k0, cnt, sl.results, sl.frames, s));
	};
	steps.input_slots = true;
	steps.gather_what = "checkpoint gather launch"; steps.zero_what = "checkpoint zero launch";
	return read_ranges_locked(c, s, steps, uoff, L, n, dst, dst_cap, offsets, status, out_len, decoded);
}

// ---------------------------------------------------------------------------
// Checkpoints inside blocks (nxz_checkpoint_fine.hip, the rules in nxz_checkpoint_fine.h): the two calls above with a state entry a
// checkpoint.  The index is the same single launch; the read is the same driver with a check and a job step of its own.
// ---------------------------------------------------------------------------
extern "C" int nxz_batch_checkpoint_index_fine(nxz_ctx_t *c, int fmt, const nxz_batch_job_t *jobs, size_t n, uint64_t span, uint32_t cp_cap,
					       uint64_t *cbit, uint64_t *uoff, nxz_checkpoint_state_t *state, uint8_t *windows,
					       nxz_checkpoint_stream_t *streams, void *stream)
{
	if (!index_args_ok(c, fmt, jobs, n, span, cp_cap, cbit, uoff, streams) || !nxz_cpf_span_ok(span) || (n && !state)) return -EINVAL;
	return index_launch(c, jobs, n, stream, "fine checkpoint index launch", [&](const uint32_t *order, hipStream_t s) {
		return nxz_launch_checkpoint_index_fine(fmt, jobs, n, span, cp_cap, cbit, uoff, state, windows, streams, order, s);
	});
}

// The index with its windows from the source alone (nxz_checkpoint_build.hip): the same single launch, the walk with a ring of the
// last 32 KiB of output.  state NULL: the coarse rule, any span; else the fine rule and its span.  jobs[i].dst is never looked at.
extern "C" int nxz_batch_checkpoint_build(nxz_ctx_t *c, int fmt, const nxz_batch_job_t *jobs, size_t n, uint64_t span, uint32_t cp_cap,
					  uint64_t *cbit, uint64_t *uoff, nxz_checkpoint_state_t *state, uint8_t *windows,
					  nxz_checkpoint_stream_t *streams, void *stream)
{
	if (!index_args_ok(c, fmt, jobs, n, span, cp_cap, cbit, uoff, streams) || (state && !nxz_cpf_span_ok(span)) || (n && !windows)) return -EINVAL;
	return index_launch(c, jobs, n, stream, "checkpoint build launch", [&](const uint32_t *order, hipStream_t s) {
		return nxz_launch_checkpoint_build(fmt, jobs, n, span, cp_cap, cbit, uoff, state, windows, streams, order, s);
	});
}

// The segments' jobs bring NXZ_JOB_SUSPEND_WHEN_FULL, which the stream-per-wavefront kernel honours and the stream-per-lane kernel
// does not.  A chunk is at most 16 384 jobs (bgzf_chunk_members), a third of what sends a batch to the lane kernel by its size
// (nxz_batch.cpp), and by default it goes to the workgroup kernel, which hands every job with history or resume state -- and every
// fresh one whose output does not fit or whose source ends early -- to the wavefront kernel.  The one way to the lane kernel is
// the tuning knob NXZ_INFLATE_LANES_MIN: with it set these chunks are kept off the lane kernel (force 2).  Force 2 rules out the
// lane and the workgroup kernel, no more: a chunk of 64 jobs or fewer may still take the cut route (nxz_inflate_cut.hip), as it may
// with NXZ_INFLATE_WG=0 or NXZ_INFLATE_CUT=1 and no force at all.  That route decodes its pieces without the flag and hands every
// stream whose pieces do not end as planned -- a target that fills among them -- to the wavefront kernel with the job as it came,
// flag included; tests/test_gpu_checkpoints_fine.py reads through both knobs.
static int fine_chunk_route()
{
	return getenv("NXZ_INFLATE_LANES_MIN") ? 2 : 0;
}

extern "C" int nxz_checkpoint_read_ranges_fine(nxz_ctx_t *c, const uint8_t *src, uint64_t src_len, const uint64_t *cbit, const uint64_t *uoff,
					       const nxz_checkpoint_state_t *state, const uint8_t *windows, uint64_t nidx, const nxz_bgzf_range_t *ranges,
					       size_t n, uint8_t *dst, uint64_t dst_cap, uint64_t *offsets, uint32_t *status, uint64_t *out_len,
					       uint64_t *decoded, void *stream)
{
	if (out_len) *out_len = 0;
	if (decoded) *decoded = 0;
	if (!c || !src || !cbit || !uoff || !state || !offsets || nidx < 2 || nidx > 0xffffffffull || (!windows && nidx > 2) || (n && (!ranges || !status)) ||
	    n >= (1ull << 31))
		return -EINVAL;
	if (forked_child()) return -ENODEV;
	(void)hipSetDevice(c->device);
	hipStream_t s = (hipStream_t)stream;
	std::lock_guard<std::mutex> use(*frame_mutex(c, s));
	const uint64_t L = nidx - 1;
	RangeSteps steps;
	steps.map = [&](uint8_t *ws) {
		int rc = nxz_launch_range_map_clear(ws, n, L, s);
		if (!rc) rc = nxz_launch_checkpoint_check_fine(src_len, cbit, uoff, state, L, ws, s);
		if (!rc) rc = nxz_launch_range_map_ranges(uoff, L, ranges, n, offsets, status, ws, s);
		if (!rc) rc = nxz_launch_checkpoint_inmax(cbit, uoff, n, L, ws, s);
		return launched("fine checkpoint map launch", rc);
	};
	steps.chunk = [&](uint8_t *ws, uint64_t k0, uint64_t cnt, const RangeSlots &sl) {
		int rc = nxz_launch_checkpoint_stage(src, cbit, uoff, windows, n, L, ws, k0, cnt, sl.islots, sl.istride, sl.oslots, sl.ostride, sl.jobs, s);
		if (!rc) rc = nxz_launch_checkpoint_jobs_fine(src, cbit, state, n, L, ws, k0, cnt, sl.jobs, sl.dht, s);
		if ((rc = launched("fine checkpoint stage launch", rc)) != 0) return rc;
		if ((rc = batch_decompress(c, sl.jobs, (size_t)cnt, sl.results, sl.dht, s, fine_chunk_route())) != 0) return rc;
		return launched("fine checkpoint verdict launch", nxz_launch_checkpoint_verdict(uoff, n, L, ws, k0, cnt, sl.results, sl.frames, s));
	};
	steps.input_slots = true;
	steps.dht_slots = true;
	steps.gather_what = "fine checkpoint gather launch"; steps.zero_what = "fine checkpoint zero launch";
	return read_ranges_locked(c, s, steps, uoff, L, n, dst, dst_cap, offsets, status, out_len, decoded);
}

// ---------------------------------------------------------------------------
// Ranges across all the rows of a batch's index (nxz_checkpoint_batch.hip, the rules in nxz_checkpoint_batch.h): the same driver once
// more.  The batch is ONE index of n_jobs * (cp_cap + 1) entries with a uoff of its own in BUF_RNG_BATCH; a row that is not good
// costs its ranges their bytes (NXZ_RANGE_BAD_STREAM), never the call (ctl[0] stays 0: no -EILSEQ).  With state a chunk is the fine
// reader's, else the coarse reader's; its segments come from any of the streams.
// ---------------------------------------------------------------------------
extern "C" int nxz_batch_checkpoint_read_ranges(nxz_ctx_t *c, const nxz_batch_job_t *jobs, size_t n_jobs, uint32_t cp_cap, const uint64_t *cbit,
						const uint64_t *uoff, const nxz_checkpoint_state_t *state, const uint8_t *windows,
						const nxz_checkpoint_stream_t *streams, const nxz_batch_range_t *ranges, size_t n, uint8_t *dst,
						uint64_t dst_cap, uint64_t *offsets, uint32_t *status, uint64_t *out_len, uint64_t *decoded, void *stream)
{
	if (out_len) *out_len = 0;
	if (decoded) *decoded = 0;
	if (!c || !cbit || !uoff || !windows || !streams || !offsets || (n_jobs && !jobs) || (n && (!ranges || !status)) || n >= (1ull << 31) ||
	    !nxz_cpb_shape_ok(n_jobs, cp_cap))
		return -EINVAL;
	if (forked_child()) return -ENODEV;
	(void)hipSetDevice(c->device);
	hipStream_t s = (hipStream_t)stream;
	std::lock_guard<std::mutex> use(*frame_mutex(c, s));
	if (!n || !n_jobs) {                                                  // no range, or no row for any range to name
		HIPCHK(hipMemsetAsync(offsets, 0, (n + 1) * sizeof(uint64_t), s), return -EIO);
		if (n) HIPCHK(hipMemsetD32Async((hipDeviceptr_t)status, NXZ_RANGE_BAD_STREAM, n, s), return -EIO);
		HIPCHK(hipStreamSynchronize(s), return -EIO);
		return 0;
	}
	const uint64_t L = nxz_cpb_entries(n_jobs, cp_cap) - 1;
	uint8_t *const bws = with_scratch(c, s, [&](nxz_ctx::Scratch &sc) {
		(void)sc.buf[BUF_RNG_BATCH].grow(s, nxz_checkpoint_batch_workspace(n_jobs, cp_cap, n));
		return sc.buf[BUF_RNG_BATCH].p;
	});
	if (!bws) return -ENOMEM;
	const uint64_t *const fuoff = nxz_checkpoint_batch_uoff(bws, n_jobs, cp_cap, n);
	RangeSteps steps;
	steps.map = [&](uint8_t *ws) {
		return launched("checkpoint batch map launch", nxz_launch_checkpoint_batch_map(jobs, n_jobs, cp_cap, cbit, uoff, state, streams, ranges, n, offsets,
											       status, bws, ws, s));
	};
	steps.chunk = [&](uint8_t *ws, uint64_t k0, uint64_t cnt, const RangeSlots &sl) {
		int rc = launched("checkpoint batch stage launch", nxz_launch_checkpoint_batch_stage(jobs, n_jobs, cp_cap, cbit, uoff, state, windows, streams, n, bws, ws,
												     k0, cnt, sl.islots, sl.istride, sl.oslots, sl.ostride, sl.jobs,
												     sl.dht, s));
		if (!rc) rc = batch_decompress(c, sl.jobs, (size_t)cnt, sl.results, state ? sl.dht : nullptr, s, state ? fine_chunk_route() : 0);
		return rc ? rc : launched("checkpoint batch verdict launch", nxz_launch_checkpoint_verdict(fuoff, n, L, ws, k0, cnt, sl.results, sl.frames, s));
	};
	steps.input_slots = true;
	steps.dht_slots = state != nullptr;
	steps.gather_what = "checkpoint batch gather launch"; steps.zero_what = "checkpoint batch zero launch";
	return read_ranges_locked(c, s, steps, fuoff, L, n, dst, dst_cap, offsets, status, out_len, decoded);
}
