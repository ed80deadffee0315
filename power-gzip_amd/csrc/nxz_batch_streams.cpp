// nxz_batch_streams.cpp -- the calls of include/nxz_engine.h's device-resident interface that take one stream per device buffer: the
// bounds, nxz_batch_deflate_streams and its dictionary, indexed and parts forms, nxz_batch_inflate_streams_part, and the pinned staging
// they share.  The host's plans (block prefix, chunk walk, chunk counts, the inflate cut, the buffers' layouts) are nxz_streams_plan.h's.
#include "nxz_ctx.h"
#include "nxz_streams_plan.h"
#include "nxz_streams_index.h"
#include "nxz_streams_part.h"
#include "nxz_inflate_part.h"
#include "nxz_shuffle.h"

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
// ... and BUF_STREAMS of `d_bytes` with the staging's upload into its front queued on `s`: the buffer, or NULL and *rc
static uint8_t *streams_upload(nxz_ctx_t *c, hipStream_t s, size_t d_bytes, const uint8_t *h, size_t up_bytes, hipEvent_t ev, int *rc)
{
	uint8_t *const d = with_scratch(c, s, [&](nxz_ctx::Scratch &r) {
		(void)r.buf[BUF_STREAMS].grow(s, d_bytes);
		return r.buf[BUF_STREAMS].p;
	});
	*rc = d ? 0 : -ENOMEM;
	if (!d) return nullptr;
	HIPCHK(hipMemcpyAsync(d, h, up_bytes, hipMemcpyHostToDevice, s), *rc = -EIO; return nullptr);
	HIPCHK(hipEventRecord(ev, s), *rc = -EIO; return nullptr);
	with_scratch(c, s, [](nxz_ctx::Scratch &r) { r.up_turn++; return 0; });
	return d;
}

// What the deflate-streams drivers share (plain, dictionary, indexed; parts).  Uploaded: [descriptors][first]([second]), the same layout
// in the staging and in the device buffer; behind it in BUF_STREAMS the streams' state and a chunk's jobs, results, owners, offsets
// and output slots; then what a form adds with lay.take(), before streams_upload() of the whole.
struct StreamsBatch {
	nxz_carve lay;
	uint8_t *st_h = nullptr, *d = nullptr;                               // the staging; BUF_STREAMS
	hipEvent_t st_ev = nullptr;
	size_t up_bytes, o_first, o_second, o_state, o_jobs, o_res, o_owner, o_off, o_slots;
	uint32_t *h_first, *h_second;                                       // (h_second NULL: the form keeps none)
	uint32_t nblk, C;                                                   // the batch's blocks, and a chunk's at most
	template <class T> T *at(size_t off) const { return (T *)(d + off); }
};
// The host's one pass into the staging: the descriptors, and first[] / second[] from blocks_of (nxz_plan_prefix: a refused stream gets
// no blocks); then the shared layout.  0, or -errno (-E2BIG from 2^31 blocks) before anything is queued.
template <class Job, class F>
static int streams_plan(nxz_ctx_t *c, hipStream_t s, const Job *jobs, size_t n, bool second, F blocks_of, StreamsBatch *b)
{
	b->lay.take(n * sizeof(Job));
	b->o_first = b->lay.take((n + 1) * sizeof(uint32_t));
	b->o_second = second ? b->lay.take((n + 1) * sizeof(uint32_t)) : 0;
	b->up_bytes = b->lay.end;
	const int rc = streams_staging(c, s, b->up_bytes, &b->st_h, &b->st_ev);
	if (rc) return rc;
	memcpy(b->st_h, jobs, n * sizeof(Job));
	b->h_first = (uint32_t *)(b->st_h + b->o_first);
	b->h_second = second ? (uint32_t *)(b->st_h + b->o_second) : nullptr;
	const int64_t total = nxz_plan_prefix(n, b->h_first, b->h_second, blocks_of);
	if (total < 0) return -E2BIG;
	b->nblk = (uint32_t)total;
	const size_t C = b->C = std::min(streams_chunk(), b->nblk);
	b->o_state = b->lay.take(n * sizeof(nxz_stream_state_t));
	b->o_jobs = b->lay.take(C * sizeof(nxz_batch_job_t)); b->o_res = b->lay.take(C * sizeof(nxz_batch_result_t));
	b->o_owner = b->lay.take(C * sizeof(uint32_t)); b->o_off = b->lay.take(C * sizeof(uint64_t));
	b->o_slots = b->lay.take(C * NXZ_STREAMS_SLOT);
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
	const Entered in(c, stream, n != 0);
	if (in.rc != 1) return in.rc;
	if (n >= (1u << 31)) return -E2BIG;
	hipStream_t s = in.s;
	const uint32_t H = nxz_streams_window(hist_max), B = nxz_streams_block_bytes(hist_max), ns = (uint32_t)n;
	// the first block's window, and whether the chunks' first blocks go apart from the rest
	const uint32_t h0 = dict ? nxz_streams_dict_window(dict->len, hist_max) : 0;
	const bool split = h0 != 0;
	StreamsBatch b;                                                      // (second: nz[], the streams with blocks in front of each stream)
	int rc = streams_plan(c, s, jobs, n, split, [&](size_t i, bool *) {
		return (dict ? nxz_streams_dict_refusal(&jobs[i], hist_max, fmt) : nxz_streams_refusal(&jobs[i], hist_max, fmt)) ? 0 : nxz_streams_blocks(jobs[i].src_len, B);
	}, &b);
	if (rc) return rc;
	const size_t C = b.C;
	// the split's own: the jobs in launch order, their results, and where each came from
	const size_t o_ljobs = split ? b.lay.take(C * sizeof(nxz_batch_job_t)) : 0, o_lres = split ? b.lay.take(C * sizeof(nxz_batch_result_t)) : 0,
		     o_pos = split ? b.lay.take(C * sizeof(uint32_t)) : 0,
		     // the index's own, behind everything the plain call lays out: a state a stream, two slot marks a block of a chunk
		     o_ist = ix ? b.lay.take(n * sizeof(nxz_stream_index_state_t)) : 0, o_marks = ix ? b.lay.take(ix->windows ? C * 2 * sizeof(uint32_t) : 0) : 0;
	if (!(b.d = streams_upload(c, s, b.lay.end, b.st_h, b.up_bytes, b.st_ev, &rc))) return rc;
	const nxz_stream_job_t *const d_desc = b.at<nxz_stream_job_t>(0);
	const uint32_t *const d_first = b.at<uint32_t>(b.o_first), *const d_nz = split ? b.at<uint32_t>(b.o_second) : nullptr;
	nxz_stream_state_t *const d_state = b.at<nxz_stream_state_t>(b.o_state);
	nxz_batch_job_t *const d_jobs = b.at<nxz_batch_job_t>(b.o_jobs), *const d_ljobs = split ? b.at<nxz_batch_job_t>(o_ljobs) : nullptr;
	nxz_batch_result_t *const d_res = b.at<nxz_batch_result_t>(b.o_res), *const d_lres = split ? b.at<nxz_batch_result_t>(o_lres) : nullptr;
	uint32_t *const d_owner = b.at<uint32_t>(b.o_owner), *const d_pos = split ? b.at<uint32_t>(o_pos) : nullptr;
	uint64_t *const d_off = b.at<uint64_t>(b.o_off);
	uint8_t *const d_slots = b.at<uint8_t>(b.o_slots);
	nxz_stream_index_state_t *const d_ist = ix ? b.at<nxz_stream_index_state_t>(o_ist) : nullptr;
	uint32_t *const d_marks = ix && ix->windows ? b.at<uint32_t>(o_marks) : nullptr;
	rc = launched("streams prologue launch", dict ? nxz_launch_streams_dict_prologue(d_desc, ns, hist_max, fmt, level, dict->id, d_state, s)
							  : nxz_launch_streams_prologue(d_desc, ns, hist_max, fmt, level, d_state, s));
	if (rc) return rc;
	if (ix && (rc = launched("streams index prologue launch", nxz_launch_streams_index_prologue(d_desc, ns, fmt, d_state, ix->cp_cap, ix->cbit, ix->uoff,
												     d_ist, s))) != 0) return rc;
	const uint32_t op_block = nxz_crc_shift_op(B);
	for (nxz_plan_chunk k = {0, 0, 0, 0}; nxz_plan_next_chunk(b.h_first, b.nblk, b.C, &k);) {
		const uint32_t b0 = k.b0, m = k.m, i_lo = k.i_lo, ni = k.i_hi - k.i_lo + 1;
		if (split) {
			// the first blocks of streams in front of the chunk, and inside it
			const nxz_plan_count f = nxz_plan_dict_firsts(b.h_first, b.h_second, k);
			rc = launched("streams expand launch", nxz_launch_streams_dict_expand(d_desc, d_first, d_nz, ns, b0, m, hist_max, h0, f.before, f.inside, d_slots,
											      d_jobs, d_ljobs, d_owner, d_pos, s));
			if (rc) return rc;
			if ((rc = batch_compress_windowed(c, fc | 0x08, dict->d_win + nxz_streams_dict_window_at(h0), f.inside, d_ljobs, m, d_lres, s)) != 0) return rc;
			if ((rc = launched("streams gather launch", nxz_launch_streams_dict_gather(d_lres, d_pos, m, d_res, s))) != 0) return rc;
		} else {
			rc = launched("streams expand launch", nxz_launch_streams_expand(d_desc, d_first, ns, b0, m, hist_max, d_slots, d_jobs, d_owner, s));
			if (rc) return rc;
			if ((rc = nxz_batch_compress(c, fc | (H ? 0x08 : 0), d_jobs, m, nullptr, 0, d_res, nullptr, s)) != 0) return rc;
		}
		rc = nxz_launch_streams_layout(d_first, i_lo, ni, b0, m, d_jobs, d_res, hist_max, op_block, d_state, d_off, s);
		if (!rc && ix) rc = nxz_launch_streams_index_sweep(d_first, i_lo, ni, b0, m, d_jobs, d_res, d_off, hist_max, ix->span, ix->cp_cap,
								    ix->cbit, ix->uoff, d_ist, d_marks, s);
		if (!rc) rc = nxz_launch_streams_pack(d_desc, d_first, d_owner, b0, m, d_jobs, d_res, d_off, s);
		if (!rc && d_marks) rc = nxz_launch_streams_index_windows(d_desc, d_owner, m, d_marks, ix->cp_cap, ix->uoff, ix->windows, s);
		if ((rc = launched("streams pack launch", rc)) != 0) return rc;
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
// the same pinned staging and upload, the same chunk walk, BUF_STREAMS under frame_use[s], everything on `s` and no host wait.  The
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
	const Entered in(c, stream, n != 0);
	if (in.rc != 1) return in.rc;
	if (n >= (1u << 31)) return -E2BIG;
	hipStream_t s = in.s;
	const uint32_t H = nxz_streams_window(hist_max), B = nxz_streams_block_bytes(hist_max), ns = (uint32_t)n;
	StreamsBatch b;                                                      // (second: sg[], the parts with a staged first block in front of each part)
	int rc = streams_plan(c, s, jobs, n, true, [&](size_t i, bool *staged) {
		if (nxz_streams_part_refusal(&jobs[i], 0, hist_max, fmt)) return (uint64_t)0;
		*staged = nxz_streams_part_staged(&jobs[i], hist_max);
		return nxz_streams_blocks(jobs[i].src_len, B);
	}, &b);
	if (rc) return rc;
	const size_t S = std::min(b.C, b.h_second[n]);                       // the staged blocks a chunk holds at most
	const size_t o_list = b.lay.take(S * sizeof(uint32_t)), o_stage = b.lay.take(S * NXZ_STREAMS_STAGE_SLOT);
	if (!(b.d = streams_upload(c, s, b.lay.end, b.st_h, b.up_bytes, b.st_ev, &rc))) return rc;
	const nxz_stream_part_job_t *const d_desc = b.at<nxz_stream_part_job_t>(0);
	const uint32_t *const d_first = b.at<uint32_t>(b.o_first), *const d_sg = b.at<uint32_t>(b.o_second);
	nxz_stream_state_t *const d_state = b.at<nxz_stream_state_t>(b.o_state);
	nxz_batch_job_t *const d_jobs = b.at<nxz_batch_job_t>(b.o_jobs);
	nxz_batch_result_t *const d_res = b.at<nxz_batch_result_t>(b.o_res);
	uint32_t *const d_owner = b.at<uint32_t>(b.o_owner), *const d_list = b.at<uint32_t>(o_list);
	uint64_t *const d_off = b.at<uint64_t>(b.o_off);
	uint8_t *const d_slots = b.at<uint8_t>(b.o_slots), *const d_stage = b.at<uint8_t>(o_stage);
	if ((rc = launched("streams part prologue launch", nxz_launch_streams_part_prologue(d_desc, ns, hist_max, fmt, level, carry, d_state, s))) != 0) return rc;
	const uint32_t op_block = nxz_crc_shift_op(B);
	for (nxz_plan_chunk k = {0, 0, 0, 0}; nxz_plan_next_chunk(b.h_first, b.nblk, b.C, &k);) {
		const uint32_t b0 = k.b0, m = k.m;
		const nxz_plan_count sg = nxz_plan_part_staged(b.h_first, b.h_second, k);   // the staged first blocks in front of the chunk and inside it
		rc = nxz_launch_streams_part_expand(d_desc, d_first, d_sg, ns, b0, m, hist_max, sg.before, d_slots, d_stage, d_jobs, d_owner, d_list, s);
		if (!rc && sg.inside) rc = nxz_launch_streams_part_stage(d_desc, d_owner, d_list, sg.inside, d_jobs, s);
		if ((rc = launched("streams part expand launch", rc)) != 0) return rc;
		if ((rc = nxz_batch_compress(c, fc | (H ? 0x08 : 0), d_jobs, m, nullptr, 0, d_res, nullptr, s)) != 0) return rc;
		rc = nxz_launch_streams_part_layout(d_desc, d_first, k.i_lo, k.i_hi - k.i_lo + 1, b0, m, d_jobs, d_res, hist_max, op_block, d_state, d_off, s);
		if (!rc) rc = nxz_launch_streams_part_pack(d_desc, d_first, d_owner, b0, m, d_jobs, d_res, d_off, d_state, s);
		if ((rc = launched("streams part pack launch", rc)) != 0) return rc;
	}
	return launched("streams part epilogue launch", nxz_launch_streams_part_epilogue(d_desc, d_first, ns, hist_max, fmt, d_state, carry, results, s));
}

// ---------------------------------------------------------------------------
// A stream READ in parts (nxz_inflate_part.hip, the rules in nxz_inflate_part.h): per chunk open -> stage -> the raw batch on the
// derived jobs with their table slots as dht_io -> close, everything on `s` and no host wait; the same pinned staging and upload,
// BUF_STREAMS under frame_use[s].  What the host cannot see is the carry -- the phase, the window that counts, the tail --, so its
// one pass sets aside the most a part's slot can take (nxz_inflate_part_slot_bound) and cuts the batch into chunks by that
// (nxz_plan_inflate_cut): a chunk ends in front of the stream that would carry its slots beyond NXZ_INFLATE_PART_SCRATCH bytes (a
// stream larger than that is a chunk of its own) or at NXZ_INFLATE_PART_CHUNK_STREAMS streams.  off[] goes up beside the descriptors: a
// chunk of m streams has m + 1 entries, the first 0, the last its staging bytes.  The decode is kept off the stream-per-lane kernel as
// the fine range reads are (fine_chunk_route, nxz_batch_ranges.cpp): the jobs bring NXZ_JOB_SUSPEND_WHEN_FULL.
// ---------------------------------------------------------------------------
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
	const Entered in(c, stream, n != 0);
	if (in.rc != 1) return in.rc;
	if (n >= (1u << 31)) return -E2BIG;
	for (size_t i = 0; i < n; i++)
		if (nxz_inflate_part_slot_bound(&jobs[i]) > 0xffffffffull) return -E2BIG;   // (window + tail + part is a raw job's src_len)
	hipStream_t s = in.s;
	// what is uploaded: [descriptors][off], the same layout in the staging and in the device buffer (a chunk a stream at the worst: 2 n entries)
	nxz_carve lay;
	lay.take(n * sizeof(nxz_inflate_part_job_t));
	const size_t o_off = lay.take(2 * n * sizeof(uint64_t)), up_bytes = lay.end;
	uint8_t *st_h = nullptr;
	hipEvent_t st_ev = nullptr;
	int rc = streams_staging(c, s, up_bytes, &st_h, &st_ev);
	if (rc) return rc;
	// one pass over the streams: the chunks and the slots' offsets inside them
	uint64_t *const h_off = (uint64_t *)(st_h + o_off);
	memcpy(st_h, jobs, n * sizeof(nxz_inflate_part_job_t));
	const nxz_plan_cut cut = nxz_plan_inflate_cut(n, inflate_part_scratch(), NXZ_INFLATE_PART_CHUNK_STREAMS, h_off,
						      [&](size_t i) { return nxz_inflate_part_slot_bound(&jobs[i]); });
	const size_t C = cut.max_cnt;
	const size_t o_work = lay.take(C * sizeof(nxz_inflate_part_work_t)), o_jobs = lay.take(C * sizeof(nxz_batch_job_t)), o_res = lay.take(C * sizeof(nxz_batch_result_t)),
		     o_dht = lay.take(C * sizeof(nxz_batch_dht_t)), o_stage = lay.take((size_t)cut.max_bytes);
	uint8_t *const d = streams_upload(c, s, lay.end, st_h, up_bytes, st_ev, &rc);
	if (!d) return rc;
	const nxz_inflate_part_job_t *const d_desc = (const nxz_inflate_part_job_t *)d;
	const uint64_t *const d_off = (const uint64_t *)(d + o_off);
	nxz_inflate_part_work_t *const d_work = (nxz_inflate_part_work_t *)(d + o_work);
	nxz_batch_job_t *const d_jobs = (nxz_batch_job_t *)(d + o_jobs);
	nxz_batch_result_t *const d_res = (nxz_batch_result_t *)(d + o_res);
	nxz_batch_dht_t *const d_dht = (nxz_batch_dht_t *)(d + o_dht);
	uint8_t *const d_stage = d + o_stage;
	size_t e0 = 0;
	for (size_t i0 = 0; i0 < n;) {
		const uint32_t m = nxz_plan_cut_streams(h_off, e0, cut.entries);
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

// ---------------------------------------------------------------------------
// The byte-shuffle filter (nxz_shuffle.hip, the rules in nxz_shuffle.h): the same pinned staging and upload, BUF_STREAMS under
// frame_use[s], everything on `s` and no host wait.  The host's one pass (nxz_shuffle_plan_batch) writes what the kernel reads of a job,
// the tile prefix and the statuses -- every refusal is the host's to see -- and all three go up in one copy; then the statuses' copy
// and one grid over the tiles.
// ---------------------------------------------------------------------------
extern "C" uint32_t nxz_shuffle_tile_elems(uint32_t elem)
{
	return elem && elem <= NXZ_SHUFFLE_ELEM_MAX ? nxz_shuffle_tile_elems_of(elem) : 0;
}

static int batch_shuffle(nxz_ctx_t *c, const nxz_shuffle_job_t *jobs, size_t n, uint32_t *status, void *stream, int undo)
{
	if (!c || (n && (!jobs || !status))) return -EINVAL;
	const Entered in(c, stream, n != 0);
	if (in.rc != 1) return in.rc;
	if (n >= (1u << 31)) return -E2BIG;
	hipStream_t s = in.s;
	nxz_carve lay;
	lay.take(n * sizeof(nxz_shuffle_plan_t));
	const size_t o_first = lay.take((n + 1) * sizeof(uint32_t)), o_st = lay.take(n * sizeof(uint32_t)), up_bytes = lay.end;
	uint8_t *st_h = nullptr;
	hipEvent_t st_ev = nullptr;
	int rc = streams_staging(c, s, up_bytes, &st_h, &st_ev);
	if (rc) return rc;
	const int64_t tiles = nxz_shuffle_plan_batch(jobs, n, (nxz_shuffle_plan_t *)st_h, (uint32_t *)(st_h + o_first), (uint32_t *)(st_h + o_st));
	if (tiles < 0) return -E2BIG;
	const uint8_t *const d = streams_upload(c, s, lay.end, st_h, up_bytes, st_ev, &rc);
	if (!d) return rc;
	return launched("shuffle launch", nxz_launch_shuffle((const nxz_shuffle_plan_t *)d, (const uint32_t *)(d + o_first), (const uint32_t *)(d + o_st),
							     (uint32_t)n, (uint32_t)tiles, undo, status, s));
}

extern "C" int nxz_batch_shuffle(nxz_ctx_t *c, const nxz_shuffle_job_t *jobs, size_t n, uint32_t *status, void *stream)
{
	return batch_shuffle(c, jobs, n, status, stream, 0);
}

extern "C" int nxz_batch_unshuffle(nxz_ctx_t *c, const nxz_shuffle_job_t *jobs, size_t n, uint32_t *status, void *stream)
{
	return batch_shuffle(c, jobs, n, status, stream, 1);
}
