// nxz_batch_ranges.cpp -- the calls of include/nxz_engine.h's device-resident interface that find their way into streams through an
// index: BGZF discovery, unpack and member index, the checkpoint index calls, and every range read (a BGZF image's, one stream's
// through its checkpoints, coarse and fine, and a batch's).  The framed decode they run is nxz_batch_framed.cpp's (framed_locked).
#include "nxz_ctx.h"
#include "nxz_streams_plan.h"
#include "nxz_checkpoint_fine.h"
#include "nxz_checkpoint_batch.h"

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
	const Entered in(c, stream, true);
	if (in.rc != 1) return in.rc;
	if (len < 26) return -EILSEQ;
	hipStream_t s = in.s;
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
	const Entered in(c, stream, true);
	if (in.rc != 1) return in.rc;
	if (len < 26) return -EILSEQ;
	uint64_t ctl[4] = {0, 0, 0, 0};
	nxz_batch_job_t *jobs = nullptr;
	int rc = bgzf_discover_locked(c, packed, len, nullptr, uoff, max_members, coff, in.s, ctl, &jobs);
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
// what the calls do differently: the slots they ask for, the names of their launches, and two callables that queue on `s`, report
// their own failures (launched) and return 0 or the error:
//   map(ws)                 the map kernels into ws (BUF_RNG): ctl = ws[0..5] as nxz_device.h lists them
//   chunk(ws, k0, cnt, sl)  staging, decode and verdict of needed members k0 .. k0 + cnt - 1, so that sl.frames and sl.results are
//                           what nxz_launch_bgzf_gather looks at
struct RangeSteps {
	bool input_slots;                 // the chunk stages its inputs: slots of ctl[5] bytes (else none, istride 0)
	bool dht_slots;                   // the chunk's jobs resume inside dynamic blocks: a nxz_batch_dht_t a member (else none, NULL)
	const char *gather_what, *zero_what;
};
template <class Map, class Chunk>
static int read_ranges_locked(nxz_ctx_t *c, hipStream_t s, const RangeSteps &steps, Map map, Chunk chunk, const uint64_t *uoff, uint64_t L, size_t n, uint8_t *dst,
			      uint64_t dst_cap, uint64_t *offsets, uint32_t *status, uint64_t *out_len, uint64_t *decoded)
{
	uint8_t *const ws = with_scratch(c, s, [&](nxz_ctx::Scratch &sc) {
		(void)sc.buf[BUF_RNG].grow(s, nxz_bgzf_ranges_workspace(n, L));
		return sc.buf[BUF_RNG].p;
	});
	if (!ws) return -ENOMEM;
	int rc = map(ws);
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
	RangeSlots sl;
	sl.ostride = stride_of(ctl[4]);
	sl.istride = steps.input_slots ? stride_of(ctl[5]) : 0;
	const uint64_t per = std::min(needed, std::min(bgzf_chunk_members(), std::max<uint64_t>(1, (1ull << 30) / std::max(sl.istride, sl.ostride))));
	nxz_carve lay;                                                       // (the table slots, where there are none, an empty array at the padded end)
	const size_t o_in = lay.take(per * sl.istride), o_out = lay.take(per * sl.ostride), o_jobs = lay.take(per * sizeof(nxz_batch_job_t)),
		     o_frames = lay.take(per * sizeof(nxz_batch_frame_t)), o_res = lay.take(per * sizeof(nxz_batch_result_t)),
		     o_dht = lay.take(steps.dht_slots ? per * sizeof(nxz_batch_dht_t) : 0);
	uint8_t *const slots = with_scratch(c, s, [&](nxz_ctx::Scratch &sc) {
		(void)sc.buf[BUF_RNG_SLOTS].grow(s, lay.end);
		return sc.buf[BUF_RNG_SLOTS].p;
	});
	if (!slots) return -ENOMEM;
	sl.islots = slots + o_in; sl.oslots = slots + o_out;
	sl.jobs = (nxz_batch_job_t *)(slots + o_jobs);
	sl.frames = (nxz_batch_frame_t *)(slots + o_frames);
	sl.results = (nxz_batch_result_t *)(slots + o_res);
	sl.dht = steps.dht_slots ? (nxz_batch_dht_t *)(slots + o_dht) : nullptr;
	for (uint64_t k0 = 0; k0 < needed; k0 += per) {
		const uint64_t cnt = std::min(per, needed - k0);
		if ((rc = chunk(ws, k0, cnt, sl)) != 0) return rc;
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
	const Entered in(c, stream, true);
	if (in.rc != 1) return in.rc;
	hipStream_t s = in.s;
	const uint64_t L = nidx - 1;
	const auto map = [&](uint8_t *ws) {
		return launched("bgzf map launch", nxz_launch_bgzf_map(packed, packed_len, coff, uoff, L, kind, ranges, n, offsets, status, ws, s));
	};
	const auto chunk = [&](uint8_t *ws, uint64_t k0, uint64_t cnt, const RangeSlots &sl) {
		const int rc = launched("bgzf jobs launch", nxz_launch_bgzf_jobs(packed, coff, uoff, n, L, ws, k0, cnt, sl.oslots, sl.ostride, sl.jobs, s));
		return rc ? rc : framed_locked(c, NXZ_FMT_GZIP, sl.jobs, (size_t)cnt, sl.results, sl.frames, s);
	};
	const RangeSteps steps = {false, false, "bgzf gather launch", "bgzf zero launch"};
	return read_ranges_locked(c, s, steps, map, chunk, uoff, L, n, dst, dst_cap, offsets, status, out_len, decoded);
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
// ... and how they go on: launch(order, s) as ordered_launch runs it
template <class Launch>
static int index_launch(nxz_ctx_t *c, const nxz_batch_job_t *jobs, size_t n, void *stream, const char *what, Launch launch)
{
	const Entered in(c, stream, n != 0, false);
	return in.rc != 1 ? in.rc : ordered_launch(c, in.s, jobs, n, what, [&](const uint32_t *order) { return launch(order, in.s); });
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
	const Entered in(c, stream, true);
	if (in.rc != 1) return in.rc;
	hipStream_t s = in.s;
	const uint64_t L = nidx - 1;
	const auto map = [&](uint8_t *ws) {
		int rc = nxz_launch_range_map_clear(ws, n, L, s);
		if (!rc) rc = nxz_launch_checkpoint_check(src_len, cbit, uoff, L, ws, s);
		if (!rc) rc = nxz_launch_range_map_ranges(uoff, L, ranges, n, offsets, status, ws, s);
		if (!rc) rc = nxz_launch_checkpoint_inmax(cbit, uoff, n, L, ws, s);
		return launched("checkpoint map launch", rc);
	};
	const auto chunk = [&](uint8_t *ws, uint64_t k0, uint64_t cnt, const RangeSlots &sl) {
		int rc = launched("checkpoint stage launch", nxz_launch_checkpoint_stage(src, cbit, uoff, windows, n, L, ws, k0, cnt, sl.islots, sl.istride,
											 sl.oslots, sl.ostride, sl.jobs, s));
		if (!rc) rc = batch_decompress(c, sl.jobs, (size_t)cnt, sl.results, nullptr, s, 0);
		return rc ? rc : launched("checkpoint verdict launch", nxz_launch_checkpoint_verdict(uoff, n, L, ws, k0, cnt, sl.results, sl.frames, s));
	};
	const RangeSteps steps = {true, false, "checkpoint gather launch", "checkpoint zero launch"};
	return read_ranges_locked(c, s, steps, map, chunk, uoff, L, n, dst, dst_cap, offsets, status, out_len, decoded);
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
int fine_chunk_route()
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
	const Entered in(c, stream, true);
	if (in.rc != 1) return in.rc;
	hipStream_t s = in.s;
	const uint64_t L = nidx - 1;
	const auto map = [&](uint8_t *ws) {
		int rc = nxz_launch_range_map_clear(ws, n, L, s);
		if (!rc) rc = nxz_launch_checkpoint_check_fine(src_len, cbit, uoff, state, L, ws, s);
		if (!rc) rc = nxz_launch_range_map_ranges(uoff, L, ranges, n, offsets, status, ws, s);
		if (!rc) rc = nxz_launch_checkpoint_inmax(cbit, uoff, n, L, ws, s);
		return launched("fine checkpoint map launch", rc);
	};
	const auto chunk = [&](uint8_t *ws, uint64_t k0, uint64_t cnt, const RangeSlots &sl) {
		int rc = nxz_launch_checkpoint_stage(src, cbit, uoff, windows, n, L, ws, k0, cnt, sl.islots, sl.istride, sl.oslots, sl.ostride, sl.jobs, s);
		if (!rc) rc = nxz_launch_checkpoint_jobs_fine(src, cbit, state, n, L, ws, k0, cnt, sl.jobs, sl.dht, s);
		if ((rc = launched("fine checkpoint stage launch", rc)) != 0) return rc;
		if ((rc = batch_decompress(c, sl.jobs, (size_t)cnt, sl.results, sl.dht, s, fine_chunk_route())) != 0) return rc;
		return launched("fine checkpoint verdict launch", nxz_launch_checkpoint_verdict(uoff, n, L, ws, k0, cnt, sl.results, sl.frames, s));
	};
	const RangeSteps steps = {true, true, "fine checkpoint gather launch", "fine checkpoint zero launch"};
	return read_ranges_locked(c, s, steps, map, chunk, uoff, L, n, dst, dst_cap, offsets, status, out_len, decoded);
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
	const Entered in(c, stream, true);
	if (in.rc != 1) return in.rc;
	hipStream_t s = in.s;
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
	const auto map = [&](uint8_t *ws) {
		return launched("checkpoint batch map launch", nxz_launch_checkpoint_batch_map(jobs, n_jobs, cp_cap, cbit, uoff, state, streams, ranges, n, offsets,
											       status, bws, ws, s));
	};
	const auto chunk = [&](uint8_t *ws, uint64_t k0, uint64_t cnt, const RangeSlots &sl) {
		int rc = launched("checkpoint batch stage launch", nxz_launch_checkpoint_batch_stage(jobs, n_jobs, cp_cap, cbit, uoff, state, windows, streams, n, bws, ws,
												     k0, cnt, sl.islots, sl.istride, sl.oslots, sl.ostride, sl.jobs,
												     sl.dht, s));
		if (!rc) rc = batch_decompress(c, sl.jobs, (size_t)cnt, sl.results, state ? sl.dht : nullptr, s, state ? fine_chunk_route() : 0);
		return rc ? rc : launched("checkpoint batch verdict launch", nxz_launch_checkpoint_verdict(fuoff, n, L, ws, k0, cnt, sl.results, sl.frames, s));
	};
	const RangeSteps steps = {true, state != nullptr, "checkpoint batch gather launch", "checkpoint batch zero launch"};
	return read_ranges_locked(c, s, steps, map, chunk, fuoff, L, n, dst, dst_cap, offsets, status, out_len, decoded);
}
