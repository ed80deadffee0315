// nxz_device.h -- structures shared by the host side of the engine and its HIP kernels.
#ifndef NXZ_DEVICE_H
#define NXZ_DEVICE_H
#include <stdint.h>
#include <stddef.h>
#include "../../include/nxz_engine.h"

// A DHT bit string (RFC1951 3.2.7, HLIT first, as carried in the CPB: inc_nx/nxu.h:390-393)
// parsed once on the device into what the encoder needs.
typedef struct nxz_dht_prepared {
	uint32_t dhtlen;      // bits
	uint32_t status;      // 0 ok, else NXZ_CC_INVALID_DHT
	uint32_t dhtw[74];    // the bit string, zero padded
	uint32_t ll[288];     // bit-reversed code | length << 16 (length 0 = symbol absent)
	uint32_t d[32];
} nxz_dht_prepared_t;

// What the LZ77 kernel hands to the entropy stage, per job (device scratch, NXZ_TOK_STRIDE bytes apart):
// two bitmaps over the positions of the block (bit p of the first: a literal token starts at
// position p; of the second: a match token starts there) and the match tokens in parse order,
// one dword each: length - 3 | (distance - 1) << 8.
// Who writes the job's result record: the LZ77 kernel spbc, sfbt (its match count) and zeros in the rest; the entropy
// kernel, launched behind it on the same jobs and results, cc, tpbc, tebc, sfbt = 0 and crc / adler, which it makes of the
// source it reads anyway (nxz_cksum_slices.h).  Nothing may read crc / adler between the two launches.  The forms of
// the LZ77 kernel that finish the block themselves (NXZ_LZ77_FUSED_FHT, NXZ_LZ77_FUSED_GEN) write every field.
#define NXZ_TOK_LITBITS    0u
#define NXZ_TOK_MATCHBITS  8192u
#define NXZ_TOK_RECORDS    16384u
#define NXZ_TOK_STRIDE     106496u     /* 16 KiB of bitmaps + 65536 / 3 records at most */
#define NXZ_TOK_MAXREC     ((NXZ_TOK_STRIDE - NXZ_TOK_RECORDS) / 4u)

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
// Pointers into device memory are used through address space 1: generic ("flat") accesses make
// the compiler drain the LDS queue completely at every wait that follows them.
#define NXZ_GLOBAL_AS __attribute__((address_space(1)))
extern "C" {
#define NXZ_LZ77_MAX_GRID 512          /* workgroups of one LZ77 launch (one per CU) */
#define NXZ_LZ77_FUSED_FHT 2            /* nxz_launch_lz77 count: the kernel writes the finished fixed-Huffman block itself (no entropy launch) */
#define NXZ_LZ77_FUSED_GEN 3            /* ... the finished dynamic-Huffman block, with the table made of its own counts (`tokens`: nxz_lz77_gen_scratch_bytes() of scratch; counts may be NULL) */
size_t nxz_lz77_cand2_bytes(void);     /* scratch of a launch: the second bucket entries in transit */
size_t nxz_lz77_gen_scratch_bytes(void);
int nxz_launch_lz77(int count, const nxz_batch_job_t *jobs, size_t n, uint8_t *tokens, uint16_t *cand2, nxz_batch_result_t *results,
		    uint32_t *counts, uint32_t *job_counter, hipStream_t stream);
/* nxz_symcount.hip: counts[i * 316 ..] of jobs[i] from the bitmaps and records at tokens + i * NXZ_TOK_STRIDE and the source.
 * nxz_launch_lz77 with count == 1 launches it itself, behind the LZ77 kernel's form that does not count */
int nxz_launch_symcount(const nxz_batch_job_t *jobs, size_t n, const uint8_t *tokens, uint32_t *counts, hipStream_t stream);
int nxz_launch_encode(int dht, int table_per_job, const nxz_batch_job_t *jobs, size_t n, const uint8_t *tokens,
		      const nxz_dht_prepared_t *tables, nxz_batch_result_t *results, hipStream_t stream);
int nxz_launch_dhtgen(const uint32_t *counts, size_t n, nxz_dht_prepared_t *prepared,
		      nxz_batch_dht_t *tables, hipStream_t stream);   /* device dhtgen: counts[n][316] -> tables (either output may be NULL) */
int nxz_launch_dht_prepare(const nxz_batch_dht_t *dht, size_t n, nxz_dht_prepared_t *out, hipStream_t stream);
int nxz_launch_wrap(const nxz_batch_job_t *jobs, size_t n, nxz_batch_result_t *results, hipStream_t stream);          /* round 1's kernel (kept for comparison: NXZ_WRAP_OLD=1) */
int nxz_launch_wrap_sliced(const nxz_batch_job_t *jobs, size_t n, nxz_batch_result_t *results, hipStream_t stream);   /* nxz_inflate_lanes.hip: the checksum kernel's pass, storing as it goes */
int nxz_launch_inflate(const nxz_batch_job_t *jobs, size_t n, nxz_batch_result_t *results,
		       nxz_batch_dht_t *dht_io, int window_in_lds, const uint32_t *order, hipStream_t stream);   /* order: NULL, or nxz_launch_order_by_length's */
/* the jobs' indices by falling source length, in `workspace` (nxz_order_workspace(n) bytes); NULL when it cannot be made */
size_t nxz_order_workspace(size_t n);
const uint32_t *nxz_launch_order_by_length(const nxz_batch_job_t *jobs, size_t n, uint8_t *workspace, hipStream_t stream);
/* token boundaries inside dynamic blocks (nxz_inflate.hip token_sync_kernel; offsets in bits from src) */
typedef struct nxz_sync_req {
	const uint8_t *src;      /* at or in front of the block's header, 4-byte aligned if the stream is */
	uint32_t srclen;         /* bytes at src */
	uint32_t header_bit;     /* the block's header */
	uint32_t guess_bit;      /* where to look: the boundary found lies behind this bit */
	uint32_t limit_bit;      /* ... and no token looked at reaches this bit (the next block's header) */
} nxz_sync_req_t;
typedef struct nxz_sync_res { uint32_t bit; uint32_t lanes; } nxz_sync_res_t;   /* bit 0xffffffff: none found; lanes bit 31: the block's BFINAL */
size_t nxz_built_tables_bytes(void);
#define NXZ_BLOCKFIND_MORE 3u      /* nxz_launch_find_blocks: `first` holds nseg first headers, then this many further ones per segment (~0: none) */
int nxz_launch_token_sync_more(const nxz_sync_req_t *breqs, uint32_t nb, nxz_batch_dht_t *tables, void *built, uint32_t first,
			       const nxz_sync_req_t *reqs, uint32_t n, nxz_sync_res_t *res, hipStream_t stream);
int nxz_launch_token_sync(const nxz_sync_req_t *breqs, uint32_t nb, nxz_batch_dht_t *tables, void *built,
			  const nxz_sync_req_t *reqs, uint32_t n, nxz_sync_res_t *res, hipStream_t stream);
/* runs of stored blocks (nxz_blockfind.hip stored_walk_kernel) */
typedef struct nxz_walk_req { const uint8_t *src; uint64_t src_len; uint64_t bit; uint32_t rem, bfinal; } nxz_walk_req_t;
typedef struct nxz_walk_res { uint64_t bit; uint32_t flags, reserved; } nxz_walk_res_t;
int nxz_launch_stored_walk(const nxz_walk_req_t *reqs, uint32_t n, nxz_walk_res_t *res, hipStream_t stream);
int nxz_launch_inflate_w16(const nxz_batch_job_t *jobs, size_t n, nxz_batch_result_t *results, nxz_batch_dht_t *dht_io, const void *built,
			   int few_and_even, hipStream_t stream);
int nxz_launch_sample_btype(const nxz_batch_job_t *jobs, size_t n, uint32_t *out, hipStream_t stream);   /* out: pinned host word */
int nxz_launch_cksum(const nxz_batch_job_t *jobs, size_t n, nxz_batch_result_t *results, hipStream_t stream);
int nxz_launch_pack_stream(const nxz_batch_job_t *jobs, const nxz_batch_result_t *results, size_t n, uint32_t final_index,
			   uint64_t *offsets, uint8_t *packed, hipStream_t stream);
/* several callers' blocks in one batch, each caller's packed as its own stream: blocks [b0, b0 + n) are member's, block `fin`
 * (an index into the batch, 0xffffffff: none) carries BFINAL, its n + 1 offsets stand at offsets[off0 ..], its stream goes to `packed` */
typedef struct nxz_pack_member { uint32_t b0, n, fin, off0; uint8_t *packed; } nxz_pack_member_t;
int nxz_launch_pack_member_streams(const nxz_batch_job_t *jobs, const nxz_batch_result_t *results, size_t nblocks, const nxz_pack_member_t *members,
				   size_t nmembers, const uint16_t *member_of, uint64_t *offsets, hipStream_t stream);
int nxz_launch_copy_items(const void *items, uint32_t n, hipStream_t stream);
int nxz_launch_copy16(const void *src, void *dst, size_t bytes, hipStream_t stream);   /* a plain device-to-device copy, 16 bytes a lane: the roofline's measured peak */   /* items: { src, dst, uint64 bytes } */
size_t nxz_inflate_lanes_workspace(size_t n);
/* nxz_inflate_cut.hip: a batch too small to fill the device a stream per wavefront -- every stream cut inside its first block */
unsigned nxz_inflate_cut_pieces(size_t n);                                   /* pieces per stream for a batch of n (below 2: not worth it) */
size_t nxz_inflate_cut_workspace(size_t n, unsigned pieces, size_t arena);   /* device bytes: control arrays + `arena` bytes for the pieces' elements */
int nxz_launch_copy_out(const nxz_batch_job_t *jobs, const nxz_batch_result_t *results, uint8_t *const *targets, size_t n, hipStream_t stream);   /* results[i].tpbc bytes of jobs[i].dst -> targets[i] */
int nxz_launch_inflate_cut(const nxz_batch_job_t *jobs, size_t n, nxz_batch_result_t *results, nxz_batch_dht_t *dht_io,
			   unsigned pieces, uint8_t *workspace, size_t arena, hipStream_t stream);
int nxz_launch_pack_members(const nxz_batch_job_t *jobs, const nxz_batch_result_t *results, size_t n,
			    uint64_t *offsets, uint8_t *packed, hipStream_t stream);
int nxz_launch_pack_zlib(const nxz_batch_job_t *jobs, const nxz_batch_result_t *results, size_t n, uint32_t flg,
			 uint64_t *offsets, uint8_t *packed, hipStream_t stream);
/* nxz_frame.hip: zlib / gzip framing around a raw inflate batch, and the members of a BGZF image */
int nxz_launch_frame_header(int fmt, const nxz_batch_job_t *jobs, size_t n, nxz_batch_frame_t *frames, nxz_batch_job_t *derived, hipStream_t stream);
int nxz_launch_frame_trailer(const nxz_batch_job_t *jobs, size_t n, nxz_batch_result_t *results, nxz_batch_frame_t *frames, hipStream_t stream);
size_t nxz_bgzf_workspace(uint64_t len, uint64_t cap);
int nxz_launch_bgzf_discover(const uint8_t *packed, uint64_t len, uint8_t *dst, uint64_t *offsets, uint64_t max_members, uint8_t *ws,
			     uint64_t cap, nxz_batch_job_t **jobs, hipStream_t stream);   /* ws[0..3]: candidates, members, bytes covered, sum of ISIZE */
int nxz_launch_bgzf_coff(const uint8_t *packed, uint64_t len, uint8_t *ws, uint64_t cap, uint64_t max_members, uint64_t *coff, hipStream_t stream);
/* nxz_bgzf.hip: ranges of a BGZF image through its member index (ws[0..4]: index faulty, needed members, bytes, pieces, largest member) */
size_t nxz_bgzf_ranges_workspace(uint64_t n, uint64_t L);
int nxz_launch_bgzf_map(const uint8_t *packed, uint64_t packed_len, const uint64_t *coff, const uint64_t *uoff, uint64_t L, int kind,
			const nxz_bgzf_range_t *ranges, uint64_t n, uint64_t *offsets, uint32_t *status, uint8_t *ws, hipStream_t stream);
/* the map in steps, for an index of another kind (nxz_checkpoint.hip): clear, the caller's own check (ws[0] != 0: faulty), the ranges */
int nxz_launch_range_map_clear(uint8_t *ws, uint64_t n, uint64_t L, hipStream_t stream);
int nxz_launch_range_map_ranges(const uint64_t *uoff, uint64_t L, const nxz_bgzf_range_t *ranges, uint64_t n, uint64_t *offsets,
				uint32_t *status, uint8_t *ws, hipStream_t stream);
void nxz_range_map_lists(uint8_t *ws, uint64_t n, uint64_t L, const uint32_t **midx, const uint32_t **list);
int nxz_launch_bgzf_jobs(const uint8_t *packed, const uint64_t *coff, const uint64_t *uoff, uint64_t n, uint64_t L, uint8_t *ws,
			 uint64_t k0, uint64_t cnt, uint8_t *slots, uint64_t stride, nxz_batch_job_t *jobs, hipStream_t stream);
int nxz_launch_bgzf_gather(const uint64_t *uoff, uint64_t n, uint64_t L, uint64_t pieces, uint8_t *ws, const uint64_t *offsets,
			   const uint8_t *slots, uint64_t stride, uint64_t k0, uint64_t cnt, const nxz_batch_frame_t *frames,
			   const nxz_batch_result_t *results, uint8_t *dst, uint32_t *status, hipStream_t stream);
int nxz_launch_bgzf_zero(uint64_t n, const uint64_t *offsets, const uint32_t *status, uint8_t *dst, hipStream_t stream);
int nxz_launch_inflate_lanes(const nxz_batch_job_t *jobs, size_t n, nxz_batch_result_t *results,
			     nxz_batch_dht_t *dht_io, uint8_t *workspace, int init_fixed, hipStream_t stream);
/* nxz_inflate_wg.hip: a stream per workgroup, source, output and tables in LDS; what it cannot do goes a stream per wavefront behind it */
size_t nxz_inflate_wg_workspace(size_t n);
int nxz_launch_inflate_wg(const nxz_batch_job_t *jobs, size_t n, nxz_batch_result_t *results, nxz_batch_dht_t *dht_io,
			  uint8_t *wg_ws, const uint32_t *order, uint8_t *const *targets, hipStream_t stream);   /* targets (may be NULL): the outputs there too, in the checksum pass */
int nxz_launch_cksum_copy(const nxz_batch_job_t *jobs, size_t n, nxz_batch_result_t *results, uint8_t *const *targets, hipStream_t stream);
/* one preset dictionary for all jobs of a batch (nxz_dict.h; the nxz_batch_*_dict calls) */
int nxz_launch_dict_jobs(const nxz_batch_job_t *in, size_t n, uint32_t W, nxz_batch_job_t *out, hipStream_t stream);          /* the caller's jobs with the deflate window "in front" */
int nxz_launch_dict_finish(const nxz_batch_job_t *in, size_t n, uint32_t W, nxz_batch_result_t *results, hipStream_t stream); /* the jobs that were not taken: NXZ_CC_INVALID_OP */
int nxz_launch_lz77_dict(int count, const nxz_batch_job_t *jobs, size_t n, uint8_t *tokens, uint16_t *cand2, nxz_batch_result_t *results,
			 uint32_t *counts, uint32_t *job_counter, const uint8_t *dict, hipStream_t stream);
int nxz_launch_inflate_wg_dict(const nxz_batch_job_t *jobs, size_t n, nxz_batch_result_t *results, uint8_t *wg_ws, const uint32_t *order,
			       const uint8_t *dwin, uint32_t dlen, uint32_t src_min, hipStream_t stream);   /* dwin: 32 KiB, its last dlen bytes the inflate window; streams below src_min source bytes: a wavefront each */
int nxz_launch_inflate_order_only_dict(const nxz_batch_job_t *jobs, size_t nslots, nxz_batch_result_t *results, const uint32_t *order,
				       const uint8_t *dict_end, uint32_t dlen, uint32_t src_below, hipStream_t stream);
int nxz_launch_pack_zlib_dict(const nxz_batch_job_t *jobs, const nxz_batch_result_t *results, size_t n, uint32_t flg, uint32_t dictid,
			      uint64_t *offsets, uint8_t *packed, hipStream_t stream);
int nxz_launch_frame_header_dict(int fmt, const nxz_batch_job_t *jobs, size_t n, nxz_batch_frame_t *frames, nxz_batch_job_t *derived,
				 uint32_t dictid, hipStream_t stream);
/* nxz_inflate_size.hip: what the streams would produce, a wavefront each, nothing written but results (nxz_size.h has the rules).
 * order: NULL, or nxz_launch_order_by_length's; dict_window: how far every job's distances may reach besides its own hist_len
 * (a shared dictionary's inflate window; jobs that say NXZ_JOB_NO_DICT do not get it) */
int nxz_launch_inflate_size(const nxz_batch_job_t *jobs, size_t n, nxz_batch_result_t *results, const uint32_t *order,
			    uint32_t dict_window, hipStream_t stream);
int nxz_launch_size_trailer(const nxz_batch_job_t *jobs, size_t n, nxz_batch_result_t *results, nxz_batch_frame_t *frames, hipStream_t stream);   /* nxz_launch_frame_trailer without the checksum comparison */
/* nxz_inflate_verify.hip: the same walk with the output passing through a 32 KiB ring in LDS that is checksummed on the way
 * (nxz_verify.h has the rules): the size record with crc and adler.  dwin: NULL, or a shared dictionary's 32 KiB image whose last
 * dlen bytes are its inflate window -- the window of every job that does not say NXZ_JOB_NO_DICT */
int nxz_launch_inflate_verify(const nxz_batch_job_t *jobs, size_t n, nxz_batch_result_t *results, const uint32_t *order,
			      const uint8_t *dwin, uint32_t dlen, hipStream_t stream);
/* nxz_gzip_members.hip: multi-member gzip jobs (nxz_gzip_members.h has the rules).  The index: a wavefront a job, member after member
 * inside the kernel.  The decode: expand (records checked, the plan, the members as framed jobs in ws: nxz_gzip_members_workspace
 * bytes) -> the framed decode of *xjobs -> join (the verdicts back into members and streams) */
int nxz_launch_gzip_members_index(const nxz_batch_job_t *jobs, size_t n, uint32_t member_cap, nxz_gzip_member_t *members,
				  nxz_gzip_stream_t *streams, const uint32_t *order, hipStream_t stream);
size_t nxz_gzip_members_workspace(size_t n, size_t total_members);
int nxz_launch_gzip_members_expand(const nxz_batch_job_t *jobs, size_t n, uint32_t member_cap, const nxz_gzip_member_t *members,
				   nxz_gzip_stream_t *streams, size_t total_members, uint8_t *ws, nxz_batch_job_t **xjobs,
				   nxz_batch_result_t **xresults, nxz_batch_frame_t **xframes, hipStream_t stream);
int nxz_launch_gzip_members_join(size_t n, uint32_t member_cap, nxz_gzip_member_t *members, nxz_gzip_stream_t *streams,
				 size_t total_members, uint8_t *ws, hipStream_t stream);
/* nxz_checkpoint.hip: the checkpoint index of raw, zlib and gzip streams and range reads through it (nxz_checkpoint.h has the rules).
 * The index: a wavefront a job; the windows: a second launch over the stored checkpoints.  The range read's steps around
 * nxz_batch_decompress: check (ws[0]: index faulty, ws[5]: the largest [window][source] of a needed segment), stage (the jobs of
 * needed segments k0 .. k0 + cnt - 1, their inputs in islots, their outputs in oslots), verdict (frames[k].status: NXZ_FRAME_OK
 * for a good segment -- what nxz_launch_bgzf_gather looks at) */
int nxz_launch_checkpoint_index(int fmt, const nxz_batch_job_t *jobs, size_t n, uint64_t span, uint32_t cp_cap, uint64_t *cbit, uint64_t *uoff,
				uint8_t *windows, nxz_checkpoint_stream_t *streams, const uint32_t *order, hipStream_t stream);
int nxz_launch_checkpoint_check(uint64_t src_len, const uint64_t *cbit, const uint64_t *uoff, uint64_t L, uint8_t *ws, hipStream_t stream);
int nxz_launch_checkpoint_inmax(const uint64_t *cbit, const uint64_t *uoff, uint64_t n, uint64_t L, uint8_t *ws, hipStream_t stream);
int nxz_launch_checkpoint_stage(const uint8_t *src, const uint64_t *cbit, const uint64_t *uoff, const uint8_t *windows, uint64_t n, uint64_t L,
				uint8_t *ws, uint64_t k0, uint64_t cnt, uint8_t *islots, uint64_t istride, uint8_t *oslots, uint64_t ostride,
				nxz_batch_job_t *jobs, hipStream_t stream);
int nxz_launch_checkpoint_verdict(const uint64_t *uoff, uint64_t n, uint64_t L, uint8_t *ws, uint64_t k0, uint64_t cnt,
				  const nxz_batch_result_t *results, nxz_batch_frame_t *frames, hipStream_t stream);
/* (the windows' launch alone, for an index of another kind) */
int nxz_launch_checkpoint_windows(const nxz_batch_job_t *jobs, size_t n, uint32_t cp_cap, const uint64_t *uoff, const nxz_checkpoint_stream_t *streams,
				  uint8_t *windows, hipStream_t stream);
/* nxz_checkpoint_fine.hip: checkpoints inside blocks (nxz_checkpoint_fine.h has the rules).  The index with a state entry beside
 * cbit / uoff, the windows by nxz_launch_checkpoint_windows.  Of the range read's steps two are its own: check (ws[0]: index or a
 * state entry faulty) and, behind nxz_launch_checkpoint_stage on the same chunk, jobs (dht[k - k0]: the segment's table for
 * nxz_batch_decompress's dht_io; the jobs' resume and NXZ_JOB_SUSPEND_WHEN_FULL) */
int nxz_launch_checkpoint_index_fine(int fmt, const nxz_batch_job_t *jobs, size_t n, uint64_t span, uint32_t cp_cap, uint64_t *cbit, uint64_t *uoff,
				     nxz_checkpoint_state_t *state, uint8_t *windows, nxz_checkpoint_stream_t *streams, const uint32_t *order,
				     hipStream_t stream);
int nxz_launch_checkpoint_check_fine(uint64_t src_len, const uint64_t *cbit, const uint64_t *uoff, const nxz_checkpoint_state_t *state, uint64_t L,
				     uint8_t *ws, hipStream_t stream);
int nxz_launch_checkpoint_jobs_fine(const uint8_t *src, const uint64_t *cbit, const nxz_checkpoint_state_t *state, uint64_t n, uint64_t L, uint8_t *ws,
				    uint64_t k0, uint64_t cnt, nxz_batch_job_t *jobs, nxz_batch_dht_t *dht, hipStream_t stream);
/* nxz_checkpoint_build.hip: the index with its windows from the source alone (nxz_checkpoint_build.h has the ring's rules): the
 * walk of the two index kernels with a 32 KiB ring of the output in LDS, dumped to a checkpoint's slot where one is stored.
 * state NULL: checkpoints at block headers only */
int nxz_launch_checkpoint_build(int fmt, const nxz_batch_job_t *jobs, size_t n, uint64_t span, uint32_t cp_cap, uint64_t *cbit, uint64_t *uoff,
				nxz_checkpoint_state_t *state, uint8_t *windows, nxz_checkpoint_stream_t *streams, const uint32_t *order,
				hipStream_t stream);
/* nxz_checkpoint_batch.hip: ranges over all the rows of a batch's index (nxz_checkpoint_batch.h has the rules).  The batch is ONE
 * index of n_jobs * (cp_cap + 1) entries with a uoff of its own in bws (nxz_checkpoint_batch_workspace bytes; _uoff: where), which
 * the map, gather, inmax and verdict launches above take as it is.  map: the rows' verdicts, the bases, the flat uoff, the ranges
 * onto it, nxz_launch_range_map_ranges, the statuses of ranges without a row, nxz_launch_checkpoint_inmax; stage:
 * nxz_launch_checkpoint_stage and, with state, nxz_launch_checkpoint_jobs_fine, the source and the window by the segment's row */
size_t nxz_checkpoint_batch_workspace(uint64_t n_jobs, uint32_t cp_cap, uint64_t n);
const uint64_t *nxz_checkpoint_batch_uoff(uint8_t *bws, uint64_t n_jobs, uint32_t cp_cap, uint64_t n);
int nxz_launch_checkpoint_batch_map(const nxz_batch_job_t *jobs, uint64_t n_jobs, uint32_t cp_cap, const uint64_t *cbit, const uint64_t *uoff,
				    const nxz_checkpoint_state_t *state, const nxz_checkpoint_stream_t *streams, const nxz_batch_range_t *ranges,
				    uint64_t n, uint64_t *offsets, uint32_t *status, uint8_t *bws, uint8_t *ws, hipStream_t stream);
int nxz_launch_checkpoint_batch_stage(const nxz_batch_job_t *in, uint64_t n_jobs, uint32_t cp_cap, const uint64_t *cbit, const uint64_t *uoff,
				      const nxz_checkpoint_state_t *state, const uint8_t *windows, const nxz_checkpoint_stream_t *streams,
				      uint64_t n, uint8_t *bws, uint8_t *ws, uint64_t k0, uint64_t cnt, uint8_t *islots, uint64_t istride,
				      uint8_t *oslots, uint64_t ostride, nxz_batch_job_t *jobs, nxz_batch_dht_t *dht, hipStream_t stream);
/* nxz_streams.hip: a stream per device buffer (nxz_batch_deflate_streams; nxz_streams.h has the rules).  desc: the caller's jobs;
 * first[n + 1]: the streams' block prefix; a chunk is the blocks [b0, b0 + m) of the batch: jobs, results, owner (the block's stream)
 * and offsets (where it goes in its stream) are indexed from b0; state: what a stream carries from chunk to chunk */
typedef struct nxz_stream_state { uint64_t written, len_done; uint32_t crc, adler, stored, cc; } nxz_stream_state_t;
int nxz_launch_streams_prologue(const nxz_stream_job_t *desc, uint32_t n, uint32_t hist_max, int fmt, int level,
				nxz_stream_state_t *state, hipStream_t stream);
int nxz_launch_streams_expand(const nxz_stream_job_t *desc, const uint32_t *first, uint32_t n, uint32_t b0, uint32_t m,
			      uint32_t hist_max, uint8_t *slots, nxz_batch_job_t *jobs, uint32_t *owner, hipStream_t stream);
int nxz_launch_streams_layout(const uint32_t *first, uint32_t i_lo, uint32_t streams, uint32_t b0, uint32_t m,
			      const nxz_batch_job_t *jobs, const nxz_batch_result_t *results, uint32_t hist_max, uint32_t op_block,
			      nxz_stream_state_t *state, uint64_t *offsets, hipStream_t stream);
int nxz_launch_streams_pack(const nxz_stream_job_t *desc, const uint32_t *first, const uint32_t *owner, uint32_t b0, uint32_t m,
			    const nxz_batch_job_t *jobs, const nxz_batch_result_t *results, const uint64_t *offsets, hipStream_t stream);
int nxz_launch_streams_epilogue(const nxz_stream_job_t *desc, const uint32_t *first, uint32_t n, uint32_t hist_max, int fmt,
				const nxz_stream_state_t *state, nxz_stream_result_t *results, hipStream_t stream);
/* nxz_streams_dict.hip: the same with a shared dictionary as the window of every stream's first block (nxz_batch_deflate_streams_dict;
 * nxz_streams_dict.h has the rules).  nz[n + 1]: the streams with blocks in front of each stream; nz_b0 / nf: the first blocks of
 * streams in front of / inside the chunk; ljobs and lresults: the chunk in launch order (its nf first blocks, then the rest), pos[t]:
 * block t's place there */
int nxz_launch_streams_dict_prologue(const nxz_stream_job_t *desc, uint32_t n, uint32_t hist_max, int fmt, int level, uint32_t dictid,
				     nxz_stream_state_t *state, hipStream_t stream);
int nxz_launch_streams_dict_expand(const nxz_stream_job_t *desc, const uint32_t *first, const uint32_t *nz, uint32_t n, uint32_t b0,
				   uint32_t m, uint32_t hist_max, uint32_t h0, uint32_t nz_b0, uint32_t nf, uint8_t *slots,
				   nxz_batch_job_t *jobs, nxz_batch_job_t *ljobs, uint32_t *owner, uint32_t *pos, hipStream_t stream);
int nxz_launch_streams_dict_gather(const nxz_batch_result_t *lresults, const uint32_t *pos, uint32_t m, nxz_batch_result_t *results,
				   hipStream_t stream);
int nxz_launch_streams_dict_epilogue(const nxz_stream_job_t *desc, const uint32_t *first, uint32_t n, uint32_t hist_max, int fmt,
				     const nxz_stream_state_t *state, nxz_stream_result_t *results, hipStream_t stream);
/* nxz_streams_index.hip: the checkpoint index of the streams as a by-product of their layout (nxz_batch_deflate_streams_indexed;
 * nxz_streams_index.h has the rules).  Each launch goes behind its namesake above; ist: the index's own per-stream state (c: the uoff
 * of the last checkpoint, count: checkpoints so far, end_bit: the sentinel's bit, on: 0 for a stream that gets no index); marks: two
 * words a block of the chunk -- the window slot of each of its headers, or NXZ_SI_NONE (NULL: no windows wanted) */
typedef struct nxz_stream_index_state { uint64_t c, end_bit; uint32_t count, on; } nxz_stream_index_state_t;
int nxz_launch_streams_index_prologue(const nxz_stream_job_t *desc, uint32_t n, int fmt, const nxz_stream_state_t *state, uint32_t cp_cap,
				      uint64_t *cbit, uint64_t *uoff, nxz_stream_index_state_t *ist, hipStream_t stream);
int nxz_launch_streams_index_sweep(const uint32_t *first, uint32_t i_lo, uint32_t streams, uint32_t b0, uint32_t m,
				   const nxz_batch_job_t *jobs, const nxz_batch_result_t *results, const uint64_t *offsets,
				   uint32_t hist_max, uint64_t span, uint32_t cp_cap, uint64_t *cbit, uint64_t *uoff,
				   nxz_stream_index_state_t *ist, uint32_t *marks, hipStream_t stream);
int nxz_launch_streams_index_windows(const nxz_stream_job_t *desc, const uint32_t *owner, uint32_t m, const uint32_t *marks,
				     uint32_t cp_cap, const uint64_t *uoff, uint8_t *windows, hipStream_t stream);
int nxz_launch_streams_index_epilogue(const nxz_stream_job_t *desc, uint32_t n, int fmt, const nxz_stream_result_t *results,
				      const nxz_stream_index_state_t *ist, uint32_t cp_cap, uint64_t *cbit, uint64_t *uoff,
				      nxz_checkpoint_stream_t *streams, nxz_batch_job_t *index_jobs, hipStream_t stream);
/* nxz_streams_part.hip: a stream written in parts, a device buffer a part (nxz_batch_deflate_streams_part; nxz_streams_part.h has the
 * rules).  The plain call's launches with the part's descriptors and the streams' carry records, and the staging of first blocks whose
 * window does not lie in front of them in memory: sg[n + 1]: the staged parts in front of each stream; sg_b0: the staged first blocks
 * in front of the chunk; stage: 65 536 bytes a staged block of the chunk; staged[q]: the chunk's q-th staged block (indexed from b0) */
int nxz_launch_streams_part_prologue(const nxz_stream_part_job_t *desc, uint32_t n, uint32_t hist_max, int fmt, int level,
				     const nxz_stream_carry_t *carry, nxz_stream_state_t *state, hipStream_t stream);
int nxz_launch_streams_part_expand(const nxz_stream_part_job_t *desc, const uint32_t *first, const uint32_t *sg, uint32_t n, uint32_t b0,
				   uint32_t m, uint32_t hist_max, uint32_t sg_b0, uint8_t *slots, uint8_t *stage, nxz_batch_job_t *jobs,
				   uint32_t *owner, uint32_t *staged, hipStream_t stream);
int nxz_launch_streams_part_stage(const nxz_stream_part_job_t *desc, const uint32_t *owner, const uint32_t *staged, uint32_t ns,
				  const nxz_batch_job_t *jobs, hipStream_t stream);
int nxz_launch_streams_part_layout(const nxz_stream_part_job_t *desc, const uint32_t *first, uint32_t i_lo, uint32_t streams, uint32_t b0,
				   uint32_t m, const nxz_batch_job_t *jobs, const nxz_batch_result_t *results, uint32_t hist_max,
				   uint32_t op_block, nxz_stream_state_t *state, uint64_t *offsets, hipStream_t stream);
int nxz_launch_streams_part_pack(const nxz_stream_part_job_t *desc, const uint32_t *first, const uint32_t *owner, uint32_t b0, uint32_t m,
				 const nxz_batch_job_t *jobs, const nxz_batch_result_t *results, const uint64_t *offsets,
				 const nxz_stream_state_t *state, hipStream_t stream);
int nxz_launch_streams_part_epilogue(const nxz_stream_part_job_t *desc, const uint32_t *first, uint32_t n, uint32_t hist_max, int fmt,
				     const nxz_stream_state_t *state, nxz_stream_carry_t *carry, nxz_stream_result_t *results, hipStream_t stream);
/* nxz_inflate_part.hip: a stream read in parts, a device buffer a part (nxz_batch_inflate_streams_part; nxz_inflate_part.h has the rules).
 * The kernels around the raw decode of a chunk of m streams: desc, carry and results are the chunk's; off[m + 1]: where each stream's
 * slot begins in `stage`; work: what open tells stage and close about a stream (the offset of the deflate data's first byte in the
 * part, whether it goes through the decode, whether it is staged); jobs, dres and dht: the raw batch's jobs, results and dht_io */
typedef struct nxz_inflate_part_work { uint32_t body, live, staged, reserved; } nxz_inflate_part_work_t;
int nxz_launch_inflate_part_open(const nxz_inflate_part_job_t *desc, uint32_t m, int fmt, nxz_inflate_carry_t *carry, const uint64_t *off,
				 uint8_t *stage, nxz_batch_job_t *jobs, nxz_batch_dht_t *dht, nxz_inflate_part_work_t *work,
				 nxz_inflate_part_result_t *results, hipStream_t stream);
int nxz_launch_inflate_part_stage(const nxz_inflate_part_job_t *desc, const nxz_inflate_carry_t *carry, const uint64_t *off, uint32_t m,
				  uint64_t bytes, const nxz_inflate_part_work_t *work, const nxz_batch_job_t *jobs, hipStream_t stream);
int nxz_launch_inflate_part_close(const nxz_inflate_part_job_t *desc, uint32_t m, nxz_inflate_carry_t *carry, const nxz_batch_job_t *jobs,
				  const nxz_batch_result_t *dres, const nxz_batch_dht_t *dht, const nxz_inflate_part_work_t *work,
				  nxz_inflate_part_result_t *results, hipStream_t stream);
/* nxz_shuffle.hip: the byte-shuffle filter (nxz_batch_shuffle / nxz_batch_unshuffle; nxz_shuffle.h has the rules).  plan[n], first[n + 1]
 * and st[n] are the host's one pass (nxz_shuffle_plan_batch) in device memory, tiles = first[n]: st goes to status, one grid takes the tiles */
struct nxz_shuffle_plan;
int nxz_launch_shuffle(const struct nxz_shuffle_plan *plan, const uint32_t *first, const uint32_t *st, uint32_t n, uint32_t tiles, int undo,
		       uint32_t *status, hipStream_t stream);
int nxz_inflate_wg_reasons(const uint8_t *wg_ws, uint32_t *out16);
int nxz_inflate_wg_prof(const uint8_t *wg_ws, unsigned long long *out12);
}

// exclusive prefix sum across one workgroup of 1024 threads (part: 1024 entries of LDS); returns the thread's start, *total
__device__ inline uint64_t nxz_block_excl(uint64_t v, uint64_t *part, uint64_t *total)
{
	const uint32_t t = threadIdx.x;
	__syncthreads();
	part[t] = v;
	__syncthreads();
	for (uint32_t d = 1; d < 1024; d <<= 1) {
		const uint64_t u = t >= d ? part[t - d] : 0;
		__syncthreads();
		part[t] += u;
		__syncthreads();
	}
	*total = part[1023];
	return part[t] - v;
}
#endif
#endif
