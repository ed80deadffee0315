/*
 * nxz_engine.h -- C ABI of the MI355X DEFLATE engine (libnxz_engine.so).
 *
 * This is the drop-in boundary of the hot path.  In libnxz/power-gzip the
 * per-byte work (LZ77, Huffman encode/decode, CRC32/Adler32) is done by the
 * POWER NX accelerator; the library talks to it through exactly six symbols
 * (everything in the reference's lib/ links with only these undefined:
 * SURVEY.md 8(b)).  This library provides those six symbols on top of HIP
 * kernels for gfx950, plus an additive batched interface for device-resident
 * buffers.
 *
 * Reference interfaces replaced (paths relative to the libnxz tree):
 *   nx_function_begin   lib/gzip_vas.c:144   (decl lib/nx_zlib.h:626)
 *   nx_function_end     lib/gzip_vas.c:166   (decl lib/nx_zlib.h:627)
 *   nxu_run_job         lib/gzip_vas.c:281   (decl lib/nx_zlib.h:629), called
 *                       only from nx_submit_job lib/nx_zlib.c:493
 *   nx_wait_ticks       lib/gzip_vas.c:203
 *   tb_freq             lib/gzip_vas.c:92    (read by nx_get_freq inc_nx/nxu.h:81-88)
 *   __crc32_vpmsum      lib/crc32_power.c    (called from lib/crc32_ppc.c:55)
 * Wire format of a job (CRB + CPB + CSB + DDE), function codes and completion
 * codes: inc_nx/nxu.h:155-202, 286-616, 803-857.  The structures below are
 * declared from the byte layout (all multi-byte fields BIG-ENDIAN); their
 * offsets are checked against the reference header in tests/test_abi.py.
 *
 * No torch / HIP types appear in any signature: plain pointers and sizes.
 */
#ifndef NXZ_ENGINE_H
#define NXZ_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------
 * Job wire format (nx_gzip_crb_cpb_t compatible, 2048 bytes, 2048-aligned)
 * ---------------------------------------------------------------------- */

/* Data descriptor element, 16 bytes (inc_nx/nxu.h:155-170).
 *   count == 0 : direct   -- addr = buffer, bytes = length
 *   count  > 0 : indirect -- addr = array of `count` direct DDEs, bytes =
 *                total; at most `bytes` bytes are processed even when the
 *                list is longer (lib/nx_deflate.c:810-813). */
typedef struct nxz_dde {
	uint32_t count_be;   /* dde_count = (be32toh(count_be) >> 8) & 0xff */
	uint32_t bytes_be;   /* ddebc */
	uint64_t addr_be;    /* ddead: host virtual address */
} __attribute__((aligned(16))) nxz_dde_t;

/* Coprocessor status block, 16 bytes (inc_nx/nxu.h:172-202).  With
 * w = be32toh(flags_be): V = w >> 31, CC = (w >> 8) & 0xff, CE = w & 0xff
 * (the three CE flags live in the top 3 bits of that byte). */
typedef struct nxz_csb {
	uint32_t flags_be;
	uint32_t tpbc_be;    /* target processed byte count */
	uint64_t fsaddr_be;
} __attribute__((aligned(16))) nxz_csb_t;

/* Request block, 256 bytes incl. the CSB at +240 (inc_nx/nxu.h:552-609). */
typedef struct nxz_crb {
	uint32_t fc_be;              /* +0   function code = be32toh(fc_be) & 0xff */
	uint32_t reserved1;          /* +4 */
	uint64_t csb_address_be;     /* +8 */
	nxz_dde_t source;            /* +16 */
	nxz_dde_t target;            /* +32 */
	uint8_t  ccb[16];            /* +48 */
	uint8_t  reserved64[176];    /* +64 */
	volatile nxz_csb_t csb;      /* +240 */
} __attribute__((aligned(128))) nxz_crb_t;

#define NXZ_LLSZ       286
#define NXZ_DSZ        30
#define NXZ_DHT_MAXSZ  288     /* bytes of DHT bit string in the CPB */

/* Parameter block, 1680 bytes (inc_nx/nxu.h:286-542). */
typedef struct nxz_cpb {
	/* ---- input region ---- */
	uint32_t in_adler_be;        /* +0   big-endian Adler-32 to continue from */
	uint32_t in_crc_le;          /* +4   CRC-32 to continue from; memory order == gzip trailer order
				      *       (little-endian), see lib/nx_deflate.c:436-449 */
	uint32_t in_w2_be;           /* +8   w=be32toh: in_histlen = w >> 20 (16-byte units); in_subc = w & 7 */
	uint32_t in_w3_be;           /* +12  w=be32toh: in_sfbt = (w >> 16) & 15; in_rembytecnt = w & 0xffff;
				      *       in_dhtlen = w & 0xfff (bits) */
	uint8_t  in_dht[NXZ_DHT_MAXSZ];  /* +16 */
	uint8_t  reserved_in[80];    /* +304 */
	/* ---- output region ---- */
	uint32_t out_adler_be;       /* +384 */
	uint32_t out_crc_le;         /* +388 memory order == gzip trailer order (little-endian) */
	uint32_t out_w2_be;          /* +392 w=be32toh: out_tebc = (w >> 16) & 7; out_subc = w & 0xffff */
	uint32_t out_w3_be;          /* +396 w=be32toh: out_sfbt = (w >> 16) & 15; out_rembytecnt = w & 0xffff;
				      *       out_dhtlen = w & 0xfff */
	union {                      /* +400 */
		uint32_t out_spbc_be;            /* compress w/o counts, wrap */
		uint32_t out_lzcount_be[NXZ_LLSZ + NXZ_DSZ];
		struct {
			uint8_t  out_dht[NXZ_DHT_MAXSZ];
			uint32_t out_spbc_decomp_be;     /* +688 */
		} d;
		uint8_t  qw25[79 * 16];
	} u;
	uint32_t out_spbc_with_count_be; /* +1664 */
	uint8_t  pad[12];
} __attribute__((aligned(128))) nxz_cpb_t;

typedef struct nxz_crb_cpb {
	nxz_crb_t crb;
	nxz_cpb_t cpb;
} __attribute__((aligned(2048))) nxz_crb_cpb_t;

/* Function codes (inc_nx/nxu.h:803-816).  Bit 0x08 = resume (history prefix
 * allowed), bit 0x04 = also return LZ symbol counts, bit 0x02 = dynamic table. */
enum {
	NXZ_FC_COMPRESS_FHT               = 0x00,
	NXZ_FC_COMPRESS_DHT               = 0x02,
	NXZ_FC_COMPRESS_FHT_COUNT         = 0x04,
	NXZ_FC_COMPRESS_DHT_COUNT         = 0x06,
	NXZ_FC_COMPRESS_RESUME_FHT        = 0x08,
	NXZ_FC_COMPRESS_RESUME_DHT        = 0x0a,
	NXZ_FC_COMPRESS_RESUME_FHT_COUNT  = 0x0c,
	NXZ_FC_COMPRESS_RESUME_DHT_COUNT  = 0x0e,
	NXZ_FC_DECOMPRESS                 = 0x10,
	NXZ_FC_DECOMPRESS_SINGLE_BLK      = 0x12,
	NXZ_FC_DECOMPRESS_RESUME          = 0x14,
	NXZ_FC_DECOMPRESS_RESUME_SINGLE_BLK = 0x16,
	NXZ_FC_WRAP                       = 0x1e,
	/* Additive (not in the reference): bit 0x20 on a DHT compress code = the engine generates the
	 * table itself, from the LZ symbol counts of this very job, exactly as the reference's dhtgen()
	 * would (lib/nx_dhtgen.c:945-1034; EOB counted once, unused symbols get no code), and encodes
	 * the job with it.  in_dht / dht[] are ignored. */
	NXZ_FC_COMPRESS_DHTGEN              = 0x22,
	NXZ_FC_COMPRESS_DHTGEN_COUNT        = 0x26,
	NXZ_FC_COMPRESS_RESUME_DHTGEN       = 0x2a,
	NXZ_FC_COMPRESS_RESUME_DHTGEN_COUNT = 0x2e
};

/* Completion codes written to CSB.CC (inc_nx/nxu.h:823-857). */
enum {
	NXZ_CC_OK            = 0,
	NXZ_CC_DATA_LENGTH   = 3,    /* with CE partial bit: normal "source ran out / trailer follows" */
	NXZ_CC_INVALID_OP    = 8,
	NXZ_CC_TARGET_SPACE  = 13,
	NXZ_CC_INVALID_CRB   = 21,
	NXZ_CC_TPBC_GT_SPBC  = 64,
	NXZ_CC_MISSING_CODE  = 66,
	NXZ_CC_INVALID_DIST  = 67,
	NXZ_CC_INVALID_DHT   = 68,
	NXZ_CC_NO_HW         = 254
};
/* CE bits as stored in the 3 most significant bits of the CE byte (inc_nx/nxu.h:762-781) */
#define NXZ_CE_PARTIAL     0x4
#define NXZ_CE_TERMINATE   0x2
#define NXZ_CE_TPBC_VALID  0x1

/* ------------------------------------------------------------------------
 * The six symbols of the reference's device transport
 * ---------------------------------------------------------------------- */

/* Device handle.  Layout-compatible prefix of the reference's struct
 * nx_dev_t (lib/nx_zlib.h:178-194): only paste_addr, fd and function are
 * touched by the transport (lib/gzip_vas.c:94-185); the library allocates
 * the struct and owns every other field. */
typedef struct nxz_dev {
	int   lib_private[8];  /* lock .. creator_pid: owned by the calling library */
	void *paste_addr;      /* +32 engine context (opaque) */
	int   fd;              /* +40 HIP device ordinal + 1 */
	int   function;        /* +44 */
} nxz_dev_t;

#define NXZ_FUNC_COMP_GZIP 2   /* lib/nx_zlib.h: NX_FUNC_COMP_GZIP */

/* Open the engine on HIP device `pri` (-1 = current / $NXZ_DEVICE).
 * 0 on success, -1 with errno set (ENODEV when no gfx950 device or the HIP
 * code object failed to load: there is NO CPU fallback). */
int nx_function_begin(int function, int pri, void *handle);
int nx_function_end(void *handle);

/* Run one job synchronously.  Source/target are HOST virtual addresses in
 * the DDEs; the engine stages them through pinned buffers, runs the kernels
 * on its stream, writes target, the CPB output region and the CSB (V=1).
 * Returns 0 when the job retired (result in csb.cc), -EAGAIN on timeout. */
int nxu_run_job(nxz_crb_cpb_t *job, void *handle);

/* Back-off helper of the retry ladders: sleeps/spins for `ticks` timebase
 * ticks and returns the accumulated wait. */
uint64_t nx_wait_ticks(uint64_t ticks, uint64_t accumulated_ticks, int do_sleep);

/* Timebase frequency in Hz (512 MHz, the POWER timebase the library's delay
 * thresholds are written for). */
extern uint64_t tb_freq;

/* CRC-32 used by the library's exported crc32() (lib/crc32_ppc.c:55 passes
 * the pre-inverted crc; this returns the raw register like the vpmsum code). */
unsigned int __crc32_vpmsum(unsigned int crc, const unsigned char *p, unsigned long len);

/* ------------------------------------------------------------------------
 * Additive batched interface (device-resident buffers).  Names are outside
 * the nx_* / zlib namespaces of lib/Versions.
 * ---------------------------------------------------------------------- */

typedef struct nxz_ctx nxz_ctx_t;

/* One job of a batch.  All pointers are DEVICE pointers; src/dst must be
 * 16-byte aligned.  For compress jobs `hist_len` bytes at src are history
 * (multiple of 16, <= 32768; lib/nx_deflate.c:853-855). */
typedef struct nxz_batch_job {
	const uint8_t *src;       /* [history][source] */
	uint8_t       *dst;
	uint32_t       src_len;   /* bytes at src including history */
	uint32_t       hist_len;
	uint32_t       dst_cap;
	uint32_t       in_crc;    /* running checksums to continue from */
	uint32_t       in_adler;
	uint32_t       dht_index; /* DHT jobs: which table of the batch's dht array */
	uint32_t       resume;    /* decompress resume state: in_rembytecnt | in_sfbt << 16 | in_subc << 20
				   * (0 = start at a block header on a byte boundary, FC 0x10) */
	uint32_t       reserved;  /* flags, additive: NXZ_JOB_SUSPEND_WHEN_FULL, NXZ_JOB_NO_DICT */
} nxz_batch_job_t;

/* Decompress jobs (additive; the reference's engine has no such thing and its library runs a job
 * that overflowed again with a quarter of the source, lib/nx_inflate.c:1399-1424): a full target is
 * not an error (CC 13) but a place to suspend, like the end of the source -- CC 3 with the resume state
 * in front of the token that did not fit, spbc = the source bytes used so far, subc = the unused
 * bits of the last of them.  nxu_run_job takes the flag from bit 0 of crb.reserved1 (big-endian 1).
 * Honoured by the stream-per-wave kernels (nxu_run_job, batches below NXZ_INFLATE_LANES_MIN streams);
 * the stream-per-lane kernel reports CC 13 as ever. */
#define NXZ_JOB_SUSPEND_WHEN_FULL 1u

/* Per-job result, written by the device (device memory, 32 bytes). */
typedef struct nxz_batch_result {
	uint32_t cc;          /* completion code (NXZ_CC_*) */
	uint32_t tpbc;        /* bytes written to dst (incl. the partial last byte) */
	uint32_t tebc;        /* compress: valid bits in the last byte, 0 == 8;
			       * decompress: out_rembytecnt when suspended inside a stored block */
	uint32_t spbc;        /* source bytes processed incl. history */
	uint32_t crc;         /* crc32 continued from in_crc */
	uint32_t adler;
	uint32_t subc;        /* decompress: unprocessed source bits */
	uint32_t sfbt;        /* decompress: bits 0..3 source final block type (inc_nx/nxu.h:466-511),
			       * bit 8 = final EOB seen, bits 16..27 = out_dhtlen when suspended
			       * inside a dynamic block (table bits are in the job's dht_io slot) */
} nxz_batch_result_t;

/* DHT table slot for batched dynamic-Huffman jobs (device memory). */
typedef struct nxz_batch_dht {
	uint32_t dhtlen;                 /* bits */
	uint8_t  dht[NXZ_DHT_MAXSZ + 4]; /* RFC1951 3.2.7 bit string, HLIT first */
} nxz_batch_dht_t;

/* Create / destroy an engine context on a HIP device.  In the batch calls
 * `stream` is a hipStream_t passed as void* (NULL = the HIP default stream). */
nxz_ctx_t *nxz_ctx_create(int device);
void       nxz_ctx_destroy(nxz_ctx_t *ctx);
const char *nxz_last_error(void);

/* Batched compress: jobs[n], results[n] (and dht[], counts[]) are DEVICE
 * arrays.  fc is one of the NXZ_FC_COMPRESS_* codes and applies to every job.
 * dht[ntables] (DHT function codes only; not the DHTGEN codes, where the engine makes a table
 * per job) are the tables jobs[].dht_index refers to.  counts (may be NULL unless fc has the COUNT bit): n x 316 uint32
 * (host byte order), LL then D, EOB counted once.
 * Asynchronous on `stream`; returns 0 or a negative errno. */
int nxz_batch_compress(nxz_ctx_t *ctx, int fc,
		       const nxz_batch_job_t *jobs, size_t n,
		       const nxz_batch_dht_t *dht, size_t ntables,
		       nxz_batch_result_t *results, uint32_t *counts,
		       void *stream);

/* The reference's dhtgen() (lib/nx_dhtgen.c:945-1034) on the device: counts[n][316] (286
 * literal/length + 30 distance counts, host byte order, as the COUNT function codes return them;
 * they are taken as they are -- raise zero counts first if the table is to serve other data,
 * lib/nx_dhtgen.c:235) -> tables[n].  Bit for bit what nxz_dhtgen() / the reference produce.
 * Asynchronous on `stream`. */
int nxz_batch_dhtgen(nxz_ctx_t *ctx, const uint32_t *counts, size_t n, nxz_batch_dht_t *tables, void *stream);

/* Batched decompress of raw-deflate streams (FC 0x10, or 0x14 when
 * jobs[].resume / hist_len are set): each job inflates until final EOB, end
 * of source or full target (CC 13); result.sfbt/subc report where it
 * stopped.  dht_io (NULL or n slots): in = table to resume inside a dynamic
 * block, out = table in force when the job suspended inside one.  A job that
 * resumes inside a dynamic block ((in_sfbt & 0xe) == 0xc) in a batch without
 * dht_io brings no table: cc = NXZ_CC_INVALID_DHT, tpbc = 0, nothing written,
 * as for a slot whose table does not parse or is not dhtlen bits long. */
int nxz_batch_decompress(nxz_ctx_t *ctx,
			 const nxz_batch_job_t *jobs, size_t n,
			 nxz_batch_result_t *results,
			 nxz_batch_dht_t *dht_io, void *stream);

/* ONE long raw-deflate stream, decoded in parallel by block-boundary speculation (additive; the
 * reference inflates a stream job after job, lib/nx_inflate.c:1060-1762).  src (DEVICE, src_len
 * bytes) holds the stream from bit first_bit on and must reach its final block; hist (DEVICE or
 * NULL): up to 32 KiB that precede the output (dictionary / earlier output); dst (DEVICE).
 * Synchronous.  Returns 0: *out_len bytes at dst, *crc / *adler of exactly those bytes (combine
 * them with yours), *end_bit = first bit behind the final block, *pieces / *rounds for the curious.
 * -ENOTSUP: the stream does not lend itself to it (shorter than 12 KiB, hardly any dynamic blocks, no
 * final block inside src, ...): use nxz_batch_decompress / nxu_run_job's resume loop.  -E2BIG:
 * dst_cap too small (*out_len = bytes needed).  -EILSEQ: not a deflate stream. */
int nxz_inflate_stream(nxz_ctx_t *ctx, const uint8_t *src, uint64_t src_len, uint64_t first_bit,
		       const uint8_t *hist, uint32_t hist_len, uint8_t *dst, uint64_t dst_cap,
		       uint64_t *out_len, uint32_t *crc, uint32_t *adler, uint64_t *end_bit,
		       uint32_t *pieces, uint32_t *rounds, void *stream);

/* The same for a PART of a stream -- what a caller of inflate() holds at one time (additive).  *state
 * in: where the stream stands at first_bit -- all zero at a block header (or the stream's start), else
 * the fields a suspended decompress job reported (out_sfbt with bit 3 set, out_rembytecnt, out_dhtlen /
 * out_dht; first_bit = 8 - in_subc of the partly used first byte); out: the same for *end_bit, which
 * is the end of src unless state->final (the final block ended at *end_bit) or the output of the
 * pieces further on did not fit dst_cap (then *end_bit is a block header before the end of src, state
 * all zero).  -E2BIG only when not even the first piece fits.  Everything else as above. */
typedef struct nxz_stream_resume {
	uint32_t sfbt;                 /* 0, or 0x8 | BFINAL inside a stored block, 0xa | fixed, 0xc | dynamic, 0xe | in a header */
	uint32_t rem;                  /* stored: bytes of the block still to come */
	uint32_t dhtlen;               /* dynamic: bits of the table in dht */
	uint32_t final;                /* out: the final block ended at *end_bit */
	uint8_t  dht[NXZ_DHT_MAXSZ];
} nxz_stream_resume_t;
int nxz_inflate_stream_part(nxz_ctx_t *ctx, const uint8_t *src, uint64_t src_len, uint64_t first_bit,
			    const uint8_t *hist, uint32_t hist_len, uint8_t *dst, uint64_t dst_cap,
			    uint64_t *out_len, uint32_t *crc, uint32_t *adler, uint64_t *end_bit,
			    nxz_stream_resume_t *state, uint32_t *pieces, void *stream);

/* A long HOST buffer -> ONE raw deflate stream in a HOST buffer (additive; what nx_deflate makes of
 * it job after job, lib/nx_deflate.c:1440-1719, for the levels that carry no history from job to job,
 * :654-680).  The source is cut into 64 KiB blocks, compressed side by side (fc = NXZ_FC_COMPRESS_FHT,
 * or NXZ_FC_COMPRESS_DHTGEN: an exact dynamic table per block made on the device), and laid back to
 * back on the device the way the reference strings jobs together: a block that ends inside a byte is
 * followed by an empty stored block (append_sync_flush, :220-243), a block that did not shrink is
 * stored (:1274-1282); with `final` the last block carries BFINAL, otherwise the run ends on a byte
 * boundary and more blocks may follow.  Groups of 256 blocks alternate between two HIP streams, so
 * the host-to-device copy of one group, the kernels of another and the copy back overlap.
 * dst_cap >= nxz_deflate_host_bound(src_len).  *crc / *adler: checksums of the source from 0 / 1
 * (combine with yours).  Synchronous; returns 0 or a negative errno. */
size_t nxz_deflate_host_bound(size_t src_len);
int nxz_deflate_host(nxz_ctx_t *ctx, int fc, const uint8_t *src, size_t src_len, int final,
		     uint8_t *dst, size_t dst_cap, size_t *out_len, uint32_t *crc, uint32_t *adler);
/* The same for the levels that carry history from job to job (5..9: lib/nx_deflate.c:654-680 sets
 * max_history_len to 4..32 KiB; :845-862 puts that much of the earlier input in front of a job's
 * source): every block's window is the hist_max bytes of the INPUT in front of it -- known up
 * front, so the blocks are still compressed side by side --, the first block's the tail of `prev`
 * (prev_len bytes the caller kept of earlier calls; may be NULL).  Blocks are 64 KiB - hist_max long
 * (window + block <= 64 KiB; hist_max is rounded down to a multiple of 16, 32 KiB at most).
 * dst_cap >= nxz_deflate_host_bound_hist(src_len, hist_max). */
size_t nxz_deflate_host_bound_hist(size_t src_len, uint32_t hist_max);
int nxz_deflate_host_hist(nxz_ctx_t *ctx, int fc, const uint8_t *src, size_t src_len, int final, uint32_t hist_max,
			  const uint8_t *prev, size_t prev_len, uint8_t *dst, size_t dst_cap, size_t *out_len,
			  uint32_t *crc, uint32_t *adler);

/* Device memory the engine keeps between calls (workspaces of nxz_inflate_stream / _part: grown on demand,
 * a workspace above NXZ_PINFLATE_KEEP_MB -- default 8192 -- is given back when its call ends): nxz_trim()
 * gives back what no call is using right now and returns the bytes freed.  For processes that share the
 * device with other users (torch, another library). */
size_t nxz_trim(void);

/* The device a context is made on when the caller names none (nx_function_begin with pri = -1, i.e.
 * NX_GZIP_DEV_NUM unset: lib/nx_zlib.c:568-576 "nx_id -1 means open any", :1281-1287): NXZ_DEVICE if set;
 * else the calling thread's device -- the process' first thread gets the current HIP device, every further
 * thread the next visible device in turn (NXZ_DEVICE_POLICY=current: always the current device).  The
 * policy itself, a pure function: requested ordinal (-1 = any), visible devices, current device, index of the
 * calling thread in order of first use, spread on / off -> device, or -1 for "no such device". */
int nxz_pick_device(int requested, int ndev, int current, unsigned thread_index, int spread);

/* Batched wrap (FC 0x1e): copy + crc32 + adler32 from the initial values. */
int nxz_batch_wrap(nxz_ctx_t *ctx, const nxz_batch_job_t *jobs, size_t n,
		   nxz_batch_result_t *results, void *stream);

/* Gzip members (RFC 1952) from the results of a compress batch, written back to back into
 * `packed` (device): member i = 18-byte header carrying the "BC" extra subfield with the
 * member's own size - 1 (the BGZF layout: readers can find every member without inflating),
 * job i's output -- or, when the job failed or did not shrink (CC != 0 or tpbc >= length + 5), a
 * stored block of its source, the per-job fallback of lib/nx_deflate.c:1292-1400 --, CRC32 and
 * ISIZE.  A stored block holds 65 535 bytes at most: a source of 65 536 bytes falls back to two,
 * 65 535 bytes and the rest, 10 bytes of headers instead of 5.  jobs[].dst must be 16-byte
 * aligned as the compress batch requires; `packed` may have any alignment.  Source blocks of
 * at most 65 280 bytes keep every member within BGZF's 64 KiB; a larger member is valid gzip
 * but NOT a BGZF member -- its BSIZE holds the low 16 bits of size - 1.  offsets (device, n + 1
 * uint64): start of each member in `packed`; offsets[n] = total bytes.  `packed` needs
 * n * 26 + sum(max(tpbc, length + 5)) bytes at most, length + 10 in place of length + 5 for a
 * job of more than 65 535 source bytes.  Asynchronous on `stream`. */
int nxz_batch_pack_gzip(nxz_ctx_t *ctx, const nxz_batch_job_t *jobs, const nxz_batch_result_t *results,
			size_t n, uint64_t *offsets, uint8_t *packed, void *stream);

/* The zlib counterpart (RFC 1950): member i = CMF 0x78 and FLG with FLEVEL from `level` (0..9, -1 = 6, as
 * zlib's deflateInit), job i's output -- or the same stored-block fallback as above --, the Adler-32 of
 * results[i] big-endian.  offsets as above; `packed` needs n * 6 + sum(max(tpbc, length + 5)) bytes at most
 * (length + 10 for a job of more than 65 535 source bytes: two stored blocks).  Asynchronous on `stream`. */
int nxz_batch_pack_zlib(nxz_ctx_t *ctx, int level, const nxz_batch_job_t *jobs, const nxz_batch_result_t *results,
			size_t n, uint64_t *offsets, uint8_t *packed, void *stream);

/* ------------------------------------------------------------------------
 * Framed streams on the device: zlib (RFC 1950) and gzip (RFC 1952)
 * ---------------------------------------------------------------------- */
enum { NXZ_FMT_ZLIB = 1, NXZ_FMT_GZIP = 2, NXZ_FMT_AUTO = 3 };   /* AUTO: per job, gzip when it starts 1f 8b, else zlib */
enum {
	NXZ_FRAME_OK = 0,
	NXZ_FRAME_BAD_HEADER,    /* gzip ID1 ID2 / reserved FLG bits; zlib FCHECK / CINFO > 7; a job with resume or hist_len set */
	NXZ_FRAME_BAD_METHOD,    /* CM != 8 */
	NXZ_FRAME_NEED_DICT,     /* zlib FDICT and the call holds no dictionary of that DICTID (nxz_batch_decompress_framed: none at all): nothing is decoded (dictid is set) */
	NXZ_FRAME_BAD_HCRC,      /* gzip FHCRC does not match the header */
	NXZ_FRAME_TRUNCATED,     /* the source ends inside the header, the deflate data or the trailer */
	NXZ_FRAME_DEFLATE,       /* the deflate data failed: results[i].cc says why */
	NXZ_FRAME_BAD_CHECK,     /* Adler-32 / CRC-32 of the trailer differs from the output's */
	NXZ_FRAME_BAD_LENGTH     /* gzip ISIZE differs from the output's length mod 2^32 */
};
/* One per job, written by the device (device memory, 52 bytes).  Offsets count from the job's src; 0 = absent. */
typedef struct nxz_batch_frame {
	uint32_t status;         /* NXZ_FRAME_* */
	uint32_t format;         /* NXZ_FMT_ZLIB / NXZ_FMT_GZIP: what the job turned out to be */
	uint32_t hdr_len;        /* header bytes */
	uint32_t end;            /* bytes of src used: header + deflate + trailer (0 unless the trailer was read) */
	uint32_t check;          /* the trailer as read: Adler-32 or CRC-32 */
	uint32_t isize;          /* gzip ISIZE as read */
	uint32_t mtime;          /* gzip MTIME */
	uint32_t dictid;         /* zlib DICTID when FDICT is set */
	uint32_t extra_off, extra_len, name_off, comment_off;
	uint8_t  flg;            /* gzip FLG / zlib FLG */
	uint8_t  xfl, os;        /* gzip XFL, OS */
	uint8_t  cinfo;          /* zlib CINFO (CMF >> 4) */
} nxz_batch_frame_t;

/* Batched decompress of zlib / gzip streams: a header kernel parses every job's header and checks it, the
 * deflate data goes through nxz_batch_decompress (the same routes as raw streams), a trailer kernel checks
 * Adler-32 / CRC-32 and ISIZE.  jobs[], results[] and frames[] are DEVICE arrays; asynchronous on `stream`.
 * jobs[].src may have any alignment; jobs[].dst must be 16-byte aligned (as for raw streams, or the streams
 * take the slower route); resume and hist_len must be 0.  results[i] is what nxz_batch_decompress writes for
 * the job's deflate data alone -- except after a header failure, when it is all zero with cc =
 * NXZ_CC_INVALID_OP and dst is not touched.  Bytes after the trailer are no error: frames[i].end < src_len.
 * A second member inside one job is not decoded (`end` tells where it starts); nxz_batch_gzip_members_size / _decode below
 * decode every member of a job. */
int nxz_batch_decompress_framed(nxz_ctx_t *ctx, int fmt, const nxz_batch_job_t *jobs, size_t n,
				nxz_batch_result_t *results, nxz_batch_frame_t *frames, void *stream);

/* A BGZF image (gzip members with the "BC" extra subfield, as nxz_batch_pack_gzip / nxz_blocked_deflate /
 * bgzip write them) in DEVICE memory -> its plain bytes at dst (DEVICE).  The members are found on the device
 * in parallel (every position that looks like a member header is a candidate; the members are the chain of
 * candidates reachable from position 0), laid out by a prefix sum of their ISIZE -- offsets[j] (DEVICE,
 * max_members + 1) -- and decoded as one framed gzip batch: frames[j] / results[j] (DEVICE, max_members)
 * per member; a member that fails does not stop the others.  Members of 65 280 bytes of source keep every
 * offset 16-byte aligned; other sizes decode correctly on the slower route.
 * Synchronous.  Returns 0: *members, *out_len (sum of ISIZE), *consumed (the prefix of whole chained members,
 * as nxz_blocked_scan).  -EILSEQ: packed does not start with a member; -E2BIG: more members than max_members
 * (*members set) or dst_cap < sum of ISIZE (*out_len set). */
int nxz_batch_unpack_gzip(nxz_ctx_t *ctx, const uint8_t *packed, uint64_t len, uint8_t *dst, uint64_t dst_cap,
			  uint64_t *offsets, nxz_batch_frame_t *frames, nxz_batch_result_t *results,
			  size_t max_members, uint64_t *members, uint64_t *consumed, uint64_t *out_len, void *stream);

/* ------------------------------------------------------------------------
 * One preset dictionary for all jobs of a batch (zlib's deflateSetDictionary / inflateSetDictionary)
 * ---------------------------------------------------------------------- */
/* `len` HOST bytes (any length, 0 = no dictionary: the _dict calls then give what their plain counterparts give).  The object
 * owns a 16-byte aligned device copy; it is immutable and may be used by many streams and threads at once; destroy it when
 * no call that uses it is still running.  The rules (power-gzip_amd/csrc/nxz_dict.h):
 *   inflate window: the last min(len, 32768) bytes, what zlib's inflateSetDictionary keeps;
 *   deflate window: the last W = min(len, 32768) & ~15 bytes (the compress kernels' histories are multiples of 16; the up to
 *   15 leading bytes are never referred to).  A compress job carries at most 65536 - W bytes.
 * 0 or a negative errno. */
typedef struct nxz_dict nxz_dict_t;
int      nxz_dict_create(nxz_ctx_t *ctx, const uint8_t *bytes, size_t len, nxz_dict_t **out);
void     nxz_dict_destroy(nxz_ctx_t *ctx, nxz_dict_t *d);
uint32_t nxz_dict_id(const nxz_dict_t *d);       /* Adler-32 of all len bytes from 1: zlib's DICTID */

/* jobs[].reserved, honoured by the _dict calls only: this job sees no dictionary */
#define NXZ_JOB_NO_DICT 2u

/* nxz_batch_compress with the dictionary's deflate window as every job's history: jobs[i].src is the source alone, hist_len
 * must be 0.  dst, results[i] and counts are bit for bit what nxz_batch_compress gives for the job [deflate window][source]
 * with hist_len = W -- except spbc, which counts the source bytes only.  The streams inflate with
 * zlib's inflateSetDictionary(the whole dictionary), or nxz_batch_decompress_dict.  The window is read from the one device
 * copy (no staging per job).  A job with hist_len != 0 or W + src_len > 65536: cc = NXZ_CC_INVALID_OP, tpbc = 0, dst untouched.
 * Every fc of nxz_batch_compress (the RESUME bit is implied).  Asynchronous on `stream`. */
int nxz_batch_compress_dict(nxz_ctx_t *ctx, int fc, const nxz_dict_t *dict, const nxz_batch_job_t *jobs, size_t n,
			    const nxz_batch_dht_t *dht, size_t ntables, nxz_batch_result_t *results, uint32_t *counts, void *stream);

/* Raw deflate streams whose distances may reach into the dictionary's inflate window: output and results[i] are what
 * nxz_batch_decompress gives for the job [inflate window][stream] with hist_len = window, failures included (a distance in
 * front of the window: NXZ_CC_INVALID_DIST) -- except spbc, which counts the stream's bytes only.  resume and hist_len must be 0
 * (else NXZ_CC_INVALID_OP, dst untouched).  Streams of NXZ_DICT_WG_MIN (environment, default 4096) source bytes or more go a
 * workgroup each with the window preloaded into LDS; what that kernel hands back (errors, early ends, small targets, dst not
 * 16-byte aligned) and every smaller stream goes a wavefront each and reads the window from the device copy -- the choice is made
 * on the device, job by job.  nxz_ctx_wg_reasons reports on the workgroup launch.  Asynchronous on `stream`, no host wait.
 * Speed (profiles/r08_dict.txt): streams of less than about 4 KiB run at 0.9 - 1.0 x of what nxz_batch_decompress makes of jobs
 * staged as [window][stream] per job -- the call saves their memory, not time --, streams of 16 - 32 KiB of output 1.1 - 1.6 x.
 * A source that is not 16-byte aligned gets a quarter of the bound (it costs the wavefront kernel more). */
int nxz_batch_decompress_dict(nxz_ctx_t *ctx, const nxz_dict_t *dict, const nxz_batch_job_t *jobs, size_t n,
			      nxz_batch_result_t *results, void *stream);

/* nxz_batch_pack_zlib for streams made by nxz_batch_compress_dict: FDICT set, FCHECK to match, DICTID (4 bytes, big-endian)
 * behind FLG -- the header zlib's deflate writes after deflateSetDictionary; for an empty dictionary still FDICT, DICTID 1.
 * `packed` needs n * 10 + sum(max(tpbc, length + 5)) bytes at most (length + 10 for a job of more than 65 535 source bytes). */
int nxz_batch_pack_zlib_dict(nxz_ctx_t *ctx, int level, const nxz_dict_t *dict, const nxz_batch_job_t *jobs,
			     const nxz_batch_result_t *results, size_t n, uint64_t *offsets, uint8_t *packed, void *stream);

/* nxz_batch_decompress_framed for a caller that holds a dictionary: a zlib job with FDICT and DICTID == nxz_dict_id(dict) is
 * decoded with it (NXZ_FRAME_OK, hdr_len 6, dictid reported); another DICTID: NXZ_FRAME_NEED_DICT, nothing decoded.  A zlib job
 * without FDICT and every gzip job is decoded WITHOUT the dictionary, so a stream that refers to it anyway fails as in zlib.
 * One batch may mix all of these. */
int nxz_batch_decompress_framed_dict(nxz_ctx_t *ctx, int fmt, const nxz_dict_t *dict, const nxz_batch_job_t *jobs, size_t n,
				     nxz_batch_result_t *results, nxz_batch_frame_t *frames, void *stream);

/* ------------------------------------------------------------------------
 * Output sizes: what a batch of streams would produce, without decoding it
 * ---------------------------------------------------------------------- */
/* Every decompress call needs a target the caller has sized; raw deflate and zlib streams carry no length, and gzip's ISIZE is
 * modulo 2^32 and not to be trusted.  This call walks the streams (block headers, tables, tokens: power-gzip_amd/csrc/
 * nxz_inflate_size.hip, the rules in nxz_size.h) and writes results[i] = what nxz_batch_decompress would write for the same job
 * with a target of dst_cap bytes -- cc, tpbc, tebc, spbc, subc and sfbt, bit 8 of sfbt (final EOB seen) and out_dhtlen in bits
 * 16..27 included; a source that ends before the final block is CC 3 with the suspend fields.  The deviations:
 *   - no checksums, no dst: crc = adler = 0 (with them: nxz_batch_decompress_verify below).  dst is never read or written and may be NULL or misaligned; src may have any
 *     alignment.  No dht_io is written.
 *   - dst_cap is the limit: the walk stops with CC 13 at the token a decode would stop at.  0xffffffff = no limit; a stream of
 *     more than 2^32 - 1 bytes of output then gets CC 13.  On CC 13 and on the error codes 66 / 67 / 68 only cc is specified.
 *     NXZ_JOB_SUSPEND_WHEN_FULL is not honoured.
 *   - hist_len (<= 32768) counts only as how far a distance may reach in front of the output: the hist_len bytes at src are
 *     skipped, never read.  A job over [window][stream] -- and so any stream that uses a preset dictionary -- is sized by
 *     setting hist_len to the window (the dictionary's inflate window: its last min(len, 32768) bytes); that is why there is no
 *     _size_dict call.  resume != 0 or hist_len > 32768: cc = NXZ_CC_INVALID_OP, every other field 0.
 * The two-pass recipe: size, an exclusive prefix sum of tpbc rounded up to 16, jobs, decode.
 * Asynchronous on `stream`: no host wait, no allocation beyond the stream's scratch.
 * Speed: not measured yet.  tools/bench_size.py runs this call beside nxz_batch_decompress on the same streams and writes
 * profiles/r10_size.txt; a size query slower than the decode it spares is not worth having, so look there before relying on it. */
int nxz_batch_decompress_size(nxz_ctx_t *ctx, const nxz_batch_job_t *jobs, size_t n,
			      nxz_batch_result_t *results, void *stream);

/* The same for zlib / gzip streams: the header kernel of nxz_batch_decompress_framed (with `dict`, which may be NULL, that of
 * nxz_batch_decompress_framed_dict and its DICTID rules: a zlib job that names the dictionary is walked with the dictionary's
 * window as its reach), the size walk on the deflate data, and a trailer step that reads frames[i].check / isize and sets end.
 * Every NXZ_FRAME_* status is decided as in the decoding calls -- except NXZ_FRAME_BAD_CHECK, which cannot be detected without the
 * output (nxz_batch_decompress_verify_framed below makes the output's checksums without a target and does detect it): a job that a decode would call BAD_CHECK is reported as it would be if its check were right, that is NXZ_FRAME_OK, or
 * NXZ_FRAME_BAD_LENGTH when gzip's ISIZE differs from tpbc.  frames[i].check is the trailer's value as read.  jobs[].dst is not
 * touched; resume and hist_len must be 0 (NXZ_FRAME_BAD_HEADER). */
int nxz_batch_decompress_size_framed(nxz_ctx_t *ctx, int fmt, const nxz_dict_t *dict /* may be NULL */,
				     const nxz_batch_job_t *jobs, size_t n,
				     nxz_batch_result_t *results, nxz_batch_frame_t *frames, void *stream);

/* ------------------------------------------------------------------------
 * Verify: checksums and trailer checks, with no target for the decoded bytes
 * ---------------------------------------------------------------------- */
/* `gzip -t` over a batch.  The size walk above with every token applied to a ring of the last 32 KiB of output in LDS, as in
 * nxz_batch_checkpoint_build below, and the ring checksummed as the output passes through it (power-gzip_amd/csrc/
 * nxz_inflate_verify.hip, the rules in nxz_verify.h).  results[i] is field for field what nxz_batch_decompress_size writes for the
 * same job, and
 *   - crc and adler are the CRC-32 and the Adler-32 of the tpbc bytes the stream makes, continued from in_crc / in_adler as
 *     nxz_batch_decompress continues them.  Both are made for every job.  They are specified wherever the size call specifies the
 *     record: cc 0, and cc 3 with the suspend fields; on CC 13 and on the error codes only cc is specified, as there.
 *   - the hist_len (<= 32768) bytes at src are READ: they are the window that distances reach into.  A job over [window][stream]
 *     verifies exactly as nxz_batch_decompress decodes it, with hist_len = window.
 * dst is never read or written and may be NULL; src may have any alignment; dst_cap stays the limit (0xffffffff: none), the
 * 2^32 - 1 edge and the refusal of resume != 0 are the size call's.  Every array is a DEVICE array.
 * Asynchronous on `stream`: no host wait, no allocation beyond the stream's scratch.  Returns 0 (n == 0 included); -EINVAL (ctx,
 * n >= 2^31, jobs / results NULL with n > 0); -ENODEV in a forked child.
 * Not part of these calls: every member of a multi-member gzip job (the first is verified, frames[i].end tells where a second
 * starts; nxz_batch_gzip_members_size finds them all); parallelism inside one stream (one job is one wavefront's serial walk, as
 * in the size and build calls); any change to `nxz_gzip -t`.
 * Speed (profiles/r18_verify.txt, MI355X), against nxz_batch_decompress_framed into full targets: 23.5 times the decode's time on 64
 * zlib -6 streams of 16 MiB (953 ms against 41 ms) and 9.3 times on 4096 streams of 1 MiB (366 ms against 39 ms), holding 10 MiB of
 * device memory against 1102 MiB and 2 MiB against 4096 MiB.  That is 1.9 and 7.7 times the size walk; over the build call's walk plus
 * ring (898 ms, 235 ms) the checksum passes add 6 % and 36 % of the verify's time -- on 4096 streams part of that is three workgroups
 * a CU where the build kernel has four.  The decode is by far the faster one where its targets fit. */
int nxz_batch_decompress_verify(nxz_ctx_t *ctx, const nxz_batch_job_t *jobs, size_t n,
				nxz_batch_result_t *results, void *stream);

/* The same for zlib / gzip streams: the header kernel of nxz_batch_decompress_framed (with `dict`, which may be NULL, that of
 * nxz_batch_decompress_framed_dict and its DICTID rules), the verify walk on the deflate data -- a job that names the dictionary
 * has the dictionary's inflate window as its window, read from the dictionary's one device copy -- and the decode's own trailer
 * kernel, comparison included.  results[i] and frames[i] are exactly what nxz_batch_decompress_framed[_dict] writes for the same
 * jobs with targets large enough: NXZ_FRAME_BAD_CHECK and NXZ_FRAME_BAD_LENGTH are decided in the decode's order, and end, check
 * and isize match.  jobs[].dst is not touched; resume and hist_len must be 0 (NXZ_FRAME_BAD_HEADER).  -EINVAL also for fmt and
 * for a dictionary of another device, frames NULL with n > 0. */
int nxz_batch_decompress_verify_framed(nxz_ctx_t *ctx, int fmt, const nxz_dict_t *dict /* may be NULL */,
				       const nxz_batch_job_t *jobs, size_t n,
				       nxz_batch_result_t *results, nxz_batch_frame_t *frames, void *stream);

/* ------------------------------------------------------------------------
 * Multi-member gzip streams: member index and batch decode
 * ---------------------------------------------------------------------- */
/* RFC 1952: a gzip file is a series of members, and a reader decodes all of them (`cat a.gz b.gz`, WARC records, appended logs).
 * These two calls extend the two-pass recipe to jobs whose src is such a series; the member is the only granule here (checkpoints
 * inside a member and range reads: nxz_batch_checkpoint_index / nxz_checkpoint_read_ranges below).  The rules (power-gzip_amd/csrc/nxz_gzip_members.h), in the order they are checked:
 *   1. a job with resume or hist_len set: NXZ_GZS_INVALID, nothing walked;
 *   2. member 0 is parsed at offset 0 by the gzip parser of the framed calls;
 *   3. behind an OK member that ends at e: e == src_len -- stop, NXZ_GZS_OK; fewer than 2 bytes left, or the next two are not
 *      1f 8b -- stop, NXZ_GZS_OK with consumed = e (trailing zeros and trailing garbage are the caller's business, as with
 *      frames[i].end); otherwise the next member starts at e;
 *   4. a member that fails (header, FHCRC, truncation, deflate data, ISIZE != the counted size) ends the walk:
 *      NXZ_GZS_MEMBER_FAILED, failed = its index, its record carries the NXZ_FRAME_* status; the members before it stay valid;
 *   5. members beyond member_cap are walked and counted (members, out_len, consumed are true values) but not stored:
 *      NXZ_GZS_MORE_MEMBERS, unless a member failed;
 *   6. uoff is the running sum of the OK members' sizes.
 * A failed member's record holds uoff, coff and status, hdr_len when its header was read, and clen, check and the counted isize
 * when its trailer was read (NXZ_FRAME_BAD_LENGTH); its other fields are 0. */
typedef struct nxz_gzip_member {   /* DEVICE, 32 bytes; offsets count from the job's src / dst */
	uint64_t uoff;             /* where the member's output starts in the job's output */
	uint32_t coff, clen;       /* member start, header + deflate + trailer bytes */
	uint32_t hdr_len, isize;   /* isize: the size the walk counted (== ISIZE as read when status is OK) */
	uint32_t check;            /* CRC-32 as read */
	uint32_t status;           /* NXZ_FRAME_* of this member */
} nxz_gzip_member_t;
typedef struct nxz_gzip_stream {   /* DEVICE, 32 bytes, one per job */
	uint32_t status;           /* NXZ_GZS_* */
	uint32_t members;          /* members found (may exceed member_cap) */
	uint32_t failed;           /* index of the first member whose status != NXZ_FRAME_OK (else == members) */
	uint32_t consumed;         /* bytes of src covered by whole OK members */
	uint64_t out_len;          /* sum of isize over the OK members (64 bits: may pass 4 GiB in the size call) */
	uint32_t cc, reserved;     /* raw decoder's code of the failed member (3 when its deflate data was cut short), else 0 */
} nxz_gzip_stream_t;
enum { NXZ_GZS_OK = 0, NXZ_GZS_MEMBER_FAILED, NXZ_GZS_MORE_MEMBERS, NXZ_GZS_TARGET_SPACE, NXZ_GZS_INVALID };

/* Pass 1, the member index: one wavefront walks a job member after member inside ONE launch (power-gzip_amd/csrc/
 * nxz_gzip_members.hip) -- header, the size walk of nxz_batch_decompress_size over the deflate bytes, the 8-byte trailer --
 * and writes members[i * member_cap + k] for k < min(members found, member_cap) and streams[i].  jobs[].src may have any
 * alignment; dst and dst_cap are not looked at, nothing but the two arrays is written.  A member of more than 2^32 - 1 bytes
 * of output is NXZ_FRAME_DEFLATE (cc 13).  One huge job is one wavefront's serial walk: parallelism comes from the batch.
 * zlib streams are not concatenable and are not handled; no dictionaries.
 * jobs, members (n * member_cap records) and streams (n) are DEVICE arrays.  Asynchronous on `stream`, no host wait.
 * Returns 0 (n == 0 included); -EINVAL (ctx, member_cap == 0, n >= 2^31, a NULL array with n > 0); -ENODEV in a forked child. */
int nxz_batch_gzip_members_size(nxz_ctx_t *ctx, const nxz_batch_job_t *jobs, size_t n, uint32_t member_cap,
				nxz_gzip_member_t *members /* n * member_cap */, nxz_gzip_stream_t *streams, void *stream);

/* Pass 2, the decode, from the arrays pass 1 wrote (the same member_cap): the first min(streams[i].failed, member_cap) members
 * of every job -- its stored OK members -- become framed gzip jobs (src + coff, clen bytes, into dst + uoff, isize bytes) in the
 * stream's scratch and go through the routes of nxz_batch_decompress_framed as ONE batch of at most total_members jobs; then the
 * decode's verdict is joined back: members[].status takes the frame status (NXZ_FRAME_BAD_CHECK shows here, the size pass cannot
 * see it), streams[i].out_len becomes the bytes decoded -- the sizes of the members that decoded OK --, and a job with a member
 * that failed gets NXZ_GZS_MEMBER_FAILED, failed = the first such index and cc = its raw result's code; the other members of the
 * job are decoded all the same.  A job the decode does not touch at all (dst not written, its streams[i] unchanged but for status):
 *   NXZ_GZS_TARGET_SPACE   streams[i].out_len > jobs[i].dst_cap;
 *   NXZ_GZS_INVALID        its summary is none of OK / MEMBER_FAILED / MORE_MEMBERS (refused before: the size pass again); or one of
 *                          its stored OK records is not OK or points outside the job
 *                          (coff + clen > src_len, uoff + isize > dst_cap: a stale or foreign index); or total_members is too
 *                          small for the batch -- then every job from the first that does not fit on.
 * total_members (HOST) is an upper bound of the members to decode: n * member_cap is always one, sum(min(failed, member_cap))
 * is the tightest; slots beyond the real count are empty jobs that every route ends at once.  Member outputs land at arbitrary
 * offsets of the job's target: a member whose dst is not 16-byte aligned takes the stream-per-wavefront route, as BGZF members
 * of odd sizes do in nxz_batch_unpack_gzip.
 * Asynchronous on `stream`: no host wait, no allocation once the stream's scratch holds a batch of this size (about 150 bytes a
 * member).  Returns 0 (n == 0 included); -EINVAL (ctx, member_cap == 0, total_members < n, n >= 2^31, a NULL array with n > 0);
 * -E2BIG (min(total_members, n * member_cap) >= 2^31); -ENOMEM; -ENODEV in a forked child.
 * Speed: not measured yet; tools/bench_members.py writes profiles/r12_members.txt. */
int nxz_batch_gzip_members_decode(nxz_ctx_t *ctx, const nxz_batch_job_t *jobs, size_t n, uint32_t member_cap,
				  nxz_gzip_member_t *members, nxz_gzip_stream_t *streams,
				  size_t total_members /* HOST: an upper bound, n * member_cap is always one */, void *stream);

/* ------------------------------------------------------------------------
 * One stream per device buffer: batched deflate of buffers of any length
 * ---------------------------------------------------------------------- */
/* The compress-side counterpart of the framed decode: a batch of DEVICE buffers of any length, each written as ONE raw, zlib or
 * gzip stream in DEVICE memory -- what nxz_deflate_host[_hist] does for one host buffer, without leaving the device (a Parquet
 * page, a Zarr or HDF5 chunk, a tensor).  fc = NXZ_FC_COMPRESS_FHT or NXZ_FC_COMPRESS_DHTGEN (else -EINVAL).  hist_max as in
 * nxz_deflate_host_hist: rounded down to a multiple of 16, 32768 at most; a block carries B = 65536 - H source bytes and block k
 * sees the min(H, k * B) bytes of the same buffer in front of it.  The deflate data of stream i is byte for byte what
 * nxz_deflate_host_hist(fc, buffer i, final = 1, hist_max, prev = NULL) writes: the same cut, the same empty stored block behind a
 * block that ends inside a byte, the same stored-block fallback, BFINAL on the last block.  Around it:
 *   NXZ_FMT_RAW    nothing
 *   NXZ_FMT_ZLIB   78 and FLG with FLEVEL from `level` (-1, 0..9: as nxz_batch_pack_zlib) in front, the Adler-32 big-endian behind
 *   NXZ_FMT_GZIP   1f 8b 08 00 00 00 00 00 04 03 in front, CRC-32 and ISIZE = src_len mod 2^32 little-endian behind
 * A buffer of length 0 gives the body 01 00 00 ff ff and blocks = 0.  `level` chooses nothing but FLEVEL.
 * jobs is a HOST array (the caller knows its buffers' sizes) and may be reused as soon as the call returns: what the engine needs
 * of it goes into pinned staging of the stream's scratch, and the host work is one pass over the streams, not over their blocks.
 * results is a DEVICE array.  A stream that is refused (results[i].cc) costs nothing and leaves its neighbours alone.
 * The blocks of the whole batch go through nxz_batch_compress in chunks of NXZ_STREAMS_CHUNK blocks (environment, read at every
 * call; default 4096, about 300 MB of scratch for the blocks' outputs before they are packed); a stream may straddle chunks, and
 * the output does not depend on the chunk size.  On the device: job expansion, layout and checksum joins, packing with framing
 * (power-gzip_amd/csrc/nxz_streams.hip, the rules in nxz_streams.h).
 * Asynchronous on `stream`: no host wait and no device allocation once the stream's scratch has grown to the batch.
 * Returns 0; -EINVAL (ctx, fc, fmt, level, jobs or results NULL with n != 0); -ENODEV in a forked child; -E2BIG when the batch
 * holds 2^31 blocks (or streams) or more; -ENOMEM when scratch cannot be had.
 * Speed (tools/bench_streams.py, profiles/r11_streams.txt; zlib, DHTGEN, hist_max 0): 0.93 of the rate of nxz_batch_compress +
 * nxz_batch_pack_zlib on the same bytes cut into 64 KiB jobs, a member per block (94 against 102 GiB/s for 4096 streams of 1 MiB and
 * for 65 536 of 64 KiB; one stream of 1 GiB: 0.77).  With hist_max 32768 -- twice the jobs -- 0.71 to 0.76, one stream 0.53. */
enum { NXZ_FMT_RAW = 0 };            /* beside NXZ_FMT_ZLIB = 1, NXZ_FMT_GZIP = 2 */
typedef struct nxz_stream_job {      /* HOST array */
	const uint8_t *src;          /* DEVICE, 16-byte aligned */
	uint8_t       *dst;          /* DEVICE, any alignment */
	uint64_t       src_len;      /* any length, 0 included */
	uint64_t       dst_cap;      /* >= nxz_deflate_stream_bound(src_len, hist_max, fmt) */
} nxz_stream_job_t;
typedef struct nxz_stream_result {   /* DEVICE array, written by the device, 32 bytes */
	uint32_t cc;                 /* 0; NXZ_CC_TARGET_SPACE (dst_cap below the bound: out_len = the bound, dst untouched);
	                                NXZ_CC_INVALID_OP (src NULL with src_len != 0, src not 16-byte aligned, dst NULL: dst untouched) */
	uint32_t blocks;             /* compress jobs the stream was cut into */
	uint64_t out_len;            /* bytes at dst: header + deflate data + trailer */
	uint32_t crc, adler;         /* of the source, from 0 / 1 */
	uint32_t stored;             /* blocks that went out as stored blocks */
	uint32_t reserved;
} nxz_stream_result_t;
/* nxz_deflate_host_bound_hist(src_len, hist_max) + 0 (raw) / 6 (zlib) / 18 (gzip) */
size_t nxz_deflate_stream_bound(uint64_t src_len, uint32_t hist_max, int fmt);
int nxz_batch_deflate_streams(nxz_ctx_t *ctx, int fc, int fmt, int level, uint32_t hist_max,
			      const nxz_stream_job_t *jobs /* HOST */, size_t n,
			      nxz_stream_result_t *results /* DEVICE */, void *stream);

/* The same call with the streams' CHECKPOINT INDEX as a by-product (the checkpoint section below has the index's rules, its
 * arrays and its readers): the call laid every block into its stream at a known byte, so it writes the rows that
 * nxz_batch_checkpoint_index would find by walking the finished streams -- without decoding anything and without the host wait
 * for out_len that building the index jobs costs.  Everything up to `results` is nxz_batch_deflate_streams's: the bytes at every
 * dst and every results[i] are exactly what that call writes for the same arguments.
 * Row i -- cbit / uoff [i * (cp_cap + 1) + k], streams[i] and, with windows, slots i * cp_cap + k -- is exactly what
 * nxz_batch_checkpoint_index(fmt, job{src = jobs[i].dst, src_len = out_len, dst = jobs[i].src, dst_cap = src_len}, span, cp_cap, ...)
 * writes: rules 1 to 5, the sentinel at [count] when count <= cp_cap, NXZ_CPS_MORE with the true count and no sentinel beyond that,
 * format = fmt, hdr_len, out_len = src_len.  A checkpoint may stand inside a byte (the empty stored block behind a block that ends
 * inside one).  windows (DEVICE, n * cp_cap slots of 32768 bytes, or NULL: positions only): the first min(uoff[k], 32768) bytes of
 * slot i * cp_cap + k are jobs[i].src[uoff[k] - w, uoff[k]); the rest of a slot and the slots beyond the stored checkpoints are not
 * written.
 * A stream that gets no index: one the compress side refuses (results[i].cc != 0), or one whose src_len or out_len does not fit 32
 * bits -- the limit of the index format; it is compressed all the same.  streams[i].status = NXZ_CPS_INVALID, count = 0,
 * cc = results[i].cc; its row and slots are not written (of a stream whose src_len fits and whose out_len turns out not to, the
 * entries found before the end are), the neighbours are unaffected.
 * index_jobs (DEVICE, n, or NULL): index_jobs[i] = the job the readers want -- src = jobs[i].dst, src_len = out_len, dst = NULL,
 * in_adler = 1, every other field 0; src = NULL and src_len = 0 for a stream without an index.  Then
 * nxz_batch_checkpoint_read_ranges(ctx, index_jobs, n, cp_cap, cbit, uoff, NULL, windows, streams, ...) reads ranges with no host
 * step in between.
 * On the device (power-gzip_amd/csrc/nxz_streams_index.hip, the rules in nxz_streams_index.h): per chunk a sweep over the block headers
 * behind the layout -- a wavefront a stream, one step per checkpoint found; (c, count) go from chunk to chunk, the index does not
 * depend on NXZ_STREAMS_CHUNK -- and a copy of the windows beside the packing, 32 KiB per stored checkpoint: at span = B half the
 * source again.  Asynchronous on `stream`: no host wait and no allocation once the stream's scratch has grown.
 * Returns as nxz_batch_deflate_streams, and -EINVAL for span == 0, cp_cap == 0, cbit, uoff or streams NULL with n > 0,
 * n * (cp_cap + 1) >= 2^32.
 * Not part of this call: the dictionary form (a first segment whose window is the dictionary has no place in the row format);
 * checkpoints inside blocks (a reader passes state == NULL); compressing or deduplicating the windows.
 * Speed (tools/bench_streams_indexed.py, profiles/r23_streams_indexed.txt; zlib, DHTGEN, hist_max 0 and 32768, a checkpoint every 64 KiB
 * and every 1 MiB): 1.01 to 1.03 of the time of nxz_batch_deflate_streams alone for 4096 streams of 1 MiB (42.9 against 41.8 ms at
 * 64 KiB, hist_max 0), 1.04 to 1.07 for 64 streams of 16 MiB (11.4 against 10.7 ms); against the route it replaces -- that call, the
 * host wait for out_len, jobs built on the host, nxz_batch_checkpoint_index with windows from the source -- 0.34 to 0.40 of the time
 * for the first shape (124 ms) and 0.015 to 0.02 for the second (753 ms: a wavefront walks 16 MiB). */
struct nxz_checkpoint_stream;         /* nxz_checkpoint_stream_t, below */
int nxz_batch_deflate_streams_indexed(nxz_ctx_t *ctx, int fc, int fmt, int level, uint32_t hist_max,
				      const nxz_stream_job_t *jobs /* HOST */, size_t n, nxz_stream_result_t *results /* DEVICE */,
				      uint64_t span, uint32_t cp_cap,
				      uint64_t *cbit, uint64_t *uoff,            /* DEVICE, n * (cp_cap + 1) each */
				      uint8_t *windows,                          /* DEVICE, n * cp_cap * 32768, or NULL */
				      struct nxz_checkpoint_stream *streams,     /* DEVICE, n */
				      nxz_batch_job_t *index_jobs,               /* DEVICE, n, or NULL */
				      void *stream);

/* The same with ONE preset dictionary for all streams (the device-side deflateSetDictionary for buffers of any length; what
 * nxz_batch_compress_dict + nxz_batch_pack_zlib_dict do for sources that fit one block).  Everything not named here is as in
 * nxz_batch_deflate_streams: jobs, results, fc, level, the chunks, asynchrony.
 * The block plan does not change: H = hist_max rounded as above, B = 65536 - H, block k starts at k * B and, for k >= 1, sees the
 * H bytes of its own buffer in front of it.  Block 0 sees the last h0 = min(H, len) & ~15 bytes of the dictionary -- the `prev`
 * rule of nxz_deflate_host_hist, not the dictionary's own deflate window: hist_max bounds this window as it bounds the others
 * (hist_max 4096 and a dictionary of 32 KiB: its last 4096 bytes).  WITH hist_max < 16 (H == 0) NO BLOCK HAS A WINDOW: the
 * stream names the dictionary in its header and never refers to it; a caller who wants the dictionary used passes a hist_max
 * (32768 for all of it).  The deflate data of stream i is byte for byte what nxz_deflate_host_hist(fc, buffer i, final = 1,
 * hist_max, prev = the dictionary's bytes, prev_len = len) writes; a buffer of length 0 gives 01 00 00 ff ff and blocks = 0.
 *   NXZ_FMT_RAW    nothing around it
 *   NXZ_FMT_ZLIB   the six bytes of nxz_batch_pack_zlib_dict in front (78, FLG with FLEVEL from `level` and FDICT, then
 *                  nxz_dict_id(dict) most significant byte first: the DICTID of the WHOLE dictionary, 1 for an empty one), the
 *                  Adler-32 of the source alone big-endian behind
 *   NXZ_FMT_GZIP   -EINVAL: gzip has no dictionary field
 * The streams inflate with zlib's inflateSetDictionary(the whole dictionary), with nxz_batch_decompress_dict (raw) and with
 * nxz_batch_decompress_framed_dict (zlib).  dst_cap >= nxz_deflate_stream_bound_dict(src_len, hist_max, fmt) = the plain bound,
 * and 4 more for zlib (0 for a format that is not taken); the refusals are the plain call's against this bound, and on
 * NXZ_CC_TARGET_SPACE out_len is this bound.
 * On the device a stream's first block goes through the LZ77 kernel as a dictionary job (its window read from the dictionary's
 * one device copy, nothing read below the buffer), every other block as a plain history job: per chunk two LZ77 launches, one
 * table and one entropy launch, and one small launch that puts the results back in order (power-gzip_amd/csrc/nxz_streams_dict.hip,
 * the rules in nxz_streams_dict.h).  How many first blocks a chunk holds the host knows from its pass over the streams: no host wait.
 * Returns as nxz_batch_deflate_streams; -EINVAL also for dict == NULL, a dictionary of another device, NXZ_FMT_GZIP.
 * Speed (tools/bench_streams_dict.py, profiles/r19_streams_dict.txt; zlib, DHTGEN, hist_max 32768): 65 536 records of 256 B to 4 KiB
 * with a 32 KiB dictionary 11.5 GiB/s, 0.85 of the rate of nxz_batch_compress_dict + nxz_batch_pack_zlib_dict on the same records
 * (13.6 GiB/s, the same bytes out) and 0.78 of the compressed bytes of nxz_batch_deflate_streams without the dictionary; 4096 streams
 * of 1 MiB 69.7 GiB/s, 0.95 of nxz_batch_deflate_streams (73.5): the chunk's LZ77 work ends twice, once per launch. */
size_t nxz_deflate_stream_bound_dict(uint64_t src_len, uint32_t hist_max, int fmt);
int nxz_batch_deflate_streams_dict(nxz_ctx_t *ctx, int fc, int fmt, int level, uint32_t hist_max,
				   const nxz_dict_t *dict,
				   const nxz_stream_job_t *jobs /* HOST */, size_t n,
				   nxz_stream_result_t *results /* DEVICE */, void *stream);

/* A stream WRITTEN IN PARTS: the source of stream i arrives over several calls (a shard that grows, a tensor stream written layer
 * by layer, a file larger than what is resident), each call compresses the part it is given and appends to nothing -- the bytes of
 * THIS part go to jobs[i].dst and the caller lays the parts' out_len bytes end to end.  What a stream carries from call to call is
 * carry[i] (DEVICE, read and written by the device: a later call may be queued behind an earlier one with no host step between)
 * and the source bytes just in front of the part, which the caller keeps or leaves where they are.  Everything not named here is
 * nxz_batch_deflate_streams's: fc, fmt, level, hist_max and its rounding, NXZ_STREAMS_CHUNK, the error returns, the asynchrony.
 * The block plan of a part is the plan of a buffer: H = hist_max rounded, B = 65536 - H, block k starts at k * B and, for k >= 1,
 * sees the H bytes of its own part in front of it.  Block 0 sees the last h0 = min(H, prev_len) & ~15 bytes of `prev` -- the `prev`
 * rule of nxz_deflate_host_hist, which nxz_batch_deflate_streams_dict restates for its dictionary; h0 == 0: no window.  The
 * deflate data of a part is byte for byte what nxz_deflate_host_hist(fc, src, src_len, final = LAST, hist_max, prev, prev_len)
 * writes: a part without NXZ_PART_LAST carries no BFINAL and ends on a byte boundary (the empty stored block behind a last block
 * that ends inside a byte), so the stream written so far inflates to every source byte so far; a part of length 0 writes no
 * deflate data without LAST and 01 00 00 ff ff with it.
 *   NXZ_PART_FIRST   the plain call's header in front (0, 2 or 10 bytes); the incoming carry[i] is ignored and started afresh
 *   NXZ_PART_LAST    the plain call's trailer behind, from the carry: the Adler-32 or the CRC-32 of all parts, ISIZE = total_in
 *                    mod 2^32; carry[i].status = 1
 * dst_cap >= nxz_deflate_stream_part_bound(src_len, hist_max, fmt, flags) = src_len + 10 a block + 16, the header with FIRST, the
 * trailer with LAST.  results[i]: out_len = this part's bytes at dst, blocks and stored count this part's blocks, crc and adler
 * are the running values of the whole stream through this part (the carry's).  For a job with FIRST | LAST the bytes at dst and
 * results[i] are exactly what nxz_batch_deflate_streams writes for the same arguments.
 * Refused (results[i].cc; dst and carry[i] untouched, the neighbours unaffected, the part may be sent again): the plain call's
 * refusals against this bound (NXZ_CC_TARGET_SPACE: out_len = the bound), and NXZ_CC_INVALID_OP for prev == NULL with
 * prev_len != 0, flag bits other than the two, FIRST with prev_len != 0 (a preset window on a stream's first part is the
 * dictionary call's job), no FIRST on a carry whose status != 0.
 * Where the window comes from: with prev + prev_len == src (the parts lie one behind the other in memory) block 0's compress job
 * simply begins h0 bytes in front of src and nothing is copied.  Otherwise a kernel of its own stages [window][block 0] in 64 KiB
 * of the stream's scratch per such block of a chunk -- 16 bytes a lane, the window from any alignment through aligned loads
 * joined by a byte shift -- and the job reads from there.  On the device: power-gzip_amd/csrc/nxz_streams_part.hip, the rules in
 * nxz_streams_part.h; which blocks are staged the host knows from its one pass over the streams.
 * Asynchronous on `stream`: no host wait and no allocation once the stream's scratch has grown.  Returns as
 * nxz_batch_deflate_streams, and -EINVAL for carry == NULL with n > 0.
 * Not part of this call: the dictionary form; the indexed form; carrying a partly filled byte from part to part (a part always
 * ends on a byte boundary: up to five bytes a part more than one call on the whole source writes); nx_deflate on top of it.
 * Speed (tools/bench_streams_part.py, profiles/r24_streams_part.txt; zlib, DHTGEN, 4096 streams of 1 MiB, medians of 5 runs taken in
 * turn, every route within 0.2 % of its median): one FIRST | LAST part 1.002 (hist_max 0) and 1.001 (32768) of the time of
 * nxz_batch_deflate_streams (41.79 against 41.70 ms, 54.56 against 54.51) -- inside that call's own spread.  A stream in 4 parts of
 * 256 KiB, a call a part: 1.006 / 1.008 with the parts contiguous, 1.007 / 1.017 with prev detached (every part's first block staged);
 * in 16 parts of 64 KiB: 1.019 / 1.022 contiguous, 1.020 / 1.053 detached (57.4 against 54.5 ms: with hist_max 32768 every second
 * block of the batch is staged). */
enum { NXZ_PART_FIRST = 1u, NXZ_PART_LAST = 2u };
typedef struct nxz_stream_part_job {   /* HOST array */
	const uint8_t *src;            /* DEVICE, 16-byte aligned: this part's source */
	uint8_t       *dst;            /* DEVICE, any alignment: where THIS part's bytes go (the caller appends them to the stream) */
	uint64_t       src_len;        /* any length, 0 included */
	uint64_t       dst_cap;        /* >= nxz_deflate_stream_part_bound(src_len, hist_max, fmt, flags) */
	const uint8_t *prev;           /* DEVICE or NULL, any alignment: the prev_len source bytes of the stream just in front of this part */
	uint32_t       prev_len;       /* any value; only the tail counts (above) */
	uint32_t       flags;          /* NXZ_PART_FIRST | NXZ_PART_LAST */
} nxz_stream_part_job_t;
typedef struct nxz_stream_carry {      /* DEVICE, 32 bytes, one per stream, read and written by the device */
	uint32_t crc, adler;           /* of all source bytes so far, from 0 / 1 */
	uint64_t total_in, total_out;  /* source bytes taken / stream bytes written so far, framing included */
	uint32_t parts;                /* parts taken, empty ones included */
	uint32_t status;               /* 0 open, 1 finished */
} nxz_stream_carry_t;
size_t nxz_deflate_stream_part_bound(uint64_t src_len, uint32_t hist_max, int fmt, uint32_t flags);
int nxz_batch_deflate_streams_part(nxz_ctx_t *ctx, int fc, int fmt, int level, uint32_t hist_max,
				   const nxz_stream_part_job_t *jobs /* HOST */, size_t n,
				   nxz_stream_carry_t *carry /* DEVICE, n, in/out */,
				   nxz_stream_result_t *results /* DEVICE, n */, void *stream);

/* The decode side (additive): a batch of raw / zlib / gzip streams READ in parts, n streams a call, one part of each -- the pieces a
 * socket, a range GET or nxz_batch_deflate_streams_part's own writer hand over.  jobs[] is a HOST array (it may be reused on
 * return); carry[] and results[] are DEVICE arrays, read and written by the device only, so part k + 1 of the whole batch may be
 * queued behind part k with no host step between.  fmt: NXZ_FMT_RAW (0), _ZLIB, _GZIP or _AUTO (per stream, as the framed call).
 * A part is THIS call's compressed bytes (src, src_len: any alignment, any length, 0 included) and a target for THIS call's output
 * (dst, dst_cap: any alignment; 16-byte aligned takes the faster route, as everywhere).  `prev` / prev_len: the OUTPUT bytes of
 * the stream just in front of dst, of which the last min(32768, prev_len, total_out) count; prev + prev_len == dst is the ordinary
 * case of outputs laid end to end.  The decode kernels want the history in front of the SOURCE, so the window is always staged:
 * [window][tail][this part from the deflate data's first byte] goes into a 16-byte aligned slot of the stream's scratch (16 bytes
 * a lane, sources of any alignment through aligned loads joined by a byte shift; one grid over all bytes of a chunk) and the raw
 * batch decodes from there with NXZ_JOB_SUSPEND_WHEN_FULL.  A part with neither window nor tail is decoded where it lies.
 * flags: NXZ_PART_FIRST only -- the incoming carry[i] is ignored and started afresh; there is no LAST, the stream says where it ends.
 * carry[i] (fixed size, needs no initial value before a FIRST part) holds the phase (header / body / trailer / done / failed), the
 * frame's facts and verdict so far (an nxz_batch_frame_t: offsets count from the stream's first byte, `end` = the bytes of the
 * stream through its trailer), where the header's byte-wise state machine stands (which field, bytes left of FEXTRA or DICTID, the
 * running header CRC for FHCRC: a header of any length may be cut anywhere, one byte a part included, and needs no tail), the decode
 * state as nxz_stream_resume_t has it plus subc, crc / adler of all output, total_in / total_out / parts, and the TAIL: the
 * tail_len source bytes that were handed over and must be seen again.  The stream stands at byte total_in - tail_len;
 * [tail][next part] is its continuation and subc applies to the first byte of that.  A part that ends inside a token leaves at most
 * 7 bytes there, one that ends inside a block header the header read so far (the engine suspends IN FRONT of a header it cannot
 * finish), one that ends inside the trailer at most 7 bytes.
 * results[i]: cc = the decode's own code (or NXZ_CC_INVALID_OP: refused); out_len = bytes written at dst by this part; crc / adler
 * the running values of the whole stream; status and in_used:
 *   NXZ_INFLATE_PART_MORE      the stream is open, send the next part; in_used = src_len
 *   NXZ_INFLATE_PART_DONE      trailer read and checked; in_used = the byte behind it (bytes beyond are no error; a second gzip member
 *                              is not decoded: start it with FIRST at src + in_used)
 *   NXZ_INFLATE_PART_DST_FULL  suspended in front of the token that did not fit (a stored block: at the byte); in_used < src_len,
 *                              0 when the target filled inside the old tail: send src + in_used again with a fresh target.  A target
 *                              that fills at a token inside the part's last byte is MORE: that byte is the tail
 *   NXZ_INFLATE_PART_FAILED    carry[i].frame.status says why (NXZ_FRAME_DEFLATE: look at cc); in_used = 0, behind a trailer that
 *                              was read and does not match the byte behind it.  zlib FDICT: NXZ_FRAME_NEED_DICT with dictid set,
 *                              nothing decoded
 * Refused (cc = NXZ_CC_INVALID_OP, status FAILED; dst and carry[i] untouched, the neighbours unaffected, the part may be sent again):
 * src == NULL with src_len != 0, dst == NULL with dst_cap != 0, prev == NULL with prev_len != 0, flag bits other than FIRST, FIRST
 * with prev_len != 0, no FIRST on a carry that is done or failed.
 * For a stream that arrives whole in one FIRST part dst, out_len, crc / adler, the frame's facts and in_used (= frame.end) are what
 * nxz_batch_decompress_framed writes for the same bytes.
 * The work goes chunk by chunk: NXZ_INFLATE_PART_SCRATCH (bytes, read at every call, default 512 MiB) bounds the staging slots of a
 * chunk, a stream larger than it gets a chunk of its own, 16 384 streams a chunk at most; the result does not depend on it.  Per
 * chunk: open (refusals, FIRST, header state machine, trailer, the derived job and its table slot), stage, nxz_batch_decompress kept
 * off the stream-per-lane kernel as the fine range reads are (NXZ_JOB_SUSPEND_WHEN_FULL), close (result and table slot -> carry
 * and results[i]).  Streams that are not in the body phase reach the decode as empty jobs.  On the device:
 * power-gzip_amd/csrc/nxz_inflate_part.hip, the rules in nxz_inflate_part.h.
 * NXZ_INFLATE_PART_TAIL: the longest dynamic block header RFC 1951 allows is 3 + 14 + 19 * 3 + 316 * 7 = 2286 bits (BFINAL / BTYPE;
 * HLIT, HDIST, HCLEN; 19 code length code lengths; 316 lengths coded singly with 7-bit codes), it may start at any of the 8 bits of
 * a byte: 2293 bits = 287 bytes, rounded up to the next multiple of 16 (tests/test_inflate_part_model_host.py builds that header).
 * Asynchronous on `stream`: no host wait and no device allocation once the stream's scratch has grown.  Returns 0, -EINVAL (a NULL
 * array with n > 0, an unknown fmt), -ENODEV, -E2BIG (n >= 2^31) or -ENOMEM as nxz_batch_deflate_streams_part does.
 * Not part of this call: a shared dictionary; the gzip members that follow the first; size-only and verify-only forms; nx_inflate
 * on top of it; zero-copy windows (a window that already lies in front of the source).
 * Speed (tools/bench_inflate_part.py, profiles/r25_inflate_part.txt; 4096 zlib -6 streams of 1 MiB of output, medians of 5 runs taken in
 * turn, every route within 0.4 % of its median but (r): 3 %): one FIRST part 1.063 of the time of nxz_batch_decompress_framed (52.57 against
 * 49.45 ms; nothing is staged: the 3 ms are what the call puts around the same decode, not separated further).  A stream in 4 parts with all calls queued and one
 * wait 268.0 ms, in 16 parts 199.7 ms: 5.4 and 4.0 times the framed call, and 0.73 and 0.28 of the only route there was before --
 * nxz_batch_decompress with resume jobs, a host wait and host-built jobs and layouts between the parts: 367.1 and 701.5 ms.  The staging
 * does not explain what the parts cost over the framed call: 1.33 and 3.05 GiB staged against 219 and 150 ms.  The time is the decode of
 * the parts behind the first: a job with history or resume state goes a stream per wavefront, and a wavefront takes about 55 ms for a
 * part of 256 KiB of output and 10 ms for one of 64 KiB however few streams there are -- 96 streams take 221 ms in 4 parts, queued or
 * built by the host alike.  Resume jobs on the stream-per-workgroup kernel would take that away; that kernel is not part of this call. */
#define NXZ_INFLATE_PART_TAIL 288
enum { NXZ_INFLATE_PHASE_HEADER = 0, NXZ_INFLATE_PHASE_BODY, NXZ_INFLATE_PHASE_TRAILER, NXZ_INFLATE_PHASE_DONE, NXZ_INFLATE_PHASE_FAILED };
enum { NXZ_INFLATE_PART_MORE = 0, NXZ_INFLATE_PART_DONE, NXZ_INFLATE_PART_DST_FULL, NXZ_INFLATE_PART_FAILED };
typedef struct nxz_inflate_part_job {  /* HOST array, 40 bytes */
	const uint8_t *src;            /* DEVICE, any alignment: this part's compressed bytes */
	uint8_t       *dst;            /* DEVICE, any alignment: where THIS part's output goes */
	const uint8_t *prev;           /* DEVICE or NULL, any alignment: the prev_len output bytes of the stream just in front of dst */
	uint32_t       src_len;        /* any length, 0 included */
	uint32_t       dst_cap;
	uint32_t       prev_len;       /* any value; only the tail counts (above) */
	uint32_t       flags;          /* NXZ_PART_FIRST */
} nxz_inflate_part_job_t;
typedef struct nxz_inflate_carry {     /* DEVICE, 704 bytes, one per stream, read and written by the device */
	uint32_t phase;                /* NXZ_INFLATE_PHASE_* */
	uint32_t hpos;                 /* header: the field the next byte belongs to (nxz_inflate_part.h) */
	uint32_t hleft;                /* header: bytes left of FEXTRA / DICTID */
	uint32_t hcrc;                 /* header: the CRC-32 register over the header bytes so far */
	nxz_batch_frame_t frame;       /* the frame's facts and its verdict (status) so far */
	uint32_t hfirst;               /* header: the stream's first byte (zlib CMF; NXZ_FMT_AUTO decides at the second) */
	uint32_t sfbt, rem, dhtlen;    /* the decode state, as nxz_stream_resume_t */
	uint32_t subc;                 /* unused bits of the first byte of [tail][next part], 0 = all eight */
	uint32_t crc, adler;           /* of all output so far, from 0 / 1 */
	uint32_t parts;                /* parts taken, empty ones included */
	uint32_t tail_len;
	uint32_t reserved[2];
	uint64_t total_in, total_out;  /* source bytes taken / output bytes written so far */
	uint8_t  dht[NXZ_DHT_MAXSZ];
	uint8_t  tail[NXZ_INFLATE_PART_TAIL];
} nxz_inflate_carry_t;
typedef struct nxz_inflate_part_result { /* DEVICE, 32 bytes, written by the device */
	uint32_t cc;
	uint32_t status;               /* NXZ_INFLATE_PART_* */
	uint32_t in_used;
	uint32_t out_len;
	uint32_t crc, adler;
	uint32_t reserved[2];
} nxz_inflate_part_result_t;
int nxz_batch_inflate_streams_part(nxz_ctx_t *ctx, int fmt /* NXZ_FMT_RAW, ZLIB, GZIP, AUTO */,
				   const nxz_inflate_part_job_t *jobs /* HOST */, size_t n,
				   nxz_inflate_carry_t *carry /* DEVICE, n, in/out */,
				   nxz_inflate_part_result_t *results /* DEVICE, n */, void *stream);

/* The byte-shuffle filter (additive): what stands between a numeric Zarr or HDF5 chunk and its deflate stream.  HDF5's standard
 * pipeline for chunked numeric datasets is H5Z_FILTER_SHUFFLE followed by deflate, Zarr's numcodecs.Shuffle + zlib; the rule here is
 * HDF5's.  With N = len / elem and r = len % elem, nxz_batch_shuffle writes dst[j * N + i] = src[i * elem + j] for i < N, j < elem --
 * byte 0 of every element, then byte 1 of every element, ... -- and copies the r leftover bytes unchanged to dst[N * elem ..].
 * nxz_batch_unshuffle is the exact inverse under the same (len, elem).  elem == 1 and len < elem are plain copies.
 * Write side: shuffle, then nxz_batch_deflate_streams(NXZ_FMT_ZLIB) on the shuffled buffer; read side: nxz_batch_decompress_framed,
 * then unshuffle with the chunk's known size and element size.
 * jobs is a HOST array and may be reused when the call returns; status is a DEVICE array: status[i] = 0, or NXZ_CC_INVALID_OP for
 * src or dst NULL with len != 0, elem == 0 or elem > NXZ_SHUFFLE_ELEM_MAX, reserved != 0, or byte ranges that overlap (src == dst
 * included; ranges that only touch are taken).  A refused job leaves dst untouched and its neighbours unaffected.
 * On the device (power-gzip_amd/csrc/nxz_shuffle.hip, the rules in nxz_shuffle.h): one grid over the tiles of all jobs, whatever mix
 * of lengths -- the host's one pass writes the tile prefix into pinned staging of the stream's scratch, a workgroup finds its
 * (job, tile) there.  A tile is nxz_shuffle_tile_elems(elem) elements: the most that fit 16 KiB, rounded down to a multiple of 16.
 * It is transposed through LDS (20 KiB of planes and a 1 KiB table at the most), with loads and stores of 16 bytes a lane on 16-byte
 * boundaries and a byte-wise head and tail around them for every plane's run: dst + j * N has whatever alignment N leaves it.  elem 2,
 * 4, 8 and 16 run with the element size as a constant; every other size up to 256, the copies included, takes one generic path.
 * Asynchronous on `stream`: no host wait, no device allocation once the stream's scratch has grown, two launches whatever n is.
 * Returns 0; -EINVAL (ctx NULL, jobs or status NULL with n != 0); -ENODEV in a forked child; -E2BIG for n >= 2^31 (or 2^31 tiles:
 * 32 TiB); -ENOMEM when scratch cannot be had.  n == 0 returns 0 and launches nothing.
 * Not part of this call: the transpose fused into the LZ77 kernel's load or the inflate kernels' flush -- a pass of its own costs
 * two sweeps of memory beside a codec that runs at a few percent of memory bandwidth; bit-shuffle (Blosc's); in-place operation.
 * Speed (tools/bench_shuffle.py, profiles/r26_shuffle.txt; medians of 5 runs taken in turn, every route within 2.5 % of its median), as
 * the time of nxz_copy_device on the same total bytes.  4096 buffers of 1 MiB (copy 1.55 ms): shuffle 0.93 / 0.92 / 0.94 and unshuffle
 * 1.00 / 1.01 / 1.01 for elem 2 / 4 / 8 -- the pass is memory-bound, 2.5 to 2.8 TiB/s of source bytes; the generic path (elem 12) 1.28
 * and 2.64.  65 536 buffers of 64 KiB (copy 1.65 ms): 1.10 and 1.18 to 1.20 for elem 2 / 4 / 8, generic 1.63 and 3.02.  The generic
 * unshuffle gathers its 16 bytes a lane with a step from byte to byte that the constant paths do with a mask; it is the one form far
 * from the copy.  Beside the codec (1024 buffers of 1 MiB, zlib, DHTGEN, hist_max 0): shuffle + nxz_batch_deflate_streams against that
 * call alone takes 1.11 of the time and leaves 0.767 of the compressed bytes on float32 random walks (0.662 against 0.863 of the
 * source), 1.18 of the time and 0.916 of the bytes on bf16 N(0, 0.02) weights (0.715 against 0.780).  The pass itself is 0.4 ms of
 * those 1.0 and 1.5 ms; the rest is the codec on other bytes. */
#define NXZ_SHUFFLE_ELEM_MAX 256
typedef struct nxz_shuffle_job {      /* HOST array, as nxz_stream_job_t: may be reused when the call returns */
	const uint8_t *src;           /* DEVICE, any alignment */
	uint8_t       *dst;           /* DEVICE, any alignment, len bytes; must not overlap src */
	uint64_t       len;           /* any length, 0 included */
	uint32_t       elem;          /* element size in bytes, 1 .. NXZ_SHUFFLE_ELEM_MAX */
	uint32_t       reserved;      /* 0 */
} nxz_shuffle_job_t;
int nxz_batch_shuffle  (nxz_ctx_t *ctx, const nxz_shuffle_job_t *jobs /* HOST */, size_t n, uint32_t *status /* DEVICE, n */, void *stream);
int nxz_batch_unshuffle(nxz_ctx_t *ctx, const nxz_shuffle_job_t *jobs /* HOST */, size_t n, uint32_t *status /* DEVICE, n */, void *stream);
/* the elements a workgroup takes of a job with this element size (0 for an elem the calls refuse) */
uint32_t nxz_shuffle_tile_elems(uint32_t elem);

/* ------------------------------------------------------------------------
 * BGZF random access: the member index and batched range reads
 * ---------------------------------------------------------------------- */
/* The member index of a BGZF image in DEVICE memory (found as nxz_batch_unpack_gzip finds the members):
 * coff[j] / uoff[j] (DEVICE, max_members + 1) = compressed / uncompressed offset of member j; coff[L] = the
 * bytes of whole chained members (nxz_blocked_scan's `consumed`), uoff[L] = sum of ISIZE.  Empty members
 * (the end marker) are members: uoff may repeat.  Synchronous (one wait, for L).  Returns 0 and *members = L;
 * -EILSEQ: packed does not start with a member; -E2BIG: L > max_members (*members set, nothing written). */
int nxz_bgzf_index(nxz_ctx_t *ctx, const uint8_t *packed, uint64_t len, uint64_t *coff, uint64_t *uoff,
		   size_t max_members, uint64_t *members, void *stream);

typedef struct nxz_bgzf_range { uint64_t begin, end; } nxz_bgzf_range_t;      /* [begin, end) */
enum { NXZ_RANGE_UOFF = 0, NXZ_RANGE_VOFF = 1 };      /* ranges in uncompressed offsets / virtual offsets (coff << 16 | within) */
enum {
	NXZ_RANGE_OK = 0,
	NXZ_RANGE_OUT_OF_BOUNDS, /* begin > end, begin < uoff[0] or end > uoff[L] (after conversion): no bytes */
	NXZ_RANGE_BAD_VOFFSET,   /* voff >> 16 is no coff[j], or voff & 0xffff exceeds that member's ISIZE: no bytes */
	NXZ_RANGE_DAMAGED,       /* a member it touches failed its framed decode, or its ISIZE is not uoff[j+1] - uoff[j]: zeros */
	NXZ_RANGE_BAD_STREAM = 4 /* nxz_batch_checkpoint_read_ranges only: the range's job has no index row to read through: no bytes */
};

/* Reads n ranges of a BGZF image.  coff / uoff (DEVICE, nidx = members + 1 entries) is an index as nxz_bgzf_index
 * writes it, or a SLICE of one (entries i..i+k): packed then holds the image's bytes from coff[0] on (packed_len of
 * them), and ranges are in the index's absolute offsets.  ranges (DEVICE, n).
 *   uncompressed byte u lies in the last member j with uoff[j] <= u (upper_bound - 1; empty members hold nothing);
 *   a virtual offset needs voff >> 16 == coff[j] for some j <= L and voff & 0xffff <= ISIZE of j (== ISIZE: the
 *   member's end, as htslib allows); it stands for uoff[j] + (voff & 0xffff);
 *   an empty range is NXZ_RANGE_OK with no bytes; begin > end, begin < uoff[0], end > uoff[L] are OUT_OF_BOUNDS.
 * Range r's bytes go to dst + offsets[r] (offsets DEVICE, n + 1, written by the engine: the exclusive prefix sum of
 * the ranges' lengths, 0 for a range that is not OK); status[r] (DEVICE, NXZ_RANGE_*).  A DAMAGED range's bytes are
 * zero; the other ranges are unaffected.  Every member is decoded at most once per call, however many ranges touch
 * it (into a 16-byte aligned slot of per-stream scratch, in chunks of at most NXZ_BGZF_CHUNK members -- default
 * 16 384 -- and 1 GiB), then the pieces are copied to dst.
 * Before anything is decoded the device checks that the index describes the image: nxz_bgzf_member_size at every
 * coff[j] - coff[0] must be coff[j+1] - coff[j], and uoff must not decrease.  Synchronous.
 * Returns 0; -EILSEQ: the index does not describe the image (nothing written); -E2BIG: dst_cap is too small
 * (*out_len = the bytes needed; offsets and status written, dst not); -EINVAL.  *out_len = bytes of all ranges,
 * *decoded = members inflated (either may be NULL). */
int nxz_bgzf_read_ranges(nxz_ctx_t *ctx, const uint8_t *packed, uint64_t packed_len,
			 const uint64_t *coff, const uint64_t *uoff, uint64_t nidx,
			 int kind, const nxz_bgzf_range_t *ranges, size_t n,
			 uint8_t *dst, uint64_t dst_cap, uint64_t *offsets, uint32_t *status,
			 uint64_t *out_len, uint64_t *decoded, void *stream);

/* ------------------------------------------------------------------------
 * Checkpoints: an index into raw, zlib and gzip streams, and range reads through it
 * ---------------------------------------------------------------------- */
/* What the BGZF calls do for images cut into members, for any deflate stream: byte ranges out of the middle of a stream without
 * inflating what lies in front.  A checkpoint is a BLOCK HEADER of the deflate data: the bit of the job's src where the header
 * starts (framing included) and the bytes of output in front of it.  Checkpoints stand only at block headers -- a stream whose
 * blocks are huge has coarse segments.  The rules (power-gzip_amd/csrc/nxz_checkpoint.h):
 *   1. checkpoint 0 is the first block header: bit = 8 * the framing's header bytes, uoff = 0;
 *   2. a later header with u bytes of output in front of it is a checkpoint when u - (uoff of the last checkpoint) >= span;
 *   3. entry [count] is the sentinel: the bit behind the final end-of-block code, and out_len;
 *   4. segment k is checkpoint k up to entry k + 1: source bytes [cbit[k] >> 3, (cbit[k+1] + 7) >> 3), of the first of them the
 *      upper (8 - (cbit[k] & 7)) & 7 bits when cbit[k] stands inside a byte, a window of min(uoff[k], 32768) bytes,
 *      uoff[k+1] - uoff[k] bytes of output;
 *   5. an index is valid when uoff[0] == 0, cbit and uoff strictly increase over the checkpoints (the sentinel's uoff may equal the
 *      last checkpoint's: an empty final block), cbit[count] <= 8 * src_len, and every segment's window + source bytes and output
 *      fit 32 bits. */
enum { NXZ_CPS_OK = 0, NXZ_CPS_STREAM_FAILED, NXZ_CPS_MORE, NXZ_CPS_NO_OUTPUT, NXZ_CPS_INVALID };
typedef struct nxz_checkpoint_stream {   /* DEVICE, 32 bytes, one per job */
	uint32_t status, count;          /* NXZ_CPS_*; count: checkpoints found, may exceed cp_cap (0 for a stream that failed) */
	uint32_t format, hdr_len;        /* what the framing turned out to be: NXZ_FMT_RAW / _ZLIB / _GZIP, its header bytes */
	uint64_t out_len;                /* bytes the stream makes */
	uint32_t cc, frame_status;       /* why a failed stream failed: the raw decoder's code, NXZ_FRAME_* */
} nxz_checkpoint_stream_t;

/* The index build: one wavefront walks one job in ONE launch (power-gzip_amd/csrc/nxz_checkpoint.hip) -- the header by the parser
 * of the framed calls (fmt: NXZ_FMT_RAW, _ZLIB, _GZIP, _AUTO; raw has none), then the size walk of nxz_batch_decompress_size, which
 * reports every block header -- and writes cbit[i * (cp_cap + 1) + k] / uoff[...] for k < min(count, cp_cap), the sentinel at
 * [count] when count <= cp_cap, and streams[i].  Checkpoints beyond cp_cap are counted, not stored: NXZ_CPS_MORE with the true
 * count and no sentinel.  Of a gzip job the FIRST member is indexed (several members: jobs cut where nxz_batch_gzip_members_size
 * says).  A job with resume or hist_len set: NXZ_CPS_INVALID, nothing walked.  A stream that fails or does not reach the end of its
 * final block: NXZ_CPS_STREAM_FAILED with cc / frame_status, count = 0, its entries are not to be used.  The trailer's checksum is
 * not checked, as in the size calls.  A stream of more than 2^32 - 1 bytes of output fails with cc 13.
 * windows (DEVICE, n * cp_cap slots of 32768 bytes, or NULL): the window of every stored checkpoint k of job i -- the
 * min(uoff[k], 32768) bytes in front of uoff[k] -- copied to the START of slot i * cp_cap + k from jobs[i].dst, which must hold the
 * stream's decoded output (the caller has just made it with nxz_batch_decompress_framed: the index is the by-product of a decode
 * already done).  dst == NULL or dst_cap < out_len: NXZ_CPS_NO_OUTPUT, the positions are valid, that stream's windows are not
 * written.  With windows == NULL dst is never looked at.  Windows without the full output: nxz_batch_checkpoint_build below.
 * jobs, cbit, uoff, windows and streams are DEVICE arrays.  Asynchronous on `stream`: no host wait, no allocation beyond the
 * stream's scratch.  Returns 0 (n == 0 included); -EINVAL (ctx, fmt, span == 0, cp_cap == 0, n >= 2^31, a NULL array with n > 0);
 * -ENODEV in a forked child.
 * Speed: not measured yet; tools/bench_checkpoints.py writes profiles/r14_checkpoints.txt. */
int nxz_batch_checkpoint_index(nxz_ctx_t *ctx, int fmt /* RAW, ZLIB, GZIP, AUTO */, const nxz_batch_job_t *jobs, size_t n,
			       uint64_t span, uint32_t cp_cap,
			       uint64_t *cbit, uint64_t *uoff,   /* DEVICE, n * (cp_cap + 1) each */
			       uint8_t *windows,                 /* DEVICE, n * cp_cap * 32768, or NULL */
			       nxz_checkpoint_stream_t *streams, void *stream);

/* Reads n ranges of ONE stream through its index: the counterpart of nxz_bgzf_read_ranges, with segments for members.  src
 * (DEVICE, src_len bytes) is the job's src, framing included; cbit / uoff (DEVICE, nidx = count + 1 entries) and windows (DEVICE,
 * count slots of 32768 bytes; may be NULL for an index of one segment) are one job's part of what nxz_batch_checkpoint_index
 * wrote.  ranges (DEVICE, n) are uncompressed offsets [begin, end) -- only NXZ_RANGE_UOFF exists here --, mapped onto segments by
 * the rule of the BGZF call; empty ranges, begin > end, end > out_len, offsets, status, dst_cap, *out_len and -E2BIG behave
 * exactly as there.  Every segment is decoded at most once per call, however many ranges touch it: [window][source bytes] is
 * staged into a 16-byte aligned slot of per-stream scratch and goes through nxz_batch_decompress as a job with hist_len = the
 * window and resume = in_subc << 20, into a slot of exactly the segment's output, in chunks of at most NXZ_BGZF_CHUNK segments
 * and 1 GiB; a larger segment goes alone.  A segment is good when the decoder made exactly its output and ended with CC 0 or
 * CC 3 (it runs out of source in front of the next header); a range that touches a segment that is not good is
 * NXZ_RANGE_DAMAGED and reads as zeros, the other ranges are unaffected.
 * Before anything is decoded the device checks the index against rule 5: a stale or foreign index never makes a kernel read
 * outside src or a window slot.  Synchronous.
 * Returns 0; -EILSEQ: the index is not valid (nothing written); -E2BIG; -EINVAL; -ENOMEM; -ENODEV in a forked child.
 * *out_len = bytes of all ranges, *decoded = segments inflated (either may be NULL).
 * Speed: not measured yet (segments go a stream per wavefront: the workgroup kernel hands back jobs with history);
 * tools/bench_checkpoints.py writes profiles/r14_checkpoints.txt. */
int nxz_checkpoint_read_ranges(nxz_ctx_t *ctx, const uint8_t *src, uint64_t src_len,
			       const uint64_t *cbit, const uint64_t *uoff, const uint8_t *windows, uint64_t nidx /* count + 1 */,
			       const nxz_bgzf_range_t *ranges, size_t n,          /* uncompressed offsets, [begin, end) */
			       uint8_t *dst, uint64_t dst_cap, uint64_t *offsets, uint32_t *status,   /* NXZ_RANGE_* */
			       uint64_t *out_len, uint64_t *decoded, void *stream);

/* ------------------------------------------------------------------------
 * Checkpoints inside blocks: a fine index and range reads through it
 * ---------------------------------------------------------------------- */
/* The two calls above cut a stream where whoever compressed it ended a block: a hardware compressor's output, a PNG IDAT or a
 * short Z_FIXED stream can be ONE block and gets ONE checkpoint, and zlib's own blocks run to hundreds of KiB of output (its Z_FIXED
 * stream of 64 MiB of text has 377).  These two cut a stream every `span` bytes of output, inside blocks:
 * a checkpoint stands in front of a TOKEN, and a 16-byte state entry beside cbit / uoff says where in a block that is.  The rules
 * (power-gzip_amd/csrc/nxz_checkpoint_fine.h, on top of nxz_checkpoint.h's rules 3 - 5, which hold as they stand):
 *   1. checkpoint 0 is the first block header, state all zero;
 *   2. tokens are a literal (1 byte), a match (len bytes) and every single byte of a stored block; end-of-block codes and headers
 *      make no bytes.  With c the uoff of the last checkpoint and u bytes of output in front of a token of n bytes: when
 *      u + n > c + span a checkpoint stands IN FRONT OF that token -- cbit the bit of src where it starts, uoff = u -- and c = u;
 *   3. a stored run so splits at exactly c + span bytes: cbit is a byte boundary, rem (1..65535) the bytes of the block to come;
 *   4. an end-of-block code and the next header between the last token that fits and the one that does not: the checkpoint stands
 *      behind that header, in the new block, with the new block's state;
 *   5. span >= 258: a token always fits an empty segment, uoff strictly increases, every segment but the last makes between
 *      span - 257 and span bytes.
 * This is where a chain of nxz_batch_decompress jobs with NXZ_JOB_SUSPEND_WHEN_FULL and dst_cap = span suspends. */
typedef struct nxz_checkpoint_state {   /* DEVICE, 16 bytes, beside cbit / uoff: n * (cp_cap + 1), the sentinel's all zero */
	uint64_t tbit;     /* dynamic block: the bit of src where the block's table starts (HLIT; header bit + 3), else 0 */
	uint32_t resume;   /* in_rembytecnt | in_sfbt << 16 as nxz_batch_job_t.resume wants them, WITHOUT in_subc; 0: at a block header.
			    * in_sfbt: 0x8 | BFINAL stored (with rem), 0xa | BFINAL fixed, 0xc | BFINAL dynamic */
	uint32_t dhtlen;   /* dynamic block: bits of the table, else 0 */
} nxz_checkpoint_state_t;

/* nxz_batch_checkpoint_index with the rules above (power-gzip_amd/csrc/nxz_checkpoint_fine.hip: the same single launch, the size
 * walk with a budget of span bytes a segment), and state[i * (cp_cap + 1) + k] beside cbit / uoff.  The table of a dynamic block
 * is not copied into the index: its position in src is enough, the source is there at read time.  Everything else -- fmt, the
 * first member of a gzip job, streams[i] and the NXZ_CPS_* outcomes, cp_cap and the sentinel, windows (the same copy from
 * jobs[i].dst), the 2^32 - 1 limit, asynchrony -- is that call's.  -EINVAL also for span < 258 and state == NULL with n > 0.
 * Speed (profiles/r15_checkpoints_fine.txt, MI355X): the index takes 0.97 - 0.98 of the coarse index's time on 64 zlib -6 streams of
 * 16 MiB; through it a 4 KiB read from the middle of a 64 MiB Z_FIXED stream (zlib's: 377 blocks) takes 3.9 ms against 10.6 ms
 * through the coarse index, the whole stream 5.1 ms against 11.6 ms; with the same tokens as ONE block, 4.0 ms against 138 ms and
 * 5.0 ms against 138 ms. */
int nxz_batch_checkpoint_index_fine(nxz_ctx_t *ctx, int fmt /* RAW, ZLIB, GZIP, AUTO */, const nxz_batch_job_t *jobs, size_t n,
				    uint64_t span /* >= 258 */, uint32_t cp_cap,
				    uint64_t *cbit, uint64_t *uoff, nxz_checkpoint_state_t *state,   /* DEVICE, n * (cp_cap + 1) each */
				    uint8_t *windows,                 /* DEVICE, n * cp_cap * 32768, or NULL */
				    nxz_checkpoint_stream_t *streams, void *stream);

/* The index AND its windows from the source alone, in ONE pass (power-gzip_amd/csrc/nxz_checkpoint_build.hip; the ring's rules in
 * nxz_checkpoint_build.h): what zran and indexed_gzip do on a CPU.  The two calls above copy their windows out of jobs[i].dst, which
 * must hold the whole decoded output; this one never looks at jobs[i].dst or dst_cap.  It is the same walk -- one job per wavefront,
 * the long jobs first -- with every token applied to a ring of the last 32 KiB of output in LDS (stored runs are read from src), and
 * the ring is written to a checkpoint's slot where the checkpoint is stored.
 * state != NULL: cbit, uoff, state and streams[i] are exactly what nxz_batch_checkpoint_index_fine writes for a job whose dst holds the
 * full output (span >= 258); state == NULL: checkpoints at block headers only, exactly what nxz_batch_checkpoint_index writes (any
 * span >= 1).  The rules, the sentinel, NXZ_CPS_MORE with the true count (the walk goes on to the end of the stream), NXZ_CPS_STREAM_FAILED
 * with cc / frame_status, NXZ_CPS_INVALID for resume / hist_len, the first member of a gzip job, the 2^32 - 1 limit and the trailer's
 * checksum that is not looked at are those calls'.  NXZ_CPS_NO_OUTPUT cannot occur.
 * windows (DEVICE, n * cp_cap slots of 32768 bytes, required): for every stored checkpoint k of a stream that ends NXZ_CPS_OK or
 * NXZ_CPS_MORE the first min(uoff[k], 32768) bytes of slot i * cp_cap + k are the bytes of output in front of uoff[k] -- the bytes the
 * calls above copy.  The rest of the slot and the slots beyond the stored checkpoints are not written.  Of a stream that fails, the
 * slots of checkpoints passed before the failure may have been written: their contents are unspecified, as its cbit entries are;
 * nothing outside that job's own cp_cap slots is touched.  src and windows may have any alignment (a 16-byte aligned slot gets
 * 16-byte stores).
 * Asynchronous on `stream`: no host wait, no allocation beyond the stream's scratch (the by-length launch order).  Returns 0 (n == 0
 * included); -EINVAL (ctx, fmt, span == 0, span < 258 with state, cp_cap == 0, n >= 2^31, jobs / cbit / uoff / windows / streams
 * NULL with n > 0); -ENODEV in a forked child.
 * Not part of this call: checking the trailer's checksum (nxz_batch_decompress_verify_framed does, also without a target); indexing one stream in several calls; compressing the windows; parallelism
 * inside one stream (one job is one wavefront's serial decode, as one job is one wavefront's serial walk above).
 * Speed (profiles/r17_checkpoint_build.txt, MI355X), against nxz_batch_decompress_framed into a full target plus
 * nxz_batch_checkpoint_index_fine with windows: 1.71 of that route's time on 64 zlib -6 streams of 16 MiB (897 ms against 525 ms) and
 * 2.7 on 4096 streams of 1 MiB (233 ms against 87 ms), with 0.32 - 0.36 of its device memory at a span of 64 KiB and 0.04 - 0.09 at
 * 1 MiB (4096 x 1 MiB: 2.3 GiB against 6.3 GiB, 0.4 GiB against 4.4 GiB).  The decode route is the faster one where its target fits. */
int nxz_batch_checkpoint_build(nxz_ctx_t *ctx, int fmt /* RAW, ZLIB, GZIP, AUTO */, const nxz_batch_job_t *jobs, size_t n,
			       uint64_t span, uint32_t cp_cap,
			       uint64_t *cbit, uint64_t *uoff,        /* DEVICE, n * (cp_cap + 1) each */
			       nxz_checkpoint_state_t *state,         /* DEVICE, n * (cp_cap + 1), or NULL: checkpoints at block headers only */
			       uint8_t *windows,                      /* DEVICE, n * cp_cap * 32768: required */
			       nxz_checkpoint_stream_t *streams, void *stream);

/* nxz_checkpoint_read_ranges through a fine index: state (DEVICE, nidx entries) is the job's part of what the call above wrote.
 * A segment's job is the coarse call's with resume = state.resume | in_subc << 20, NXZ_JOB_SUSPEND_WHEN_FULL, a target of exactly
 * the segment's output and, inside a dynamic block, the table -- bits [tbit, tbit + dhtlen) of src shifted to bit 0 -- in a
 * nxz_batch_dht_t slot of per-stream scratch that goes to nxz_batch_decompress as dht_io.  The segment's source ends with the byte
 * that holds cbit[k + 1]; a short token whole inside the real bits behind that boundary does not fit the target and is a place to
 * suspend (CC 3), a cut token runs out of source (CC 3).  A segment is good as there: CC 0 or CC 3 and exactly its bytes.
 * The index check adds, per entry: entry 0 has resume 0; resume has bits in 0..19 only; in_sfbt is 0 or 0x8..0xd; stored: rem in
 * 1..65535 and cbit % 8 == 0, else rem 0; dynamic: 1 <= dhtlen <= 8 * NXZ_DHT_MAXSZ, tbit >= 3, tbit + dhtlen <= cbit, else
 * tbit = dhtlen = 0 -- a stale or foreign index never makes a kernel read outside src, a window slot or a table slot (-EILSEQ).
 * A state array of zeros over a coarse index reads exactly what nxz_checkpoint_read_ranges reads.  Everything else is that call's. */
int nxz_checkpoint_read_ranges_fine(nxz_ctx_t *ctx, const uint8_t *src, uint64_t src_len,
				    const uint64_t *cbit, const uint64_t *uoff, const nxz_checkpoint_state_t *state, const uint8_t *windows,
				    uint64_t nidx /* count + 1 */, const nxz_bgzf_range_t *ranges, size_t n,
				    uint8_t *dst, uint64_t dst_cap, uint64_t *offsets, uint32_t *status,   /* NXZ_RANGE_* */
				    uint64_t *out_len, uint64_t *decoded, void *stream);

/* ------------------------------------------------------------------------
 * Batched range reads: ranges across all the streams of an indexed batch, in one call
 * ---------------------------------------------------------------------- */
/* The three index calls take n jobs and write n rows; the two readers above take ONE row and wait for the host twice a call.  This
 * call takes the batch's index as the index calls wrote it -- thousands of resident shards, a few records wanted from each -- and
 * reads ranges of any of its streams: one map, one decode batch over the segments of all streams, the same two waits for the whole
 * batch (power-gzip_amd/csrc/nxz_checkpoint_batch.hip; the rules in nxz_checkpoint_batch.h).
 * jobs (DEVICE, n_jobs) is the array the index call was given: src and src_len are read, dst is not.  cbit / uoff (DEVICE,
 * n_jobs * (cp_cap + 1)), state (the same, or NULL: a coarse index), windows (DEVICE, n_jobs * cp_cap slots of 32768 bytes) and
 * streams (DEVICE, n_jobs) are what nxz_batch_checkpoint_index / _index_fine / _build wrote, with the same cp_cap.
 * Per range: ranges[r] = (job, begin, end) reads [begin, end) of the uncompressed bytes of stream `job` exactly as
 * nxz_checkpoint_read_ranges (state == NULL) / nxz_checkpoint_read_ranges_fine (state) reads it through row `job`: the same
 * upper-bound rule onto segments; an empty range is NXZ_RANGE_OK with no bytes; begin > end or end > out_len (the row's sentinel
 * uoff) is NXZ_RANGE_OUT_OF_BOUNDS; a range that touches a segment that is not good is NXZ_RANGE_DAMAGED and reads as zeros.
 * offsets (DEVICE, n + 1) is the exclusive prefix sum of the OK ranges' lengths in the order of `ranges`; ranges may name jobs in any
 * order, and any number of them the same job.  Every segment of every stream is decoded at most once per call, however many ranges
 * touch it; *decoded = the distinct segments inflated over the whole batch.
 * A stream's validity is that stream's alone: a range is NXZ_RANGE_BAD_STREAM (no bytes, length 0 in offsets) when job >= n_jobs,
 * streams[job].status != NXZ_CPS_OK, streams[job].count is 0 or exceeds cp_cap, jobs[job].src is NULL, the row fails rule 5 against
 * jobs[job].src_len or, with state, a per-entry check listed at nxz_checkpoint_read_ranges_fine.  Ranges of other streams are
 * unaffected, and this call never returns -EILSEQ: one stale row does not cost a caller the others.  The single-stream calls'
 * guarantee holds row by row: a stale or foreign row never makes a kernel read outside that job's src, its own cp_cap window slots
 * or a table slot.  (Every row is checked, named by a range or not: a thread an entry.)
 * state == NULL reads exactly what a state array of zeros reads.  With state a segment's job is the fine reader's: resume =
 * state.resume | in_subc << 20, NXZ_JOB_SUSPEND_WHEN_FULL, a target of exactly the segment's output and, inside a dynamic block, the
 * table -- bits [tbit, tbit + dhtlen) of that job's src -- in a nxz_batch_dht_t slot.  Segments are staged as [window][source bytes]
 * and go through nxz_batch_decompress as one batch over all streams, in chunks of at most NXZ_BGZF_CHUNK segments and 1 GiB; a chunk
 * may hold segments of many streams.
 * Synchronous: the two waits of the single-stream call, once.  Returns 0 (n == 0 or n_jobs == 0 included: *out_len = 0, and with
 * n_jobs == 0 every range is NXZ_RANGE_BAD_STREAM); -E2BIG, *out_len and dst == NULL sizing exactly as there (offsets and status
 * written, dst not); -EINVAL: ctx, cbit, uoff, windows, streams or offsets NULL, jobs NULL with n_jobs > 0, cp_cap == 0,
 * n_jobs >= 2^31, n >= 2^31, n_jobs * (cp_cap + 1) >= 2^32, ranges or status NULL with n > 0; -ENODEV in a forked child; -ENOMEM
 * when scratch cannot be had.
 * Not part of this call: BGZF images (nxz_bgzf_read_ranges stays single-image); multi-member gzip jobs (the first member is what the
 * index holds); an asynchronous form.
 * Speed (profiles/r22_checkpoint_batch.txt, MI355X; tools/bench_checkpoint_batch.py), against the loop of nxz_checkpoint_read_ranges_fine
 * calls over the same ranges, one 4 KiB range a stream: 0.017 of the loop's time on 64 zlib -6 streams of 16 MiB (4.1 ms against 240 ms
 * at a span of 64 KiB, 61 ms against 3.7 s at 1 MiB) and 0.001 - 0.004 on 4096 streams of 1 MiB (7.9 ms against 15.4 s, 41 ms against
 * 10.5 s); the whole stream as the range, 4096 x 1 MiB: 0.004 - 0.006 (95 ms against 16.6 s, 42 ms against 10.5 s: 42 and 95 GiB/s of
 * output).  The batched call is slower at none of these points. */
typedef struct nxz_batch_range {     /* DEVICE, 24 bytes */
	uint32_t job;                /* row of the index: 0 .. n_jobs - 1 */
	uint32_t reserved;           /* 0 */
	uint64_t begin, end;         /* uncompressed offsets of that stream, [begin, end) */
} nxz_batch_range_t;
int nxz_batch_checkpoint_read_ranges(nxz_ctx_t *ctx, const nxz_batch_job_t *jobs, size_t n_jobs, uint32_t cp_cap,
				     const uint64_t *cbit, const uint64_t *uoff,          /* DEVICE, n_jobs * (cp_cap + 1) each */
				     const nxz_checkpoint_state_t *state,                 /* DEVICE, n_jobs * (cp_cap + 1), or NULL: a coarse index */
				     const uint8_t *windows,                              /* DEVICE, n_jobs * cp_cap * 32768 */
				     const nxz_checkpoint_stream_t *streams,              /* DEVICE, n_jobs */
				     const nxz_batch_range_t *ranges, size_t n,           /* DEVICE */
				     uint8_t *dst, uint64_t dst_cap, uint64_t *offsets /* n + 1 */, uint32_t *status /* n, NXZ_RANGE_* */,
				     uint64_t *out_len, uint64_t *decoded, void *stream);

/* Device memory, pinned host memory, streams and asynchronous copies, for callers that hold
 * host buffers and do not link the HIP runtime themselves.  A stream made here is passed as
 * the `stream` argument of the batch calls; nxz_stream_destroy also releases the per-stream
 * scratch the batch calls keep. */
void *nxz_dev_malloc(nxz_ctx_t *ctx, size_t bytes);
void  nxz_dev_free(nxz_ctx_t *ctx, void *p);
void *nxz_pinned_malloc(nxz_ctx_t *ctx, size_t bytes);
void  nxz_pinned_free(nxz_ctx_t *ctx, void *p);
void *nxz_stream_create(nxz_ctx_t *ctx);
void  nxz_stream_destroy(nxz_ctx_t *ctx, void *stream);
int   nxz_copy_to_device(nxz_ctx_t *ctx, void *dst_dev, const void *src_host, size_t bytes, void *stream);
int   nxz_copy_to_host(nxz_ctx_t *ctx, void *dst_host, const void *src_dev, size_t bytes, void *stream);
/* Measurement aid: a device-to-device copy by a 16-bytes-a-lane kernel (what the roofline's measured HBM peak is taken with);
 * bytes a multiple of 16, both pointers 16-byte aligned; asynchronous on `stream`. */
int   nxz_copy_device(nxz_ctx_t *ctx, void *dst_dev, const void *src_dev, size_t bytes, void *stream);

/* Measurement aid (bench.py's roofline): with timing on, every compress batch records events
 * around its kernels; nxz_ctx_stage_ms waits for them and returns the milliseconds spent in the
 * LZ77, table generator and entropy kernels since the last call, and how many launches of each. */
void nxz_ctx_stage_timing(nxz_ctx_t *ctx, int on);
int  nxz_ctx_stage_ms(nxz_ctx_t *ctx, double ms[3], unsigned *launches);
/* Measurement aid: of the last nxz_batch_decompress of n streams on `stream` that went a stream per lane, how many
 * streams the fixed-code-only kernel handed back to the general one (waits for the stream; -ENOENT: no such batch). */
int  nxz_ctx_lanes_handed_back(nxz_ctx_t *ctx, void *stream, size_t n, uint32_t *count);
/* Measurement aid: of the last nxz_batch_decompress on `stream` that went a stream per workgroup (nxz_inflate_wg.hip), how many
 * streams that kernel handed back to the stream-per-wavefront kernel (out16[15]) and why (out16[1..10]: the job's fields, a block
 * header, a stored block, a dynamic table, its sub-tables, too many rounds, no end-of-block, a bad token, no room, a bad distance);
 * waits for the stream; -ENOENT: no such batch. */
int  nxz_ctx_wg_reasons(nxz_ctx_t *ctx, void *stream, uint32_t *out16);
/* ... and, for a batch run with NXZ_WG_PROF=1, the cycles of one lane by phase and the counts (12 words: load, block headers, tables, first
 * pass, later rounds, writing pass, matches, out; rounds, streams, coded blocks, pieces) */
int  nxz_ctx_wg_prof(nxz_ctx_t *ctx, void *stream, unsigned long long *out12);

/* Block until everything queued on `stream` by this context has finished. */
int nxz_ctx_sync(nxz_ctx_t *ctx, void *stream);

/* Worst-case compressed size the engine needs as dst_cap for `src_len`
 * source bytes (fixed-Huffman literals are 9 bits, + header/EOB + 16-byte
 * store granularity). */
size_t nxz_compress_bound(size_t src_len);

/* 0 in a process that was forked after a context was created (the HIP runtime does not survive
 * fork(); such a child gets ENODEV / CC 254 from every entry point and should use software zlib,
 * which is what libnxz_preload.so does), else 1. */
int nxz_engine_usable(void);

/* Library version string. */
const char *nxz_engine_version(void);

#ifdef __cplusplus
}
#endif
#endif /* NXZ_ENGINE_H */
