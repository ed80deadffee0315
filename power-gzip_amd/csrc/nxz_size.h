// nxz_size.h -- the rules of the output-size query (nxz_batch_decompress_size, include/nxz_engine.h) as plain code that compiles
// for the device (nxz_inflate_size.hip: the walk that counts what a stream would produce) and for the host (tests/native/size_host.cpp).
//
// The walk decides three things by arithmetic alone, and they are here so that the kernel and a host program run the same code:
//   fit        a token of `len` bytes behind `produced` bytes of output still fits a target of dst_cap bytes.  Both are 32-bit
//              fields and dst_cap may be 0xffffffff ("no limit"): the sum is taken in 64 bits, it must not wrap;
//   distance   a match may reach `produced + hist` bytes back: what the stream made so far and the history the job declares
//              (jobs[i].hist_len, at most 32768; the size query reads none of those bytes);
//   the record what goes into nxz_batch_result_t at each kind of stop, field for field what nxz_batch_decompress writes
//              (oracle/nxz_inflate.c), with crc = adler = 0: the walk sees no output bytes.
#ifndef NXZ_SIZE_H
#define NXZ_SIZE_H
#include <stdint.h>
#include "../../include/nxz_engine.h"

#if defined(__HIPCC__)
#define NXZ_SIZE_HD __host__ __device__
#else
#define NXZ_SIZE_HD
#endif

#define NXZ_SIZE_WINDOW 32768u

/* a job the size query takes: fresh (no resume state), a history no longer than the window */
NXZ_SIZE_HD inline bool nxz_size_job_ok(uint32_t resume, uint32_t hist_len) { return resume == 0 && hist_len <= NXZ_SIZE_WINDOW; }
/* the bytes in front of the stream in jobs[i].src that are history: skipped, never read */
NXZ_SIZE_HD inline uint32_t nxz_size_hist_bytes(uint32_t hist_len, uint32_t src_len) { return hist_len < src_len ? hist_len : src_len; }

NXZ_SIZE_HD inline bool nxz_size_fits(uint32_t produced, uint32_t len, uint32_t dst_cap) { return (uint64_t)produced + len <= dst_cap; }
NXZ_SIZE_HD inline bool nxz_size_dist_ok(uint32_t dist, uint64_t produced, uint32_t hist) { return dist <= produced + hist; }

/* the record of a job that was refused: NXZ_CC_INVALID_OP, every other field 0 */
NXZ_SIZE_HD inline nxz_batch_result_t nxz_size_refused(void)
{
	nxz_batch_result_t r = {};
	r.cc = NXZ_CC_INVALID_OP;
	return r;
}

/* Where the walk stopped.  cc: 0, or the error met (NXZ_CC_TARGET_SPACE, _MISSING_CODE, _INVALID_DIST, _INVALID_DHT).  With cc 0:
 * final_eob -- behind the end-of-block code of the final block, subc = the bits of the source behind it; else the source ran
 * out: sfbt = where (1000 stored, 1010 fixed, 1100 dynamic, 1110 header; bit 0 BFINAL), subc = the bits from the start of the
 * token or header that could not be finished, rem = the bytes of a stored block still to come, dhtbits = the length of the
 * dynamic block's table when one was read (have_dht). */
typedef struct nxz_size_stop {
	uint32_t cc, final_eob, produced, sfbt, subc, rem, have_dht, dhtbits;
} nxz_size_stop_t;

NXZ_SIZE_HD inline nxz_batch_result_t nxz_size_record(const nxz_size_stop_t *s, uint32_t src_len)
{
	nxz_batch_result_t r = {};
	uint32_t cc = s->cc, spbc = src_len, subc = s->subc;
	if (s->final_eob && subc > 0xfff8) {               /* 16-bit SUBC: whole excess bytes stay unread */
		const uint32_t drop = (subc - 0xfff8 + 7) / 8;
		spbc -= drop; subc -= drop * 8;
	}
	if (cc == NXZ_CC_OK && !(s->final_eob && subc < 8)) cc = NXZ_CC_DATA_LENGTH;
	r.cc = cc;
	r.tpbc = (cc == NXZ_CC_OK || cc == NXZ_CC_DATA_LENGTH) ? s->produced : 0;
	r.tebc = s->rem;
	r.spbc = spbc;
	r.subc = subc;
	r.sfbt = s->sfbt | (s->final_eob ? 0x100u : 0) | (((s->sfbt & 0xe) == 0xc && s->have_dht) ? s->dhtbits << 16 : 0);
	return r;
}
#endif
