// nxz_inflate_part.h -- the rules of nxz_batch_inflate_streams_part (include/nxz_engine.h: a stream read in parts, a device buffer a
// part) as plain code that compiles for the device (nxz_inflate_part.hip), for the engine's host side (nxz_batch_streams.cpp) and for a
// host test program (tests/native/inflate_part_host.cpp).  Every function works on the carry record where it lies (704 bytes: never
// a copy).  The field rules of the headers and the trailer's comparison are nxz_frame.h's; here is what a stream in parts adds:
//
//   the refusals       a part that is not taken: dst and the carry stay as they are;
//   the start          what NXZ_PART_FIRST makes of a carry;
//   the header         nxz_frame_parse's walk a byte at a time: which field the next byte belongs to, the bytes left of FEXTRA or
//                      DICTID, the running header CRC -- a header of any length may be cut anywhere and needs no tail;
//   the slot           [window][tail][the part from the deflate data's first byte], how long it is and how much room the host,
//                      which cannot see the carry, sets aside for it;
//   the job            the raw decode's job and table slot from the carry;
//   the close          the decode's result and table slot back into the carry and the part's result: the tail rule, in_used, status;
//   the trailer        its bytes collected in the tail, the check when the last one is there.
#ifndef NXZ_INFLATE_PART_H
#define NXZ_INFLATE_PART_H
#include "nxz_frame.h"

#define NXZ_INFLATE_PART_WINDOW 32768u
#define NXZ_INFLATE_PART_CHUNK_STREAMS 16384u              /* a chunk's decode is one raw batch: below every size that samples the batch or goes a stream per lane (nxz_batch.cpp holds it against NXZ_LANES_MIN) */
#define NXZ_INFLATE_PART_SCRATCH_DEFAULT (512ull << 20)   /* NXZ_INFLATE_PART_SCRATCH */

/* (a copy loop a thread runs stays a loop: unrolled, it holds every word in a register at once) */
#if defined(__HIPCC__)
#define NXZ_IP_LOOP _Pragma("unroll 1")
#else
#define NXZ_IP_LOOP
#endif
/* a table's 288 bytes, word by word (both ends 4-byte aligned) */
NXZ_HD inline void nxz_inflate_part_copy_table(uint8_t *to, const uint8_t *from)
{
	NXZ_IP_LOOP
	for (uint32_t k = 0; k < NXZ_DHT_MAXSZ / 4; k++) ((uint32_t *)to)[k] = ((const uint32_t *)from)[k];
}

/* where the header's state machine stands: 0 .. 9 the fixed bytes (zlib: 0 CMF, 1 FLG), then the optional fields */
enum { NXZ_IPH_XLEN0 = 10, NXZ_IPH_XLEN1, NXZ_IPH_EXTRA, NXZ_IPH_NAME, NXZ_IPH_COMMENT, NXZ_IPH_HCRC0, NXZ_IPH_HCRC1, NXZ_IPH_ZDICT };
/* what a header byte did */
enum { NXZ_IPH_MORE = 0, NXZ_IPH_COMPLETE, NXZ_IPH_FAILED };

/* ---- the refusals: 0, or the completion code of a part that is not taken.  phase, tail_len: the incoming carry's (looked at without
 * FIRST only; a record that was never started holds anything: a tail longer than a tail can be is no stream's) ---- */
NXZ_HD inline uint32_t nxz_inflate_part_refusal(const nxz_inflate_part_job_t *j, uint32_t phase, uint32_t tail_len)
{
	if ((!j->src && j->src_len) || (!j->dst && j->dst_cap) || (!j->prev && j->prev_len) || (j->flags & ~(uint32_t)NXZ_PART_FIRST) ||
	    ((j->flags & NXZ_PART_FIRST) && j->prev_len))
		return NXZ_CC_INVALID_OP;
	if (!(j->flags & NXZ_PART_FIRST) && (phase >= NXZ_INFLATE_PHASE_DONE || tail_len > NXZ_INFLATE_PART_TAIL)) return NXZ_CC_INVALID_OP;
	return 0;
}
/* (the host's view: everything but the carry) */
NXZ_HD inline bool nxz_inflate_part_fmt_ok(int fmt) { return fmt == NXZ_FMT_RAW || fmt == NXZ_FMT_ZLIB || fmt == NXZ_FMT_GZIP || fmt == NXZ_FMT_AUTO; }

/* ---- the start: a fresh stream (the table and the tail hold nothing that counts) ---- */
NXZ_HD inline void nxz_inflate_part_start(nxz_inflate_carry_t *c, int fmt)
{
	c->phase = fmt == NXZ_FMT_RAW ? NXZ_INFLATE_PHASE_BODY : NXZ_INFLATE_PHASE_HEADER;
	c->hpos = 0; c->hleft = 0; c->hcrc = 0xffffffffu; c->hfirst = 0;
	c->frame = nxz_batch_frame_t();
	c->frame.format = fmt == NXZ_FMT_GZIP ? (uint32_t)NXZ_FMT_GZIP : fmt == NXZ_FMT_RAW ? (uint32_t)NXZ_FMT_RAW : (uint32_t)NXZ_FMT_ZLIB;   /* (AUTO: zlib until the magic is seen) */
	c->sfbt = c->rem = c->dhtlen = c->subc = 0;
	c->crc = 0; c->adler = 1;
	c->parts = 0; c->tail_len = 0;
	c->reserved[0] = c->reserved[1] = 0;
	c->total_in = c->total_out = 0;
}

/* ---- the header ---- */
NXZ_HD inline uint32_t nxz_inflate_part_header_fail(nxz_inflate_carry_t *c, uint32_t st)
{
	c->frame.status = st;
	c->frame.hdr_len = st == NXZ_FRAME_NEED_DICT ? 6 : 0;             /* (as nxz_frame_parse leaves it) */
	c->phase = NXZ_INFLATE_PHASE_FAILED;
	return NXZ_IPH_FAILED;
}
/* the field behind stage k of a gzip header (0 the fixed bytes, 1 FEXTRA, 2 FNAME, 3 FCOMMENT); frame.hdr_len: the bytes so far */
NXZ_HD inline uint32_t nxz_inflate_part_header_next(nxz_inflate_carry_t *c, uint32_t k)
{
	nxz_batch_frame_t *const f = &c->frame;
	const uint32_t flg = f->flg;
	if (k < 1 && (flg & 4)) { c->hpos = NXZ_IPH_XLEN0; return NXZ_IPH_MORE; }
	if (k < 2 && (flg & 8)) { c->hpos = NXZ_IPH_NAME; f->name_off = f->hdr_len; return NXZ_IPH_MORE; }
	if (k < 3 && (flg & 16)) { c->hpos = NXZ_IPH_COMMENT; f->comment_off = f->hdr_len; return NXZ_IPH_MORE; }
	if (flg & 2) { c->hpos = NXZ_IPH_HCRC0; return NXZ_IPH_MORE; }
	f->status = NXZ_FRAME_OK;
	c->phase = NXZ_INFLATE_PHASE_BODY;
	return NXZ_IPH_COMPLETE;
}
/* one byte of the header (phase HEADER): NXZ_IPH_MORE, or _COMPLETE (phase BODY: the next byte is deflate data), or _FAILED (phase
 * FAILED, frame.status says why) */
NXZ_HD inline uint32_t nxz_inflate_part_header_byte(nxz_inflate_carry_t *c, int fmt, uint32_t b)
{
	nxz_batch_frame_t *const f = &c->frame;
	const uint32_t n = f->hdr_len, pos = c->hpos;                     /* n: the bytes in front of this one */
	uint32_t st = NXZ_FRAME_OK, stage = 4;                            /* a fault; < 4: this byte ends stage `stage` of a gzip header */
	bool complete = false;
	f->hdr_len = n + 1;
	if (pos != NXZ_IPH_HCRC0 && pos != NXZ_IPH_HCRC1) c->hcrc = nxz_crc_step(c->hcrc, b);
	if (n == 0) c->hfirst = b;
	if (n == 1 && fmt == NXZ_FMT_AUTO && nxz_gzip_magic(c->hfirst, b)) f->format = NXZ_FMT_GZIP;
	if (f->format != NXZ_FMT_GZIP) {
		if (pos == NXZ_IPH_ZDICT) {
			f->dictid = f->dictid << 8 | b;
			if (--c->hleft == 0) st = NXZ_FRAME_NEED_DICT;
		} else if (n == 0) c->hpos = 1;
		else {
			f->flg = (uint8_t)b; f->cinfo = (uint8_t)(c->hfirst >> 4);
			const uint32_t z = nxz_zlib_header_status(c->hfirst, b);
			if (z == NXZ_FRAME_NEED_DICT) { c->hpos = NXZ_IPH_ZDICT; c->hleft = 4; }
			else if (z != NXZ_FRAME_OK) st = z;
			else complete = true;
		}
	} else if (n < 10) {
		c->hpos = n + 1;
		if (n == 3) f->flg = (uint8_t)b;
		if (n < 4) st = nxz_gzip_fixed_status(n, b);                    /* (AUTO: bytes 0 and 1 are the magic, or this is no gzip stream) */
		else if (n < 8) f->mtime |= b << (8 * (n - 4));
		else if (n == 8) f->xfl = (uint8_t)b;
		else { f->os = (uint8_t)b; stage = 0; }
	} else if (pos == NXZ_IPH_XLEN0) { f->extra_len = b; c->hpos = NXZ_IPH_XLEN1; }
	else if (pos == NXZ_IPH_XLEN1) {
		f->extra_len |= b << 8; f->extra_off = n + 1;
		c->hleft = f->extra_len; c->hpos = NXZ_IPH_EXTRA;
		if (!c->hleft) stage = 1;
	} else if (pos == NXZ_IPH_EXTRA) { if (--c->hleft == 0) stage = 1; }
	else if (pos == NXZ_IPH_NAME) { if (!b) stage = 2; }
	else if (pos == NXZ_IPH_COMMENT) { if (!b) stage = 3; }
	else if (pos == NXZ_IPH_HCRC0) { c->hleft = b; c->hpos = NXZ_IPH_HCRC1; }
	else if ((~c->hcrc & 0xffff) != (c->hleft | b << 8)) st = NXZ_FRAME_BAD_HCRC;      /* NXZ_IPH_HCRC1 */
	else complete = true;
	if (st != NXZ_FRAME_OK) return nxz_inflate_part_header_fail(c, st);
	if (stage < 4) return nxz_inflate_part_header_next(c, stage);
	if (!complete) return NXZ_IPH_MORE;
	f->status = NXZ_FRAME_OK;
	c->phase = NXZ_INFLATE_PHASE_BODY;
	return NXZ_IPH_COMPLETE;
}
/* the part's bytes through the state machine while the phase is HEADER: how many it took */
NXZ_HD inline uint32_t nxz_inflate_part_header_run(nxz_inflate_carry_t *c, int fmt, const uint8_t *p, uint32_t len)
{
	uint32_t q = 0;
	NXZ_IP_LOOP
	while (q < len && nxz_inflate_part_header_byte(c, fmt, p[q++]) == NXZ_IPH_MORE) ;
	return q;
}

/* ---- the slot ---- */
NXZ_HD inline uint32_t nxz_inflate_part_window(uint32_t prev_len, uint64_t total_out)
{
	const uint32_t w = prev_len < NXZ_INFLATE_PART_WINDOW ? prev_len : NXZ_INFLATE_PART_WINDOW;
	return total_out < w ? (uint32_t)total_out : w;
}
/* the room the host sets aside for a part's slot: the largest window, a full tail, every byte of the part -- a multiple of 16 */
NXZ_HD inline uint64_t nxz_inflate_part_slot_bound(const nxz_inflate_part_job_t *j)
{
	return ((uint64_t)(j->prev_len < NXZ_INFLATE_PART_WINDOW ? j->prev_len : NXZ_INFLATE_PART_WINDOW) + NXZ_INFLATE_PART_TAIL + j->src_len + 15) & ~15ull;
}

/* ---- the trailer ---- */
NXZ_HD inline uint32_t nxz_inflate_part_trailer_len(uint32_t format) { return format == NXZ_FMT_RAW ? 0 : nxz_frame_trailer_bytes(format); }
/* phase TRAILER: up to `avail` bytes at p join the trailer bytes in the tail; how many were taken */
NXZ_HD inline uint32_t nxz_inflate_part_trailer_take(nxz_inflate_carry_t *c, const uint8_t *p, uint32_t avail)
{
	/* (a record that was never started may say TRAILER with any tail: nothing is taken where the tail is a trailer's length or more) */
	const uint32_t tl = nxz_inflate_part_trailer_len(c->frame.format), want = c->tail_len < tl ? tl - c->tail_len : 0, k = avail < want ? avail : want;
	NXZ_IP_LOOP
	for (uint32_t i = 0; i < k; i++) c->tail[c->tail_len + i] = p[i];
	c->tail_len += k;
	return k;
}
/* ... and, when all are there (total_in counts them already), the verdict: true, phase DONE or FAILED */
NXZ_HD inline bool nxz_inflate_part_trailer_finish(nxz_inflate_carry_t *c)
{
	nxz_batch_frame_t *const f = &c->frame;
	if (c->tail_len < nxz_inflate_part_trailer_len(f->format)) return false;
	uint32_t check = 0, isize = 0, st = NXZ_FRAME_OK;
	if (f->format != NXZ_FMT_RAW) st = nxz_frame_trailer_status(f->format, c->tail, c->crc, c->adler, (uint32_t)c->total_out, true, &check, &isize);
	f->check = check; f->isize = isize; f->status = st;
	f->end = (uint32_t)c->total_in;
	c->tail_len = 0;
	c->phase = st == NXZ_FRAME_OK ? NXZ_INFLATE_PHASE_DONE : NXZ_INFLATE_PHASE_FAILED;
	return true;
}

/* ---- a part's result from the carry as it stands ---- */
NXZ_HD inline void nxz_inflate_part_report(const nxz_inflate_carry_t *c, uint32_t cc, uint32_t status, uint32_t in_used, uint32_t out_len,
					   nxz_inflate_part_result_t *o)
{
	o->cc = cc; o->status = status; o->in_used = in_used; o->out_len = out_len;
	o->crc = c->crc; o->adler = c->adler;
	o->reserved[0] = o->reserved[1] = 0;
}
NXZ_HD inline void nxz_inflate_part_refuse(uint32_t cc, nxz_inflate_part_result_t *o)
{
	o->cc = cc; o->status = NXZ_INFLATE_PART_FAILED; o->in_used = 0; o->out_len = 0; o->crc = 0; o->adler = 0;
	o->reserved[0] = o->reserved[1] = 0;
}

/* ---- the open: everything of an accepted part that needs no decode.  Returns true when the part goes on to the decode (phase BODY
 * with bytes to decode): *body = the offset of the first of them in the part; else the part is settled and *o is its result ---- */
NXZ_HD inline bool nxz_inflate_part_open(nxz_inflate_carry_t *c, const nxz_inflate_part_job_t *j, int fmt, uint32_t *body, nxz_inflate_part_result_t *o)
{
	if (j->flags & NXZ_PART_FIRST) nxz_inflate_part_start(c, fmt);
	uint32_t q = 0;
	if (c->phase == NXZ_INFLATE_PHASE_HEADER) q = nxz_inflate_part_header_run(c, fmt, j->src, j->src_len);
	*body = q;
	if (c->phase == NXZ_INFLATE_PHASE_BODY && q < j->src_len) return true;
	uint32_t status = NXZ_INFLATE_PART_MORE, used = j->src_len;
	if (c->phase == NXZ_INFLATE_PHASE_TRAILER) {
		used = nxz_inflate_part_trailer_take(c, j->src, j->src_len);
		c->total_in += used;
		if (nxz_inflate_part_trailer_finish(c)) status = c->phase == NXZ_INFLATE_PHASE_DONE ? NXZ_INFLATE_PART_DONE : NXZ_INFLATE_PART_FAILED;
	} else if (c->phase == NXZ_INFLATE_PHASE_FAILED) {                /* the header's fault */
		status = NXZ_INFLATE_PART_FAILED; used = 0;
	} else c->total_in += used;
	c->parts++;
	nxz_inflate_part_report(c, NXZ_CC_OK, status, used, 0, o);
	return false;
}

/* ---- the job of a part that goes on to the decode: [window][tail][part from `body`] at `slot` (16-byte aligned) -- or, with
 * neither window nor tail, the part where it lies.  That shortcut, and a dst of any alignment, hand the raw batch pointers that
 * nxz_batch_job_t's own comment wants 16-byte aligned: they rely on what nxz_batch_decompress_framed already relies on -- every
 * decode route takes a source of any alignment, and a target that is not 16-byte aligned on its slower path
 * (tests/test_gpu_inflate_part.py runs sources and targets at every alignment).  *table: the slot's table when the stream stands inside a dynamic block ---- */
NXZ_HD inline bool nxz_inflate_part_staged(const nxz_inflate_carry_t *c, const nxz_inflate_part_job_t *j)
{
	return nxz_inflate_part_window(j->prev_len, c->total_out) != 0 || c->tail_len != 0;
}
NXZ_HD inline nxz_batch_job_t nxz_inflate_part_decode_job(const nxz_inflate_carry_t *c, const nxz_inflate_part_job_t *j, uint32_t body, uint8_t *slot,
							  nxz_batch_dht_t *table)
{
	const uint32_t w = nxz_inflate_part_window(j->prev_len, c->total_out);
	nxz_batch_job_t d;
	d.src = nxz_inflate_part_staged(c, j) ? slot : j->src + body;
	d.dst = j->dst;
	d.hist_len = w;
	d.src_len = w + c->tail_len + (j->src_len - body);
	d.dst_cap = j->dst_cap;
	d.in_crc = c->crc; d.in_adler = c->adler;
	d.dht_index = 0;
	d.resume = (c->rem & 0xffff) | (c->sfbt & 15) << 16 | (c->subc & 7) << 20;
	d.reserved = NXZ_JOB_SUSPEND_WHEN_FULL;
	if ((c->sfbt & 0xe) == 0xc) {
		table->dhtlen = c->dhtlen;
		nxz_inflate_part_copy_table(table->dht, c->dht);
	}
	return d;
}
/* a part that does not go on to the decode still has a job in the chunk's batch: an empty one */
NXZ_HD inline nxz_batch_job_t nxz_inflate_part_idle_job(uint8_t *slot)
{
	nxz_batch_job_t d;
	d.src = slot; d.dst = slot;
	d.src_len = d.hist_len = d.dst_cap = d.in_crc = d.dht_index = d.resume = 0;
	d.in_adler = 1;
	d.reserved = NXZ_JOB_SUSPEND_WHEN_FULL;
	return d;
}

/* ---- the close: the decode's result r for job d (table: its slot) into the carry and the part's result.  With L = the bytes of
 * [tail][part from body] and `cons` of them touched by the decode (spbc less the window):
 *   a failure               phase FAILED, NXZ_FRAME_DEFLATE, nothing else moves;
 *   the final end-of-block   the deflate data ends at dend = cons - subc / 8; the trailer's bytes from there on go into the tail and
 *                           are checked when all are there (raw: at once);
 *   suspended, cons == L    the source ran out (or the target filled at a token inside the last byte): the stream stands `back` =
 *                           ceil(subc / 8) bytes in front of the end, those bytes are the new tail, MORE, in_used = src_len;
 *   suspended, cons < L     the target is full: DST_FULL, the stream stands at P = cons - back; in_used = P less the old tail, and
 *                           what is left of the old tail when P lies inside it stays the tail. ---- */
NXZ_HD inline void nxz_inflate_part_fail_deflate(nxz_inflate_carry_t *c, uint32_t cc, nxz_inflate_part_result_t *o)
{
	c->frame.status = NXZ_FRAME_DEFLATE;
	c->phase = NXZ_INFLATE_PHASE_FAILED;
	nxz_inflate_part_report(c, cc, NXZ_INFLATE_PART_FAILED, 0, 0, o);
}
NXZ_HD inline void nxz_inflate_part_close(nxz_inflate_carry_t *c, const nxz_inflate_part_job_t *j, uint32_t body, const nxz_batch_job_t *d,
					  const nxz_batch_result_t *r, const nxz_batch_dht_t *table, nxz_inflate_part_result_t *o)
{
	const uint32_t hist = d->hist_len, L = d->src_len - hist, told = c->tail_len;
	const uint8_t *const s = d->src + hist;                           /* [tail][part from body] */
	c->parts++;
	if ((r->cc != NXZ_CC_OK && r->cc != NXZ_CC_DATA_LENGTH) || r->spbc < hist || r->spbc - hist > L) {
		nxz_inflate_part_fail_deflate(c, r->cc, o);
		return;
	}
	const uint32_t cons = r->spbc - hist;
	if (r->sfbt & 0x100) {
		const uint32_t dend = cons - (r->subc >> 3);
		c->crc = r->crc; c->adler = r->adler; c->total_out += r->tpbc;
		c->sfbt = c->rem = c->dhtlen = c->subc = 0;
		c->tail_len = 0;
		c->phase = NXZ_INFLATE_PHASE_TRAILER;
		const uint32_t at = dend + nxz_inflate_part_trailer_take(c, s + dend, L - dend), used = body + (at > told ? at - told : 0);
		c->total_in += used;
		const bool done = nxz_inflate_part_trailer_finish(c);
		nxz_inflate_part_report(c, r->cc, !done ? NXZ_INFLATE_PART_MORE : c->phase == NXZ_INFLATE_PHASE_DONE ? NXZ_INFLATE_PART_DONE : NXZ_INFLATE_PART_FAILED,
					used, r->tpbc, o);
		return;
	}
	const uint32_t back = (r->subc + 7) >> 3, kind = r->sfbt & 0xe, tlen = kind == 0xc ? table->dhtlen : 0;
	if (back > cons || tlen > NXZ_DHT_MAXSZ * 8 || (cons == L && back > NXZ_INFLATE_PART_TAIL)) {
		nxz_inflate_part_fail_deflate(c, r->cc, o);
		return;
	}
	const uint32_t P = cons - back;
	c->crc = r->crc; c->adler = r->adler; c->total_out += r->tpbc;
	c->sfbt = r->sfbt & 15; c->rem = kind == 0x8 ? r->tebc : 0; c->subc = r->subc & 7;
	c->dhtlen = tlen;
	if (kind == 0xc) nxz_inflate_part_copy_table(c->dht, table->dht);
	uint32_t used, status, keep_to;
	if (cons == L) { status = NXZ_INFLATE_PART_MORE; used = j->src_len; keep_to = L; }
	else { status = NXZ_INFLATE_PART_DST_FULL; used = body + (P > told ? P - told : 0); keep_to = P < told ? told : P; }
	/* the new tail: bytes [P, keep_to) of s -- never the carry's own bytes: a part with a tail is staged */
	NXZ_IP_LOOP
	for (uint32_t k = 0; k < keep_to - P; k++) c->tail[k] = s[P + k];
	c->tail_len = keep_to - P;
	c->total_in += used;
	nxz_inflate_part_report(c, r->cc, status, used, r->tpbc, o);
}
#endif
