// nxz_encode.hip -- entropy stage of the DEFLATE compression engine (gfx950, wave64).
//
// Second half of the COMPRESS function codes (issued at /root/reference lib/nx_deflate.c:1808,1841;
// contract inc_nx/nxu.h:286-616, consumer code lib/nx_deflate.c:969-1078): the LZ77 kernel
// (nxz_lz77.hip) leaves, per job, two position bitmaps (where a literal token starts, where a
// match token starts) and the match tokens' (length, distance) records in parse order; this
// kernel turns them into one deflate block -- fixed code, a caller's dynamic table, or the
// table the device built from this very job's symbol counts (nxz_dhtgen.hip).
//
// Position parallel: a 256-thread workgroup per job walks the block in rounds of 2048
// positions, 8 consecutive positions per lane.  A lane knows its tokens from the two bitmaps,
// reads its literals from the source and its matches from the record array (rank of a match =
// number of match bits in front of it; the ranks of all 2048 bitmap words are made once per job),
// sums the code lengths, gets a bit offset from the workgroup prefix sum and ORs its codes into
// an LDS window that leaves as coalesced dwords.  A round's match records are turned into their
// codes once each, a round ahead, by the lanes that copy them to LDS; the lanes of the round only
// load a finished code.  Nothing here is serial over the block, and with ~21 KiB of LDS seven
// workgroups share a CU, so the latencies of one hide behind the others.
// The block's checksums are made here as well (the LZ77 kernel's non-fused forms leave crc / adler of the result
// record to this kernel: its one workgroup a CU has nothing to hide their table look-ups behind): a pass over the
// source at the top, 64-byte slices side by side (nxz_cksum_slices.h), the CRC table in the not yet used windows.
// Bit for bit the encoder of oracle/nxz_lz77.c (put_tokens / nxo_encode_fixed / nxo_encode_dynamic).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include "nxz_device.h"
#include "nxz_cksum_slices.h"

namespace nxze {

constexpr int NT = 256;
constexpr uint32_t RPOS = 2048;                 // positions per round: 8 per lane, two quads of 4
constexpr uint32_t LANE_BITS_MAX = 144;         // three 48-bit match tokens in 8 positions
constexpr uint32_t HDR_WORDS = 74;              // 3 + 2283 bits of a dynamic header at most
constexpr uint32_t WWORDS = NT * LANE_BITS_MAX / 32 + HDR_WORDS + 2;   // 1228
constexpr uint32_t RECMAX = RPOS / 3 + 6;       // match tokens that can start in one round

typedef uint32_t v4u __attribute__((ext_vector_type(4)));
typedef uint32_t v2u __attribute__((ext_vector_type(2)));

// The tokens that start in four consecutive positions, as one bit string (<= 96 bits: a match at
// the first position and one at the fourth).  Straight-line code, the same for every lane.
struct Quad { uint32_t a0, a1, a2, nb; };

// A match record (length - 3, distance - 1) as its finished code: x = bits 0..31, y = bits 32..47 | bit length << 16
// (<= 20 bits of length code and extra bits, then <= 28 of distance code and extra bits).  Done once per record, by the
// lane that copies it to LDS, not by every lane whose quad might hold a match.
// CHECK: a symbol without a code can occur (a caller's table; the table the device made of this very block's counts has
// a code for every symbol the block uses -- nxz_dhtgen.hip as lib/nx_dhtgen.c:252-270 -- and the fixed code for all)
template <bool CHECK>
__device__ __forceinline__ v2u code_record(const uint32_t *lltab, const uint32_t *dtab, uint32_t r, bool &missing)
{
	const uint32_t l3 = r & 0xff, d = (r >> 8) & 0x7fff;
	uint32_t le = l3 < 8 ? 0 : (29 - (uint32_t)__builtin_clz(l3 | 8));
	const uint32_t ls = l3 == 255 ? 28 : (le << 2) + (l3 >> le);
	if (l3 == 255) le = 0;
	const uint32_t de = d < 4 ? 0 : (30 - (uint32_t)__builtin_clz(d | 4));
	const uint32_t ds = d < 4 ? d : 2 * de + 2 + ((d >> de) & 1);
	const uint32_t lt = lltab[257 + ls], dt = dtab[ds];
	const uint32_t ll = lt >> 16, dl = dt >> 16;
	if (CHECK) missing = ll == 0 || dl == 0;
	const uint32_t lo = (lt & 0xffff) | ((l3 & ((1u << le) - 1)) << ll);          // <= 20 bits
	const uint32_t hi = (dt & 0xffff) | ((d & ((1u << de) - 1)) << dl);           // <= 28 bits
	const uint64_t mv = (uint64_t)lo | ((uint64_t)hi << (ll + le));
	return (v2u){ (uint32_t)mv, (uint32_t)(mv >> 32) | ((ll + le + dl + de) << 16) };
}

template <bool CHECK>
__device__ __forceinline__ Quad encode_quad(const uint32_t *lltab, const v2u *rec, uint32_t &ri,
					    uint32_t b, uint32_t lit4, uint32_t tok4, bool &missing)
{
	// literals: four look-ups whether or not a literal starts there (a position without one adds no bits)
	uint32_t e0 = lltab[b & 0xff], e1 = lltab[(b >> 8) & 0xff], e2 = lltab[(b >> 16) & 0xff], e3 = lltab[b >> 24];
	if (CHECK) missing |= ((lit4 & 1) && !(e0 >> 16)) || ((lit4 & 2) && !(e1 >> 16)) || ((lit4 & 4) && !(e2 >> 16)) || ((lit4 & 8) && !(e3 >> 16));
	e0 = (lit4 & 1) ? e0 : 0; e1 = (lit4 & 2) ? e1 : 0; e2 = (lit4 & 4) ? e2 : 0; e3 = (lit4 & 8) ? e3 : 0;
	// the literals among themselves, <= 60 bits: two pairs in 32 bits each, one wide shift
	const uint32_t n0 = e0 >> 16, n2 = e2 >> 16, n01 = n0 + (e1 >> 16);
	const uint32_t p01 = (e0 & 0xffff) | ((e1 & 0xffff) << n0), p23 = (e2 & 0xffff) | ((e3 & 0xffff) << n2);
	// the quad is x, then y: a match lies behind all its literals, but for one at the first position, where a literal
	// (or a second match) can only follow at the fourth -- matches are at least three bytes long
	uint64_t x = (uint64_t)p01 | ((uint64_t)p23 << n01), y = 0;
	uint32_t nx = n01 + n2 + (e3 >> 16), ny = 0;
	if (__ballot(tok4 != 0)) {
		const v2u m = rec[ri];                                                  // coded when it was staged
		const uint64_t mv = (uint64_t)m.x | ((uint64_t)(m.y & 0xffff) << 32);
		const uint32_t mn = m.y >> 16;
		if (tok4 & 1) { y = x; ny = nx; x = mv; nx = mn; }                     // (here x was the fourth position's literal alone)
		else if (tok4) { y = mv; ny = mn; }
		ri += tok4 ? 1 : 0;
		if (__ballot(tok4 == 9)) {
			const v2u m2 = rec[ri];
			if (tok4 == 9) { y = (uint64_t)m2.x | ((uint64_t)(m2.y & 0xffff) << 32); ny = m2.y >> 16; ri++; }
		}
	}
	// nx <= 60 (four literals) and y < 2^48; behind a match (nx <= 48) y is one literal or a match
	const uint64_t lo = x | (y << nx);
	Quad q;
	q.a0 = (uint32_t)lo; q.a1 = (uint32_t)(lo >> 32); q.a2 = nx ? (uint32_t)(y >> (64 - nx)) : 0; q.nb = nx + ny;
	return q;
}

// ORs a quad's bits into the window at bit position bitpos
__device__ __forceinline__ void emit_quad(uint32_t *w, const Quad &q, uint32_t bitpos)
{
	if (!q.nb) return;
	const uint32_t sh = bitpos & 31, wi = bitpos >> 5, endw = (sh + q.nb + 31) >> 5;   // dwords touched: 1..4
	const uint64_t s01 = (((uint64_t)q.a1 << 32) | q.a0) << sh, s12 = (((uint64_t)q.a2 << 32) | q.a1) << sh;
	atomicOr(&w[wi], (uint32_t)s01);
	if (endw > 1) atomicOr(&w[wi + 1], (uint32_t)(s01 >> 32));
	if (endw > 2) atomicOr(&w[wi + 2], (uint32_t)(s12 >> 32));
	if (endw > 3) atomicOr(&w[wi + 3], (uint32_t)(((uint64_t)q.a2 << sh) >> 32));
}

template <bool DHT, bool CHECK = DHT>
__global__ __launch_bounds__(NT) void encode_kernel(const nxz_batch_job_t *__restrict__ jobs_, const uint8_t *__restrict__ tokens_,
						     const nxz_dht_prepared_t *__restrict__ tables_, int table_per_job,
						     nxz_batch_result_t *__restrict__ results_, uint32_t njobs)
{
	__shared__ uint32_t lltab[288];
	__shared__ uint32_t dtab[32];
	__shared__ __attribute__((aligned(16))) uint32_t win[2][WWORDS + 2];   // two windows: one fills while the other leaves
	// the round's match tokens as finished codes (code_record).  One buffer: a round reads it before its first barrier,
	// the next round's are written between that barrier and the second
	__shared__ __attribute__((aligned(8))) v2u recbuf[RECMAX + 2];
	__shared__ uint16_t rankpre[2048 + 2];                                 // matches in front of every 32 positions; [2048] = all
	__shared__ uint32_t wsum[2][NT / 64];
	__shared__ uint32_t errflag;
	__shared__ uint32_t ckred[4][NT / 64];                                 // the wavefronts' checksum parts
	__shared__ uint32_t ckout[2];                                          // crc, adler of the result record
	const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
	const uint32_t bid = blockIdx.x;
	if (bid >= njobs) return;
	const nxz_batch_job_t job = jobs_[bid];
	const uint32_t total = job.src_len;
	const uint32_t h = job.hist_len < total ? job.hist_len : total;
	const uint32_t n = total - h;
	// (the source alone: for the jobs of nxz_batch_compress_dict -- nxzl77::dict_jobs_kernel -- the h bytes below it are NOT memory of the caller's)
	const uint8_t NXZ_GLOBAL_AS *src = (const uint8_t NXZ_GLOBAL_AS *)job.src + h;
	const uint8_t NXZ_GLOBAL_AS *tk = (const uint8_t NXZ_GLOBAL_AS *)tokens_ + (size_t)bid * NXZ_TOK_STRIDE;
	const uint32_t NXZ_GLOBAL_AS *litb = (const uint32_t NXZ_GLOBAL_AS *)(tk + NXZ_TOK_LITBITS);
	const uint32_t NXZ_GLOBAL_AS *tokb = (const uint32_t NXZ_GLOBAL_AS *)(tk + NXZ_TOK_MATCHBITS);
	const uint32_t NXZ_GLOBAL_AS *recs = (const uint32_t NXZ_GLOBAL_AS *)(tk + NXZ_TOK_RECORDS);
	uint32_t NXZ_GLOBAL_AS *dstw = (uint32_t NXZ_GLOBAL_AS *)job.dst;
	const uint32_t cap_words = job.dst_cap >> 2;
	const nxz_dht_prepared_t NXZ_GLOBAL_AS *tb = DHT ? (const nxz_dht_prepared_t NXZ_GLOBAL_AS *)tables_ + (table_per_job ? bid : job.dht_index) : nullptr;
	const uint32_t nwords = (n + 31) >> 5;

	// What a lane needs of a round is asked for a round ahead, so that the loads' latency hides
	// behind the work on the round before: its 8 source bytes, the two bitmap words that hold its
	// 8 positions, and its share of the round's match records (to be coded into the LDS copy).
	struct Fetch { v2u bytes; uint32_t litw, tokw, rec[3], nrec; };
	auto fetch = [&](uint32_t r0, Fetch &f) {
		const uint32_t p0 = r0 + 8 * t;
		f.bytes = (v2u){ 0, 0 }; f.litw = 0; f.tokw = 0;
		if (p0 < n) {
			f.litw = litb[p0 >> 5];
			f.tokw = tokb[p0 >> 5];
			if (p0 + 8 <= n) f.bytes = *(const v2u NXZ_GLOBAL_AS *)(src + p0);
			else {
				// ragged end: nothing is read past the source
				uint64_t v = 0;
				for (uint32_t i = 0; i < 8; i++) if (p0 + i < n) v |= (uint64_t)src[p0 + i] << (8 * i);
				f.bytes = (v2u){ (uint32_t)v, (uint32_t)(v >> 32) };
			}
		}
	};
	auto fetch_recs = [&](uint32_t r0, Fetch &f) {                // needs rankpre
		const uint32_t ra = __builtin_amdgcn_readfirstlane(rankpre[r0 >> 5]);
		const uint32_t rb = __builtin_amdgcn_readfirstlane(rankpre[(r0 + RPOS) >> 5 < 2048 ? (r0 + RPOS) >> 5 : 2048]);
		f.nrec = rb - ra < RECMAX ? rb - ra : RECMAX;
#pragma unroll
		for (int j = 0; j < 3; j++) f.rec[j] = t + 256 * j < f.nrec ? recs[ra + t + 256 * j] : 0;
	};
	bool missing = false;
	// Every record is coded once, here, by the lane that fetched it; a pass none of the wavefront's lanes has a record
	// for is skipped (a usual round: one pass on the first few wavefronts).  Every staged record is a token of the block.
	auto stage_recs = [&](const Fetch &f) {
#pragma unroll
		for (int j = 0; j < 3; j++) {
			const bool have = t + 256 * j < f.nrec;
			if (!__ballot(have)) break;
			bool miss = false;
			const v2u c = code_record<CHECK>(lltab, dtab, f.rec[j], miss);
			if (have) {
				recbuf[t + 256 * j] = c;
				if (CHECK) missing |= miss;
			}
		}
	};
	// ---- CRC-32 and Adler-32 of the source (seeded: job.in_crc, job.in_adler), as the LZ77 kernel's fused forms make them ----
	// The slice-by-4 table (4 KiB) stands in the windows, which are cleared only afterwards: no LDS of its own, seven
	// workgroups a CU as before.
	{
		static_assert(sizeof(win) >= 1024 * sizeof(uint32_t) && NT == (int)nxzck::LANES, "the CRC table borrows the windows; a lane per table column");
		uint32_t *T = &win[0][0];
		nxzck::table_column(T, (uint32_t)t);
		__syncthreads();
		const nxzck::Shape shp = nxzck::shape_of(n);
		const nxzck::Part p = nxzck::lane_part((const uint8_t *)src, shp, job.in_crc ^ 0xffffffffu, (uint32_t)t, T);
		uint32_t c = p.crc, tc = p.tailcrc, a1 = p.s1, a2 = p.s2;
		for (int o = 32; o > 0; o >>= 1) {
			c ^= __shfl_down(c, o, 64);
			tc ^= __shfl_down(tc, o, 64);
			a1 += __shfl_down(a1, o, 64);
			a2 += __shfl_down(a2, o, 64);
		}
		if (lane == 0) { ckred[0][wave] = c; ckred[1][wave] = tc; ckred[2][wave] = a1; ckred[3][wave] = a2; }
		__syncthreads();                                         // (and the table is done with: the windows are cleared below)
		if (t == 0) {
			c = 0; tc = 0; a1 = 0; a2 = 0;
			for (int w = 0; w < NT / 64; w++) { c ^= ckred[0][w]; tc ^= ckred[1][w]; a1 += ckred[2][w]; a2 += ckred[3][w]; }
			uint32_t oc, oa;
			nxzck::finish(shp, job.in_crc, job.in_adler, c, tc, a1, a2, oc, oa);
			ckout[0] = oc; ckout[1] = oa;                        // (thread 0 reads them back itself, at the end)
		}
	}
	Fetch nx;
	fetch(0, nx);                                                // round 0's bytes travel while the tables are set up

	// ---- tables, windows, ranks ----
	for (uint32_t i = t; i < 2 * (WWORDS + 2); i += NT) (&win[0][0])[i] = 0;
	if (t == 0) errflag = 0;
	{
		const v4u NXZ_GLOBAL_AS *tw = (const v4u NXZ_GLOBAL_AS *)tokb;
		v4u a = { 0, 0, 0, 0 }, b = a;
		if (8u * t < nwords) { a = tw[2 * t]; b = tw[2 * t + 1]; }
		const uint32_t w[8] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w };
		uint32_t c[8], s = 0;
#pragma unroll
		for (int k = 0; k < 8; k++) {
			c[k] = s;
			s += 8u * t + k < nwords ? (uint32_t)__popc(w[k]) : 0;  // (what lies behind the block's last word is not the kernel's)
		}
		uint32_t incl = s;
		for (int o = 1; o < 64; o <<= 1) { const uint32_t u = __shfl_up(incl, o, 64); if (lane >= o) incl += u; }
		if (lane == 63) wsum[0][wave] = incl;
		if (DHT) {
			for (int i = t; i < 288; i += NT) lltab[i] = tb->ll[i];
			if (t < 32) dtab[t] = tb->d[t];
		} else {
			for (int i = t; i < 288; i += NT) {
				// RFC1951 3.2.6 fixed code; entry = bit-reversed code | len << 16
				uint32_t len, code;
				if (i < 144) { len = 8; code = 0x30 + i; }
				else if (i < 256) { len = 9; code = 0x190 + (i - 144); }
				else if (i < 280) { len = 7; code = i - 256; }
				else { len = 8; code = 0xC0 + (i - 280); }
				lltab[i] = (__builtin_bitreverse32(code) >> (32 - len)) | (len << 16);
			}
			if (t < 32) dtab[t] = (__builtin_bitreverse32((uint32_t)t) >> 27) | (5u << 16);
		}
		__syncthreads();
		uint32_t off = incl - s;
		for (int k = 0; k < wave; k++) off += wsum[0][k];
#pragma unroll
		for (int k = 0; k < 8; k++) rankpre[8 * t + k] = (uint16_t)(off + c[k]);
		if (t == NT - 1) rankpre[2048] = (uint16_t)(off + s);
	}
	uint32_t base_bits;                                          // bits already in the current window (uniform)
	if (DHT) {
		const uint32_t hb = tb->dhtlen + 3;                      // BFINAL = 1 as emitted (the host rewrites it, lib/nx_deflate.c:158), BTYPE = 10
		const uint32_t nw = (hb + 31) >> 5;
		for (uint32_t i = t; i < nw && i < HDR_WORDS; i += NT) {
			const uint32_t cur = i < 74 ? tb->dhtw[i] : 0, prev = i ? tb->dhtw[i - 1] : 0;
			uint32_t w = (cur << 3) | (i ? prev >> 29 : 5u);
			if (i == (hb >> 5)) w &= (1u << (hb & 31)) - 1;       // the last, partial dword
			win[0][i] = w;
		}
		base_bits = hb;
	} else {
		if (t == 0) win[0][0] = 3u;                              // BFINAL = 1, BTYPE = 01
		base_bits = 3;
	}
	__syncthreads();
	// round 0's records: no round in front to hide behind
	{
		fetch_recs(0, nx);
		stage_recs(nx);
	}
	__syncthreads();

	uint32_t wordbase = 0, par = 0;
	for (uint32_t r0 = 0; r0 < n; r0 += RPOS, par ^= 1) {
		const Fetch k = nx;
		const bool more = r0 + RPOS < n;
		if (more) { fetch(r0 + RPOS, nx); fetch_recs(r0 + RPOS, nx); }
		uint32_t *w_ = win[par];
		const uint32_t p0 = r0 + 8 * t;
		const uint32_t sh8 = p0 & 24;
		const uint32_t lit8 = (k.litw >> sh8) & 0xff, tok8 = (k.tokw >> sh8) & 0xff;
		Quad q0{0, 0, 0, 0}, q1{0, 0, 0, 0};
		if (__ballot((lit8 | tok8) != 0)) {
			// my first record: matches of the round in front of my positions
			uint32_t ri = (uint32_t)rankpre[p0 >> 5 < 2048 ? p0 >> 5 : 2048] + (uint32_t)__popc(k.tokw & ((1u << (p0 & 31)) - 1)) - (uint32_t)rankpre[r0 >> 5];
			if (p0 >= n) ri = 0;
			q0 = encode_quad<CHECK>(lltab, recbuf, ri, k.bytes.x, lit8 & 15, tok8 & 15, missing);
			q1 = encode_quad<CHECK>(lltab, recbuf, ri, k.bytes.y, lit8 >> 4, tok8 >> 4, missing);
		}
		const uint32_t nbits = q0.nb + q1.nb;
		uint32_t incl = nbits;
		for (int o = 1; o < 64; o <<= 1) { const uint32_t u = __shfl_up(incl, o, 64); if (lane >= o) incl += u; }
		if (lane == 63) wsum[par][wave] = incl;
		__syncthreads();
		uint32_t bitpos = base_bits + incl - nbits, roundbits = 0;
#pragma unroll
		for (int w = 0; w < NT / 64; w++) { const uint32_t s = wsum[par][w]; if (w < wave) bitpos += s; roundbits += s; }
		emit_quad(w_, q0, bitpos);
		emit_quad(w_, q1, bitpos + q0.nb);
		// the next round's records (asked for at the top of this round), coded, into the LDS copy: this round has read its own
		if (more) stage_recs(nx);
		__syncthreads();
		// this window leaves (whole dwords) and is cleared; its last, partial dword opens the other
		// window, which the next round fills (atomicOr: that round's lanes may be there already)
		const uint32_t tot = base_bits + roundbits, nfull = tot >> 5;
		for (uint32_t i = t; i < nfull; i += NT) {
			if (wordbase + i < cap_words) dstw[wordbase + i] = w_[i];
			w_[i] = 0;
		}
		if (t == 0) {
			const uint32_t keep = w_[nfull];
			if (keep) atomicOr(&win[par ^ 1][0], keep);
			w_[nfull] = 0;
		}
		wordbase += nfull;
		base_bits = tot & 31;
	}
	if (missing) errflag = 1;
	__syncthreads();
	uint32_t *w_ = win[par];
	// a job without any round (n == 0) still has its header in the window
	if (base_bits >= 32) {
		const uint32_t nfull = base_bits >> 5;
		for (uint32_t i = t; i < nfull; i += NT)
			if (wordbase + i < cap_words) dstw[wordbase + i] = w_[i];
		const uint32_t keep = w_[nfull];
		__syncthreads();
		if (t == 0) w_[0] = keep;
		wordbase += nfull;
		base_bits &= 31;
		__syncthreads();
	}
	// ---- EOB + tail ----
	if (t == 0) {
		const uint32_t lt = lltab[256];
		uint32_t cc = 0;
		if (wordbase > cap_words) cc = NXZ_CC_TARGET_SPACE;
		if (DHT && (errflag || (lt >> 16) == 0)) cc = NXZ_CC_MISSING_CODE;
		if (DHT && tb->status) cc = NXZ_CC_INVALID_DHT;
		const uint64_t acc = (uint64_t)w_[0] | ((uint64_t)(lt & 0xffff) << base_bits);
		const uint32_t bits = base_bits + (lt >> 16);
		const uint64_t totbits = (uint64_t)wordbase * 32 + bits;
		const uint32_t tpbc = (uint32_t)((totbits + 7) >> 3);
		if (tpbc > job.dst_cap) cc = cc ? cc : NXZ_CC_TARGET_SPACE;
		if (cc != NXZ_CC_TARGET_SPACE && (uint64_t)wordbase * 4 + (bits + 7) / 8 <= job.dst_cap) {
			uint8_t NXZ_GLOBAL_AS *o = (uint8_t NXZ_GLOBAL_AS *)job.dst + (size_t)wordbase * 4;
			for (uint32_t b = 0; b < (bits + 7) / 8; b++) o[b] = (uint8_t)(acc >> (8 * b));
		}
		if (cc == 0 && tpbc > total) cc = NXZ_CC_TPBC_GT_SPBC;
		nxz_batch_result_t *r = results_ + bid;
		r->cc = cc;
		r->tpbc = cc == NXZ_CC_TARGET_SPACE ? 0 : tpbc;
		r->tebc = (uint32_t)(totbits & 7);
		r->sfbt = 0;                                            // (the LZ77 kernel left its match count there)
		r->crc = ckout[0];
		r->adler = ckout[1];
	}
}

} // namespace nxze

extern "C" int nxz_launch_encode(int dht, int table_per_job, const nxz_batch_job_t *jobs, size_t n, const uint8_t *tokens,
				 const nxz_dht_prepared_t *tables, nxz_batch_result_t *results, hipStream_t stream)
{
	if (n == 0) return 0;
	// NXZ_ENCODE_CHECK=1: the tables the device made go through the kernel form that looks for symbols without a code as well
	// (cc 11 instead of a zero-length code in the block if the LZ77 kernel's counts and its tokens ever disagreed) -- the same
	// bytes, a few per cent slower; tests/test_gpu_parity.py runs the corpus blocks this way.  (Read at every call: the tests switch it.)
	const char *chk = getenv("NXZ_ENCODE_CHECK");
	if (dht && table_per_job && !(chk && atoi(chk) != 0)) hipLaunchKernelGGL((nxze::encode_kernel<true, false>), dim3((unsigned)n), dim3(nxze::NT), 0, stream, jobs, tokens, tables, table_per_job, results, (uint32_t)n);
	else if (dht) hipLaunchKernelGGL(nxze::encode_kernel<true>, dim3((unsigned)n), dim3(nxze::NT), 0, stream, jobs, tokens, tables, table_per_job, results, (uint32_t)n);
	else hipLaunchKernelGGL(nxze::encode_kernel<false>, dim3((unsigned)n), dim3(nxze::NT), 0, stream, jobs, tokens, tables, 0, results, (uint32_t)n);
	return (int)hipGetLastError();
}
