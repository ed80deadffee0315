// nxz_inflate_walk.h -- the walk of the output-size queries as a device function: from the first block header of a deflate stream to
// the place it stops, counting the bytes every token would make (no window, no stores, 64-bit sums, src at any alignment).  Shared by
// nxz_inflate_size.hip (nxzs::size_kernel: a stream a wavefront) and nxz_gzip_members.hip (nxzg::index_kernel: a wavefront walks
// member after member of a gzip job); with a hook, by the checkpoint kernels (nxz_checkpoint.hip, nxz_checkpoint_fine.hip) and -- a hook
// that is handed the bytes of every token -- by nxz_checkpoint_build.hip and nxz_inflate_verify.hip.  Like nxz_inflate_decode.h it is written for a workgroup of ONE wavefront.
#ifndef NXZ_INFLATE_WALK_H
#define NXZ_INFLATE_WALK_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "nxz_device.h"
#include "nxz_inflate_decode.h"
#include "nxz_size.h"

namespace nxzs {
using namespace nxzi;

struct Smem {
	uint32_t stage[STAGE / 4 + 4];
	Huff hl;
	HuffD hd;
	uint8_t lens[320];
	uint8_t cl[32];
};

// The chain of real token starts through the lanes' answers of a multi-token step (the walk of nxz_inflate.hip's walk_chain: tl is
// the bits of the token that would start at a lane's bit, 0 for none; every lane names the lane its token ends at, the walk is one
// v_readlane a link).  starts: the lanes on the chain that hold a token; off: the bits they use, all told.
__device__ __forceinline__ void chain_by_lane(int lane, const uint32_t tl, uint64_t &starts, uint32_t &off)
{
	const uint32_t to = (uint32_t)lane + tl;
	const uint32_t nxt = (tl && to < 64) ? to : (uint32_t)lane;
	const uint64_t valid = __ballot(tl != 0);
	uint32_t at = 0;
	uint64_t seen = 0;
	for (;;) {
		uint32_t before = 0;
#pragma unroll
		for (int u = 0; u < 4; u++) {
			seen |= 1ull << at;
			before = at;
			at = (uint32_t)__builtin_amdgcn_readlane((int)nxt, (int)at);
		}
		if (at == before) break;
	}
	starts = seen & valid;
	off = 0;
	if (starts) {
		const uint32_t last = 63 - (uint32_t)__builtin_clzll(starts);
		off = last + (uint32_t)__builtin_amdgcn_readlane((int)tl, (int)last);
	}
}

// what the walk calls at every block header -- the bit of src the header starts at, the bytes of output in front of it (the same in
// every lane) -- unless the caller passes a hook of its own (nxz_checkpoint.hip): nothing
struct NoHook { __device__ __forceinline__ void operator()(uint64_t, uint32_t) const {} };

// A hook that also cuts between tokens (nxz_checkpoint_fine.hip) declares `static constexpr bool fine` and has two more members:
//   uint32_t budget(uint32_t cap)    the output the walk may reach before the next cut, never above cap
//   void cut(uint64_t bit, uint32_t out, uint32_t sfbt, uint32_t rem, uint64_t tpos, uint32_t tbits)
//                                    a token that starts at `bit` (a stored byte: the byte) does not fit the budget: the output in
//                                    front of it, the block's sfbt, the stored bytes still to come, where the block's table starts
//                                    (the bit behind the 3-bit header) and its bits -- both 0 unless the block is dynamic
// The walk asks for the budget behind every header and every cut.  Without `fine` none of this is compiled: the budget is cap.
template <class H, class = void> struct cuts_tokens { static constexpr bool value = false; };
template <class H> struct cuts_tokens<H, decltype((void)H::fine)> { static constexpr bool value = true; };

// A hook that keeps the output (nxz_checkpoint_build.hip: a ring of the last 32 KiB) declares `static constexpr bool bytes` and
// receives the bytes of every token, in front of the header or cut call that follows them:
//   void lit(bool on, uint32_t at, uint32_t sym)                     a lane with `on` set holds the literal of output byte `at`
//   void match(uint32_t at, uint32_t dist, uint32_t len)             the whole wavefront, the same in every lane: len bytes at `at`
//                                                                    from dist back (dist < len: the copy feeds on itself)
//   void stored(uint32_t at, const NXZ_GLOBAL_AS uint8_t *p, uint32_t n)   the whole wavefront: n stored bytes at p are output bytes at `at` on
// Without `bytes` none of this is compiled: stored runs are counted, not read.
template <class H, class = void> struct keeps_bytes { static constexpr bool value = false; };
template <class H> struct keeps_bytes<H, decltype((void)H::bytes)> { static constexpr bool value = true; };

// The walk over srclen bytes at src for a target of cap bytes (0xffffffff: no limit); hist: how far a distance may reach in front of
// the output.  stop says where and why it ended (nxz_size.h; produced and, behind the final end-of-block code, subc are set), end_bit
// the bit of src it stands at -- in 64 bits, where stop.subc is a 32-bit field.  Every lane gets the same answers.
template <class Hook = NoHook>
__device__ __forceinline__ void walk(Smem &sm, const NXZ_GLOBAL_AS uint8_t *src, const uint32_t srclen, const uint32_t cap, const uint32_t hist,
				     const int lane, nxz_size_stop_t &stop, uint64_t &end_bit, Hook hook = Hook())
{
	Bits b;
	b.src = src; b.srclen = srclen; b.total_bits = (uint64_t)srclen * 8; b.pos = 0;
	b.stage_base = 0xffffffffu; b.stage = sm.stage; b.lane = lane;

	constexpr bool FINE = cuts_tokens<Hook>::value;
	constexpr bool KEEP = keeps_bytes<Hook>::value;
	uint32_t out = 0;                          // bytes the tokens so far make: never above cap
	uint32_t soft = cap;                       // what they may make before the hook cuts (FINE; else cap for good)
	uint64_t tpos = 0;                         // FINE: the table of the dynamic block in work
	uint32_t tlen = 0;
	// a token of len bytes that starts at `bit` fits -- if need be behind a cut in front of it
	auto fits_or_cut = [&](uint32_t len, uint64_t bit, uint32_t sfbt) __attribute__((always_inline)) -> bool {
		if (nxz_size_fits(out, len, soft)) return true;
		if constexpr (FINE) {
			if (soft < cap) {
				hook.cut(bit, out, sfbt, 0, tpos, tlen);
				soft = hook.budget(cap);
				return nxz_size_fits(out, len, soft);
			}
		}
		return false;
	};
	int state = 0;                             // 0 header, 1 stored, 2 coded
	uint32_t bfinal = 0, btype = 0, rem = 0;
	bool lit_mode = false;                     // the last multi-token step met literals only

	// two 256-byte blocks of the source in registers (lane k: dword k from the 4-byte boundary at or below src)
	const uint32_t skew = (uint32_t)((uintptr_t)src & 3);
	const NXZ_GLOBAL_AS uint8_t *abase = src - skew;
	const uint64_t alen = (uint64_t)srclen + skew;         // bytes from abase to the end of the source
	uint32_t W0 = 0, W1 = 0, wbase = 0x80000000u;          // wbase: dword index of W0's lane 0 (a multiple of 64; none yet)
	auto load_block = [&](uint32_t blk) -> uint32_t {
		const uint32_t idx = blk * 64 + lane;
		const uint64_t byte = (uint64_t)idx * 4;
		uint32_t w = 0;
		if (byte + 4 <= alen) w = ((const NXZ_GLOBAL_AS uint32_t *)abase)[idx];      // (the first dword may begin up to 3 bytes in front of src: the same aligned dword, never used)
		else for (uint32_t k = 0; byte + k < alen; k++) w |= (uint32_t)abase[byte + k] << (8 * k);
		return w;
	};

	for (;;) {
		if (state != 2) b.bb_sync();
		if (state == 0) {
			const uint64_t hdr = b.pos;
			hook(hdr, out);
			if constexpr (FINE) { soft = hook.budget(cap); tpos = 0; tlen = 0; }
			if (!b.have(3)) { stop.sfbt = 0xe; stop.subc = (uint32_t)(b.total_bits - hdr); break; }
			const uint32_t v = b.peek();
			bfinal = v & 1; btype = (v >> 1) & 3;
			b.pos += 3;
			if (btype == 0) {
				b.pos = (b.pos + 7) & ~7ull;
				if (!b.have(32)) { stop.sfbt = 0xe | bfinal; stop.subc = (uint32_t)(b.total_bits - hdr); break; }
				const uint32_t w = b.peek();
				b.pos += 32;
				if (((w ^ (w >> 16)) & 0xffff) != 0xffff) { stop.cc = NXZ_CC_INVALID_DHT; break; }
				rem = w & 0xffff;
				state = 1;
			} else if (btype == 1) {
				for (int i = lane; i < 288; i += 64) sm.lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8;
				if (lane < 30) sm.lens[288 + lane] = 5;
				__syncthreads();
				build<LBITS>(sm.hl, sm.lens, 288, lane);
				build<DBITS>(sm.hd, sm.lens + 288, 30, lane);
				state = 2;
			} else if (btype == 2) {
				int hlit, hdist; uint32_t tbits;
				const int rc = read_dht(b, sm, hlit, hdist, tbits);
				if (rc == 1) { stop.sfbt = 0xe | bfinal; stop.subc = (uint32_t)(b.total_bits - hdr); break; }
				if (rc < 0) { stop.cc = NXZ_CC_INVALID_DHT; break; }
				build<LBITS>(sm.hl, sm.lens, hlit, lane);
				build<DBITS>(sm.hd, sm.lens + hlit, hdist, lane);
				stop.have_dht = 1; stop.dhtbits = tbits;
				if constexpr (FINE) { tpos = hdr + 3; tlen = tbits; }
				state = 2;
			} else { stop.cc = NXZ_CC_INVALID_DHT; break; }
			lit_mode = false;
		} else if (state == 1) {
			// stored bytes: byte aligned; counted, not read (KEEP: handed to the hook)
			const uint64_t srcleft = (b.total_bits - b.pos) >> 3;
			const uint32_t n = rem < srcleft ? rem : (uint32_t)srcleft;
			if (!nxz_size_fits(out, n, soft)) {
				if constexpr (FINE) {
					if (soft < cap) {                                       // the run splits behind the bytes that fit
						const uint32_t take = soft - out;
						if constexpr (KEEP) hook.stored(out, src + (uint32_t)(b.pos >> 3), take);
						out += take; rem -= take;
						b.pos += (uint64_t)take * 8;
						hook.cut(b.pos, out, 0x8 | bfinal, rem, 0, 0);
						soft = hook.budget(cap);
						continue;
					}
				}
				stop.cc = NXZ_CC_TARGET_SPACE; break;
			}
			if constexpr (KEEP) hook.stored(out, src + (uint32_t)(b.pos >> 3), n);
			out += n; rem -= n;
			b.pos += (uint64_t)n * 8;
			if (rem) { stop.sfbt = 0x8 | bfinal; stop.subc = (uint32_t)(b.total_bits - b.pos); stop.rem = rem; break; }
			if (bfinal) { stop.final_eob = 1; break; }
			state = 0;
		} else {
			// ---- multi-token step (nxz_inflate.hip's, without everything that touches the window) ----
			while (b.pos + 256 <= b.total_bits) {
				const uint64_t abit = b.pos + 8 * skew;                 // the position counted from abase
				const uint32_t q = uni((uint32_t)(abit >> 5)), sh = uni((uint32_t)abit & 31);
				uint32_t wb = uni(wbase);
				if (q - wb >= 64u) {
					if (q - wb < 128u) { wb += 64; W0 = W1; W1 = load_block((wb >> 6) + 1); }
					else { wb = q & ~63u; W0 = load_block(wb >> 6); W1 = load_block((wb >> 6) + 1); }
					wbase = wb;
				}
				wb = uni(wb);
				const uint32_t qi = q - wb;                              // 0..63: dwords qi..qi+4 are in W0/W1
				auto word = [&](uint32_t i) __attribute__((always_inline)) -> uint32_t {
					const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)W0, (int)(i & 63)), hi = (uint32_t)__builtin_amdgcn_readlane((int)W1, (int)(i & 63));
					return i < 64 ? lo : hi;
				};
				uint32_t s0, s1, s2, s3, s4;
				if (qi < 60) {
					s0 = (uint32_t)__builtin_amdgcn_readlane((int)W0, (int)qi); s1 = (uint32_t)__builtin_amdgcn_readlane((int)W0, (int)(qi + 1));
					s2 = (uint32_t)__builtin_amdgcn_readlane((int)W0, (int)(qi + 2)); s3 = (uint32_t)__builtin_amdgcn_readlane((int)W0, (int)(qi + 3));
					s4 = (uint32_t)__builtin_amdgcn_readlane((int)W0, (int)(qi + 4));
				} else { s0 = word(qi); s1 = word(qi + 1); s2 = word(qi + 2); s3 = word(qi + 3); s4 = word(qi + 4); }
				// this lane's 64 bits of the source: [pos + lane, pos + lane + 64)
				const uint32_t bo = sh + (uint32_t)lane, di = bo >> 5, r = bo & 31;        // di = 0..2
				const uint32_t a0 = di == 0 ? s0 : di == 1 ? s1 : s2;
				const uint32_t a1 = di == 0 ? s1 : di == 1 ? s2 : s3;
				const uint32_t w0 = __builtin_amdgcn_alignbit(a1, a0, r);
				const uint32_t el = sm.hl.fast[w0 & ((1u << LBITS) - 1)];
				if (lit_mode) {
					// a stretch of literals: the tokens are counted, nothing else
					const uint32_t lsym = el & 0xfff;
					const uint32_t ltl = (el && lsym < 256) ? el >> 12 : 0;
					uint32_t off;
					uint64_t starts;
					chain_by_lane(lane, ltl, starts, off);
					lit_mode = off > 63;
					const uint32_t cnt = (uint32_t)__builtin_popcountll(starts);
					if (!cnt || !nxz_size_fits(out, cnt, soft)) { lit_mode = false; continue; }
					if constexpr (KEEP)
						hook.lit((starts >> lane) & 1, out + __builtin_amdgcn_mbcnt_hi((uint32_t)(starts >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)starts, 0)), lsym);
					out += cnt;
					b.pos += off;
					continue;
				}
				const uint32_t a2 = di == 0 ? s2 : di == 1 ? s3 : s4;
				const uint32_t w1 = __builtin_amdgcn_alignbit(a2, a1, r);
				const uint32_t nb = el >> 12, sym = el & 0xfff;
				const bool islit = el && sym < 256;
				const bool islen = sym > 256 && sym < 257 + 29;
				uint32_t lbase, eb, dbase, ebd;
				len_params(islen ? sym - 257 : 0, lbase, eb);
				const uint32_t mlen = lbase + (__builtin_amdgcn_alignbit(w1, w0, nb) & ((1u << eb) - 1));
				const uint32_t o2 = nb + eb;                                               // <= 11 + 5
				const uint32_t ed = sm.hd.fast[__builtin_amdgcn_alignbit(w1, w0, o2) & ((1u << DBITS) - 1)];
				const uint32_t ds = ed & 0xfff;
				const bool okd = ed && ds < 30;
				dist_params(okd ? ds : 0, dbase, ebd);
				const uint32_t o3 = o2 + (ed >> 12);                                       // <= 16 + 9
				const uint32_t mdist = dbase + (__builtin_amdgcn_alignbit(w1, w0, o3) & ((1u << ebd) - 1));
				const uint32_t tl = islit ? nb : (islen && okd) ? o3 + ebd : 0;            // bits of the token; 0: not for this step
				const uint32_t ob = islit ? 1 : mlen;                                      // bytes it makes
				uint32_t off;
				uint64_t starts;
				chain_by_lane(lane, tl, starts, off);
				if (!starts) break;
				// how many bytes stand in front of each token: prefix sum of the byte counts over the token starts
				bool isstart = (starts >> lane) & 1;
				const uint32_t x = isstart ? ob : 0;
				uint32_t incl = x;
				incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x111, 0xf, 0xf, false);   // row_shr:1
				incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x112, 0xf, 0xf, false);   // row_shr:2
				incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x114, 0xf, 0xf, false);   // row_shr:4
				incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x118, 0xf, 0xf, false);   // row_shr:8
				incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x142, 0xa, 0xf, false);   // row_bcast:15
				incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x143, 0xc, 0xf, false);   // row_bcast:31
				// a token that does not fit the target, or a match that reaches in front of the history: the step ends
				// before it (the one-token path says what is wrong).  Once output and history make a window's worth every
				// distance of the format is legal: a scalar test spares the lanes theirs.
				const bool reach_all = (uint64_t)out + hist >= NXZ_SIZE_WINDOW;
				const uint64_t bad = __ballot(isstart && (!nxz_size_fits(out, incl, soft) ||
									  (!reach_all && !islit && !nxz_size_dist_ok(mdist, (uint64_t)out + (incl - x), hist))));
				if (bad) {
					const uint32_t first = (uint32_t)__builtin_ctzll(bad);
					starts &= (1ull << first) - 1;
					off = first;
					if (!starts) break;
				}
				if constexpr (KEEP) {
					// All literals of the step at once, then the matches in chain order (nxz_inflate.hip's order for a window
					// in LDS).  In a ring a literal written ahead of its turn may land on the byte, nearly 32 KiB back, that a
					// match in front of it still has to read: such a step (rare) goes token by token.
					const bool mine = (starts >> lane) & 1;
					const uint32_t opos = incl - x;
					const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, (int)(63 - __builtin_clzll(starts)));
					const uint64_t lits = __ballot(islit);
					const bool ordered = __ballot(mine && !islit && mdist + total > NXZ_SIZE_WINDOW) != 0;
					if (!ordered) hook.lit(mine && islit, out + opos, sym);
					uint64_t mm = ordered ? starts : starts & ~lits;
					while (mm) {
						const uint32_t l = (uint32_t)__builtin_ctzll(mm);
						mm &= mm - 1;
						if ((lits >> l) & 1) { hook.lit((uint32_t)lane == l, out + opos, sym); continue; }
						hook.match(out + (uint32_t)__builtin_amdgcn_readlane((int)opos, (int)l), (uint32_t)__builtin_amdgcn_readlane((int)mdist, (int)l),
							   (uint32_t)__builtin_amdgcn_readlane((int)ob, (int)l));
					}
				}
				out += (uint32_t)__builtin_amdgcn_readlane((int)incl, (int)(63 - __builtin_clzll(starts)));
				lit_mode = !(starts & ~__ballot(islit));                    // (nothing but literals: the next step may be the short one)
				b.pos += off;
			}
			// the step stopped at a token it leaves to the one-token path (or never ran)
			lit_mode = false;
			b.bb_sync();
			const uint64_t sym_start = b.pos;
			const uint32_t sfbt = (btype == 1 ? 0xa : 0xc) | bfinal;
			uint32_t nb;
			b.bb_fill();
			int sym = decode_sym<LBITS>(sm.hl, (uint32_t)b.bb, nb);
			if (sym < 0 || !b.have(nb)) {
				if (!b.have(sym < 0 ? 15 : nb)) { stop.sfbt = sfbt; stop.subc = (uint32_t)(b.total_bits - sym_start); break; }
				stop.cc = NXZ_CC_MISSING_CODE; break;
			}
			b.bb_drop(nb);
			if (sym < 256) {
				if (!fits_or_cut(1, sym_start, sfbt)) { stop.cc = NXZ_CC_TARGET_SPACE; break; }
				if constexpr (KEEP) hook.lit(lane == 0, out, (uint32_t)sym);
				out++;
			} else if (sym == 256) {
				if (bfinal) { stop.final_eob = 1; break; }
				state = 0;
			} else {
				sym -= 257;
				if (sym >= 29) { stop.cc = NXZ_CC_MISSING_CODE; break; }
				uint32_t lbase, eb;
				len_params((uint32_t)sym, lbase, eb);
				b.bb_fill();
				if (!b.have(eb)) { stop.sfbt = sfbt; stop.subc = (uint32_t)(b.total_bits - sym_start); break; }
				const uint32_t len = lbase + ((uint32_t)b.bb & ((1u << eb) - 1));
				b.bb_drop(eb);
				b.bb_fill();
				const int ds = decode_sym<DBITS>(sm.hd, (uint32_t)b.bb, nb);
				if (ds < 0 || !b.have(nb)) {
					if (!b.have(ds < 0 ? 15 : nb)) { stop.sfbt = sfbt; stop.subc = (uint32_t)(b.total_bits - sym_start); break; }
					stop.cc = NXZ_CC_INVALID_DIST; break;
				}
				if (ds >= 30) { stop.cc = NXZ_CC_INVALID_DIST; break; }
				b.bb_drop(nb);
				uint32_t dbase;
				dist_params((uint32_t)ds, dbase, eb);
				b.bb_fill();
				if (!b.have(eb)) { stop.sfbt = sfbt; stop.subc = (uint32_t)(b.total_bits - sym_start); break; }
				const uint32_t dist = dbase + ((uint32_t)b.bb & ((1u << eb) - 1));
				b.bb_drop(eb);
				if (!nxz_size_dist_ok(dist, out, hist)) { stop.cc = NXZ_CC_INVALID_DIST; break; }
				if (!fits_or_cut(len, sym_start, sfbt)) { stop.cc = NXZ_CC_TARGET_SPACE; break; }
				if constexpr (KEEP) hook.match(out, dist, len);
				out += len;
			}
		}
	}
	if (stop.final_eob) { stop.sfbt = 0; stop.subc = (uint32_t)(b.total_bits - b.pos); }
	stop.produced = out;
	end_bit = b.pos;
}

} // namespace nxzs
#endif
