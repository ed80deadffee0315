// nxz_checkpoint_build.h -- the rules of the one-pass index build (nxz_batch_checkpoint_build, include/nxz_engine.h) as plain code that
// compiles for the device (nxz_checkpoint_build.hip) and for the host (tests/native/checkpoint_build_host.cpp).  Which tokens get a
// checkpoint, what an entry and a stream's record hold: nxz_checkpoint.h and nxz_checkpoint_fine.h, as they stand.  This file adds
// what keeping the last 32 KiB of output in a ring needs:
//   the ring     output byte u lives at ring position u mod 32768;
//   a run        len bytes of output from byte u on (a stored run, a match's target or source) are one piece of the ring, or two
//                around the wrap;
//   the dump     the window of a checkpoint at u -- the min(u, 32768) bytes in front of u, oldest first -- as such a run;
//   a match      byte i of a copy of len bytes from dist back comes from byte i mod dist of the dist bytes in front of the target
//                (dist < len: the copy feeds on itself), the remainder without a division.
#ifndef NXZ_CHECKPOINT_BUILD_H
#define NXZ_CHECKPOINT_BUILD_H
#include "nxz_checkpoint.h"

#define NXZ_CB_RING NXZ_CP_WINDOW        /* bytes of the ring: a power of two, the window of the format */
#define NXZ_CB_MASK (NXZ_CB_RING - 1u)

/* ---- the ring -------------------------------------------------------------------------------------------------------------- */
/* where output byte u lives (u in 32 bits as the walk counts it; a difference that wrapped below 0 lands right as well) */
NXZ_CP_HD inline uint32_t nxz_cb_ring_pos(uint64_t u) { return (uint32_t)u & NXZ_CB_MASK; }

/* ---- a run of len bytes from output byte u on (len <= 32768) --------------------------------------------------------------- */
/* the bytes of it that lie in front of the wrap: the first piece is ring [nxz_cb_ring_pos(u), + that), the second ring [0, len - that) */
NXZ_CP_HD inline uint32_t nxz_cb_first_piece(uint64_t u, uint32_t len)
{
	const uint32_t room = NXZ_CB_RING - nxz_cb_ring_pos(u);
	return len < room ? len : room;
}
typedef struct nxz_cb_pieces {
	uint32_t start[2], len[2];       /* ring [start[k], start[k] + len[k]), k = 0 first; len[1] = 0: no wrap; start[1] = 0 */
} nxz_cb_pieces_t;
NXZ_CP_HD inline nxz_cb_pieces_t nxz_cb_run(uint64_t u, uint32_t len)
{
	nxz_cb_pieces_t p;
	p.start[0] = nxz_cb_ring_pos(u); p.len[0] = nxz_cb_first_piece(u, len);
	p.start[1] = 0; p.len[1] = len - p.len[0];
	return p;
}
/* a run longer than the ring leaves its last 32768 bytes: the bytes of it to skip */
NXZ_CP_HD inline uint64_t nxz_cb_run_skip(uint64_t n) { return n > NXZ_CB_RING ? n - NXZ_CB_RING : 0; }

/* ---- the dump -------------------------------------------------------------------------------------------------------------- */
/* the window of a checkpoint with u bytes of output in front of it: w = nxz_cp_window_len(u) bytes from output byte u - w on, to
 * the start of the checkpoint's slot */
NXZ_CP_HD inline nxz_cb_pieces_t nxz_cb_dump(uint64_t u)
{
	const uint32_t w = nxz_cp_window_len(u);
	return nxz_cb_run(u - w, w);
}

/* ---- a match --------------------------------------------------------------------------------------------------------------- */
/* i mod dist for i < 320 and dist < 259 (a copy that feeds on itself: dist < len <= 258) by one multiplication: m is the
 * rounded-up reciprocal in 20 bits, computed once a match; the quotient is exact while i / 2^20 < 1 / dist */
NXZ_CP_HD inline uint32_t nxz_cb_recip(uint32_t dist) { return (1u << 20) / dist + 1; }
NXZ_CP_HD inline uint32_t nxz_cb_mod(uint32_t i, uint32_t dist, uint32_t m) { return i - ((i * m) >> 20) * dist; }
/* the output byte that byte i of a match of len bytes at `at`, dist back, is a copy of: always in front of `at` */
NXZ_CP_HD inline uint64_t nxz_cb_match_src(uint64_t at, uint32_t dist, uint32_t len, uint32_t i)
{
	return at - dist + (dist < len ? nxz_cb_mod(i, dist, nxz_cb_recip(dist)) : i);
}
#endif
