// nxz_checkpoint_fine.h -- the rules of the fine checkpoint calls (nxz_batch_checkpoint_index_fine / nxz_checkpoint_read_ranges_fine,
// include/nxz_engine.h) as plain code that compiles for the device (nxz_checkpoint_fine.hip) and for the host
// (tests/native/checkpoint_fine_host.cpp).  What nxz_checkpoint.h says of an index, a segment and a range holds here as it stands;
// this file adds what a checkpoint INSIDE a block needs:
//   the budget   a segment makes at most span bytes: the checkpoint stands in front of the first byte-making token (a literal, a
//                match, every single byte of a stored block) that would carry the output beyond (uoff of the last checkpoint) + span;
//   the state    where in a block a checkpoint stands: the decoder's resume fields and, for a dynamic block, where in src the
//                block's table is -- the table is not copied into the index, the source is there at read time;
//   validity     what a state entry must satisfy before a kernel follows it into src or a table slot;
//   a segment    the job fields that differ from a coarse segment's, and the table slot's bytes.
#ifndef NXZ_CHECKPOINT_FINE_H
#define NXZ_CHECKPOINT_FINE_H
#include "nxz_checkpoint.h"

#define NXZ_CPF_SPAN_MIN 258u    /* the longest token: with a span of that or more a token always fits an empty segment */

/* ---- the budget ------------------------------------------------------------------------------------------------------------ */
NXZ_CP_HD inline bool nxz_cpf_span_ok(uint64_t span) { return span >= NXZ_CPF_SPAN_MIN; }
/* the output the segment in work may reach: (uoff of the last checkpoint) + span, never above cap -- the sum in 64 bits, the
 * answer in the walk's 32-bit field */
NXZ_CP_HD inline uint32_t nxz_cpf_budget(const nxz_cp_acc_t *a, uint64_t span, uint32_t cap)
{
	const uint64_t lim = span > ~0ull - a->last_uoff ? ~0ull : a->last_uoff + span;
	return lim < cap ? (uint32_t)lim : cap;
}
/* The walk (nxz_inflate_walk.h) applies the rule with this budget and nxz_size_fits: a token that does not fit the budget, while the
 * budget is below the real cap, gets a checkpoint in front of it (nxz_cp_add) and the budget is taken anew. */

/* ---- the state ------------------------------------------------------------------------------------------------------------- */
#define NXZ_CPF_SFBT_STORED 0x8u         /* | BFINAL; with rem */
#define NXZ_CPF_SFBT_FIXED 0xau
#define NXZ_CPF_SFBT_DYNAMIC 0xcu
NXZ_CP_HD inline uint32_t nxz_cpf_sfbt(uint32_t resume) { return (resume >> 16) & 15; }
NXZ_CP_HD inline uint32_t nxz_cpf_rem(uint32_t resume) { return resume & 0xffff; }
NXZ_CP_HD inline bool nxz_cpf_is_stored(uint32_t sfbt) { return (sfbt & 0xe) == NXZ_CPF_SFBT_STORED; }
NXZ_CP_HD inline bool nxz_cpf_is_dynamic(uint32_t sfbt) { return (sfbt & 0xe) == NXZ_CPF_SFBT_DYNAMIC; }
/* the entry of a checkpoint in front of a token: sfbt with BFINAL in bit 0, rem the bytes of a stored block still to come (else 0),
 * tbit / dhtlen where the dynamic block's table is (taken for a dynamic block only).  sfbt 0: at a block header, all zero. */
NXZ_CP_HD inline nxz_checkpoint_state_t nxz_cpf_state(uint32_t sfbt, uint32_t rem, uint64_t tbit, uint32_t dhtlen)
{
	nxz_checkpoint_state_t s = {};
	if (!sfbt) return s;
	s.resume = (nxz_cpf_is_stored(sfbt) ? rem & 0xffff : 0) | (sfbt & 15) << 16;
	if (nxz_cpf_is_dynamic(sfbt)) { s.tbit = tbit; s.dhtlen = dhtlen; }
	return s;
}

/* ---- validity -------------------------------------------------------------------------------------------------------------- */
/* the state of entry j (j < L) beside cbit[j]: entry 0 stands at a header; resume holds in_rembytecnt and in_sfbt and nothing else;
 * in_sfbt is 0 or 0x8..0xd; a stored checkpoint has bytes to come and stands at a byte boundary; only a dynamic one names a table,
 * of 1 .. 8 * NXZ_DHT_MAXSZ bits that begin behind a 3-bit header and end in front of the checkpoint */
NXZ_CP_HD inline bool nxz_cpf_state_ok(const nxz_checkpoint_state_t *s, uint64_t j, uint64_t cbit_j)
{
	const uint32_t sfbt = nxz_cpf_sfbt(s->resume), rem = nxz_cpf_rem(s->resume);
	if (s->resume >> 20) return false;
	if (j == 0 && s->resume != 0) return false;
	if (sfbt != 0 && (sfbt < 0x8 || sfbt > 0xd)) return false;
	if (nxz_cpf_is_stored(sfbt) ? (rem == 0 || (cbit_j & 7) != 0) : rem != 0) return false;
	if (nxz_cpf_is_dynamic(sfbt)) {
		if (s->dhtlen < 1 || s->dhtlen > 8 * NXZ_DHT_MAXSZ || s->tbit < 3) return false;
		if (s->tbit > cbit_j || s->dhtlen > cbit_j - s->tbit) return false;
	} else if (s->tbit != 0 || s->dhtlen != 0) return false;
	return true;
}
/* entry j of a fine index: nxz_cp_entry_ok and its state */
NXZ_CP_HD inline bool nxz_cpf_entry_ok(const uint64_t *cbit, const uint64_t *uoff, const nxz_checkpoint_state_t *state, uint64_t L, uint64_t j,
				       uint64_t src_len)
{
	return nxz_cp_entry_ok(cbit, uoff, L, j, src_len) && nxz_cpf_state_ok(&state[j], j, cbit[j]);
}
/* the whole index, one entry after the other (the host's form; the device checks a thread an entry) */
NXZ_CP_HD inline bool nxz_cpf_index_ok(const uint64_t *cbit, const uint64_t *uoff, const nxz_checkpoint_state_t *state, uint64_t nidx, uint64_t src_len)
{
	if (nidx < 2) return false;
	for (uint64_t j = 0; j + 1 < nidx; j++)
		if (!nxz_cpf_entry_ok(cbit, uoff, state, nidx - 1, j, src_len)) return false;
	return true;
}

/* ---- a segment's job: what differs from nxz_checkpoint.h's ----------------------------------------------------------------- */
/* resume: the state's fields and the unused bits of the first source byte */
NXZ_CP_HD inline uint32_t nxz_cpf_resume(const nxz_checkpoint_state_t *s, uint64_t cbit_k) { return s->resume | nxz_cp_resume(cbit_k); }
/* reserved: a token behind the segment's last -- whole inside the up to 7 bits that follow cbit[k + 1] in the last source byte --
 * does not fit the target of exactly the segment's output, and that must be a place to suspend (CC 3), not CC 13 */
NXZ_CP_HD inline uint32_t nxz_cpf_job_flags(void) { return NXZ_JOB_SUSPEND_WHEN_FULL; }
/* byte i of the segment's table slot: bits [tbit + 8 i, tbit + 8 i + 8) of src shifted to bit 0, what lies beyond dhtlen bits zero.
 * Reads src only where a bit of the table is: with nxz_cpf_state_ok and nxz_cp_entry_ok that is inside the source. */
NXZ_CP_HD inline uint8_t nxz_cpf_dht_byte(const uint8_t *src, uint64_t tbit, uint32_t dhtlen, uint32_t i)
{
	if (8ull * i >= dhtlen) return 0;
	const uint64_t first = tbit + 8ull * i, end = tbit + dhtlen;          /* the bits wanted: [first, min(first + 8, end)) */
	const uint32_t sh = (uint32_t)(first & 7);
	uint32_t v = src[first >> 3] >> sh;
	if (sh && ((first >> 3) + 1) * 8 < end) v |= (uint32_t)src[(first >> 3) + 1] << (8 - sh);
	const uint32_t left = dhtlen - 8 * i;
	if (left < 8) v &= (1u << left) - 1;
	return (uint8_t)v;
}
#endif
