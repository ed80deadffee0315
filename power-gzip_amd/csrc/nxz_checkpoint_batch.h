// nxz_checkpoint_batch.h -- the rules of the batched range read (nxz_batch_checkpoint_read_ranges, include/nxz_engine.h) as plain code
// that compiles for the device (nxz_checkpoint_batch.hip) and for the host (tests/native/checkpoint_batch_host.cpp).  What
// nxz_checkpoint.h and nxz_checkpoint_fine.h say of an index, a segment and a state entry holds here row by row; this file adds what
// a BATCH of indexes needs -- everything that decides where a kernel may read:
//   the layout   the index calls' own: entry k of row i is element i * (cp_cap + 1) + k of cbit / uoff / state, its window is slot
//                i * cp_cap + k.  The batch is read as ONE index of n_jobs * (cp_cap + 1) entries in that very order: the flat
//                entry IS the element, so cbit, state and the windows are used where they lie and only uoff gets a copy;
//   a row        its verdict: the stream's record and rule 5 (with state: the per-entry checks) against that job's src_len;
//   the bases    base[i] = the bytes the good rows in front of row i make; a row that is not good makes none;
//   the flat uoff  base[i] + uoff[i][k] for k <= count, base[i + 1] behind the sentinel and all over a row that is not good: it never
//                decreases, and what lies between one stream's sentinel and the next stream's checkpoint 0 is a run of empty
//                members, which hold nothing (nxz_bgzf_range.h) -- no range reaches a segment outside its own stream;
//   a range      (job, begin, end) -> [base[job] + begin, base[job] + end) of the flat index, or why not.
#ifndef NXZ_CHECKPOINT_BATCH_H
#define NXZ_CHECKPOINT_BATCH_H
#include "nxz_checkpoint_fine.h"

/* ---- the layout ------------------------------------------------------------------------------------------------------------ */
NXZ_CP_HD inline uint64_t nxz_cpb_stride(uint32_t cp_cap) { return (uint64_t)cp_cap + 1; }
/* a batch the call takes: the flat index has fewer than 2^32 entries (the map's lists are 32-bit), so every product below fits */
NXZ_CP_HD inline bool nxz_cpb_shape_ok(uint64_t n_jobs, uint32_t cp_cap)
{
	return cp_cap != 0 && n_jobs < (1ull << 31) && n_jobs * nxz_cpb_stride(cp_cap) < (1ull << 32);
}
/* the entries of the flat index; its segments (the map's L) are one fewer */
NXZ_CP_HD inline uint64_t nxz_cpb_entries(uint64_t n_jobs, uint32_t cp_cap) { return n_jobs * nxz_cpb_stride(cp_cap); }
NXZ_CP_HD inline uint64_t nxz_cpb_entry(uint64_t row, uint32_t k, uint32_t cp_cap) { return row * nxz_cpb_stride(cp_cap) + k; }
NXZ_CP_HD inline uint64_t nxz_cpb_row_of(uint64_t e, uint32_t cp_cap) { return e / nxz_cpb_stride(cp_cap); }
NXZ_CP_HD inline uint32_t nxz_cpb_k_of(uint64_t e, uint32_t cp_cap) { return (uint32_t)(e % nxz_cpb_stride(cp_cap)); }
/* the window slot of checkpoint k < cp_cap of a row, and its first byte in `windows` (below 2^32 slots: below 2^47 bytes) */
NXZ_CP_HD inline uint64_t nxz_cpb_window_slot(uint64_t row, uint32_t k, uint32_t cp_cap) { return row * cp_cap + k; }
NXZ_CP_HD inline uint64_t nxz_cpb_window_at(uint64_t row, uint32_t k, uint32_t cp_cap) { return nxz_cpb_window_slot(row, k, cp_cap) * NXZ_CP_WINDOW; }

/* ---- a row's verdict ------------------------------------------------------------------------------------------------------- */
/* the stream's record: a whole index (NXZ_CPS_OK: sentinel and windows are there) of 1 .. cp_cap checkpoints over a source that is there */
NXZ_CP_HD inline bool nxz_cpb_head_ok(uint32_t status, uint32_t count, uint32_t cp_cap, bool have_src)
{
	return status == NXZ_CPS_OK && count >= 1 && count <= cp_cap && have_src;
}
/* entry k < count of a row whose record is good: rule 5 over the row's count checkpoints, and its state where there is one.
 * cbit / uoff / state: the ROW's part (count + 1 entries are read at most, count <= cp_cap) */
NXZ_CP_HD inline bool nxz_cpb_entry_ok(const uint64_t *cbit, const uint64_t *uoff, const nxz_checkpoint_state_t *state, uint32_t count, uint32_t k,
				       uint64_t src_len)
{
	return state ? nxz_cpf_entry_ok(cbit, uoff, state, count, k, src_len) : nxz_cp_entry_ok(cbit, uoff, count, k, src_len);
}
/* the whole row, one entry after the other (the host's form; the device checks a thread an entry) */
NXZ_CP_HD inline bool nxz_cpb_row_ok(uint32_t status, uint32_t count, uint32_t cp_cap, bool have_src, const uint64_t *cbit, const uint64_t *uoff,
				     const nxz_checkpoint_state_t *state, uint64_t src_len)
{
	if (!nxz_cpb_head_ok(status, count, cp_cap, have_src)) return false;
	for (uint32_t k = 0; k < count; k++)
		if (!nxz_cpb_entry_ok(cbit, uoff, state, count, k, src_len)) return false;
	return true;
}

/* ---- the bases ------------------------------------------------------------------------------------------------------------- */
/* what a row adds to the bases behind it: the sentinel's uoff of a good row (the out_len the single-stream calls go by), else nothing */
NXZ_CP_HD inline uint64_t nxz_cpb_extent(bool good, const uint64_t *uoff_row, uint32_t count) { return good ? uoff_row[count] : 0; }
/* A good row's extent is at most count * (2^32 - 1): rule 5 bounds every segment's output.  Over a batch nxz_cpb_shape_ok takes that
 * is below 2^32 * 2^32: the sum of all extents -- every base, every flat uoff, every mapped range -- fits 64 bits, no check needed. */
NXZ_CP_HD inline uint64_t nxz_cpb_extent_max(uint32_t count) { return (uint64_t)count * 0xffffffffull; }
/* base[0 .. n_jobs] from the rows' extents, one after the other (the host's form; the device scans) */
NXZ_CP_HD inline void nxz_cpb_bases(const uint64_t *extent, uint64_t n_jobs, uint64_t *base)
{
	base[0] = 0;
	for (uint64_t i = 0; i < n_jobs; i++) base[i + 1] = base[i] + extent[i];
}

/* ---- the flat uoff --------------------------------------------------------------------------------------------------------- */
/* entry k <= cp_cap of a row with bases base_row / base_next: nothing of a row that is not good is read */
NXZ_CP_HD inline uint64_t nxz_cpb_flat_uoff(bool good, uint64_t base_row, uint64_t base_next, const uint64_t *uoff_row, uint32_t count, uint32_t k)
{
	if (!good) return base_row;                                           /* (== base_next) */
	return k <= count ? base_row + uoff_row[k] : base_next;
}
/* is flat segment e one of a good row's own (k < count)?  What the map hands to the stage kernel always is; the kernel asks anyway.
 * bad: a word a row, 0 for a good one; count: that row's */
NXZ_CP_HD inline bool nxz_cpb_segment_ok(uint64_t e, uint64_t n_jobs, uint32_t cp_cap, const uint32_t *bad, const nxz_checkpoint_stream_t *streams)
{
	const uint64_t row = nxz_cpb_row_of(e, cp_cap);
	if (row >= n_jobs || bad[row]) return false;
	return nxz_cpb_k_of(e, cp_cap) < streams[row].count && streams[row].count <= cp_cap;
}

/* ---- a range --------------------------------------------------------------------------------------------------------------- */
/* (job, begin, end) onto the flat index: [*fb, *fe), or [0, 0) with the reason.  bad[n_jobs], base[n_jobs + 1] */
NXZ_CP_HD inline uint32_t nxz_cpb_map_range(uint32_t job, uint64_t begin, uint64_t end, uint64_t n_jobs, const uint32_t *bad, const uint64_t *base,
					    uint64_t *fb, uint64_t *fe)
{
	*fb = *fe = 0;
	if (job >= n_jobs || bad[job]) return NXZ_RANGE_BAD_STREAM;
	const uint64_t b0 = base[job], extent = base[job + 1] - b0;
	if (begin > end || end > extent) return NXZ_RANGE_OUT_OF_BOUNDS;
	*fb = b0 + begin; *fe = b0 + end;
	return NXZ_RANGE_OK;
}
#endif
