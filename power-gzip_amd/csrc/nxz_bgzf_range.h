// nxz_bgzf_range.h -- the mapping of a BGZF read range onto the member index, as plain code that compiles for the device
// (nxz_bgzf.hip: a thread a range) and for the host (tests/native/bgzf_range_host.cpp).
//
// The index (include/nxz_engine.h, nxz_bgzf_index): coff[0..L] / uoff[0..L], member j holds compressed bytes
// [coff[j], coff[j+1]) and uncompressed bytes [uoff[j], uoff[j+1]).  Members may be empty (the 28-byte end marker,
// empty members inside), so uoff may repeat; coff never does.
//   member of byte u   the last j < L with uoff[j] <= u (upper_bound - 1): the one non-empty member that holds u
//                      whenever uoff[0] <= u < uoff[L], however many empty members share its start
//   virtual offset v   coff[j] = v >> 16 for some j <= L (j = L: the end of the data), within = v & 0xffff <= ISIZE of
//                      member j (== ISIZE: its end, as htslib allows) -> uoff[j] + within
//   range [b, e)       b > e, b < uoff[0] or e > uoff[L]: out of bounds; b == e: empty and fine
#ifndef NXZ_BGZF_RANGE_H
#define NXZ_BGZF_RANGE_H
#include <stdint.h>
#include "../../include/nxz_engine.h"

#if defined(__HIPCC__)
#define NXZ_RHD __host__ __device__
#else
#define NXZ_RHD
#endif

// the number of entries of a[0..n) that are <= v (a sorted): upper_bound; the last such entry is that minus one
NXZ_RHD inline uint64_t nxz_bgzf_upper(const uint64_t *a, uint64_t n, uint64_t v)
{
	uint64_t lo = 0, hi = n;
	while (lo < hi) {
		const uint64_t m = lo + ((hi - lo) >> 1);
		if (a[m] <= v) lo = m + 1;
		else hi = m;
	}
	return lo;
}

// the member that holds uncompressed byte u; the caller has checked uoff[0] <= u < uoff[L]
NXZ_RHD inline uint64_t nxz_bgzf_member_of(const uint64_t *uoff, uint64_t L, uint64_t u) { return nxz_bgzf_upper(uoff, L, u) - 1; }

// virtual offset -> uncompressed offset; NXZ_RANGE_OK or NXZ_RANGE_BAD_VOFFSET
NXZ_RHD inline uint32_t nxz_bgzf_voff_to_uoff(const uint64_t *coff, const uint64_t *uoff, uint64_t L, uint64_t voff, uint64_t *u)
{
	const uint64_t c = voff >> 16, within = voff & 0xffff;
	const uint64_t k = nxz_bgzf_upper(coff, L + 1, c);
	if (k == 0 || coff[k - 1] != c) return NXZ_RANGE_BAD_VOFFSET;
	const uint64_t j = k - 1, isize = j < L ? uoff[j + 1] - uoff[j] : 0;
	if (within > isize) return NXZ_RANGE_BAD_VOFFSET;
	*u = uoff[j] + within;
	return NXZ_RANGE_OK;
}

// range [b, e) of the given kind -> [*ub, *ue) in uncompressed offsets (0, 0 unless NXZ_RANGE_OK)
NXZ_RHD inline uint32_t nxz_bgzf_resolve(const uint64_t *coff, const uint64_t *uoff, uint64_t L, int kind, uint64_t b, uint64_t e,
					 uint64_t *ub, uint64_t *ue)
{
	*ub = *ue = 0;
	if (kind == NXZ_RANGE_VOFF) {
		if (nxz_bgzf_voff_to_uoff(coff, uoff, L, b, &b) != NXZ_RANGE_OK || nxz_bgzf_voff_to_uoff(coff, uoff, L, e, &e) != NXZ_RANGE_OK)
			return NXZ_RANGE_BAD_VOFFSET;
	}
	if (b > e || b < uoff[0] || e > uoff[L]) return NXZ_RANGE_OUT_OF_BOUNDS;
	*ub = b; *ue = e;
	return NXZ_RANGE_OK;
}

#endif
