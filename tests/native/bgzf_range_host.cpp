// bgzf_range_host.cpp -- TEST ONLY.  The mapping of BGZF read ranges onto a member index
// (power-gzip_amd/csrc/nxz_bgzf_range.h, the code the device's range_map_kernel runs) compiled for the host.
// Reads cases from stdin, all little-endian uint64:
//   L, coff[0..L], uoff[0..L], nq, then nq x (kind, begin, end)
// and prints a line per query: "status ub ue first last" (first = last = -1 for a range with no bytes).
// Every index sits in an allocation of exactly its length (run under AddressSanitizer).
#include <cstdint>
#include <cstdio>
#include <vector>
#include "nxz_bgzf_range.h"

static bool rd(uint64_t *v) { return fread(v, 8, 1, stdin) == 1; }

int main()
{
	for (uint64_t L; rd(&L);) {
		std::vector<uint64_t> coff(L + 1), uoff(L + 1);
		for (auto &v : coff) if (!rd(&v)) return 2;
		for (auto &v : uoff) if (!rd(&v)) return 2;
		uint64_t nq;
		if (!rd(&nq)) return 2;
		for (uint64_t i = 0; i < nq; i++) {
			uint64_t kind, b, e, ub, ue;
			if (!rd(&kind) || !rd(&b) || !rd(&e)) return 2;
			const uint32_t st = nxz_bgzf_resolve(coff.data(), uoff.data(), L, (int)kind, b, e, &ub, &ue);
			long long first = -1, last = -1;
			if (ue > ub) {
				first = (long long)nxz_bgzf_member_of(uoff.data(), L, ub);
				last = (long long)nxz_bgzf_member_of(uoff.data(), L, ue - 1);
			}
			printf("%u %llu %llu %lld %lld\n", st, (unsigned long long)ub, (unsigned long long)ue, first, last);
		}
	}
	return 0;
}
