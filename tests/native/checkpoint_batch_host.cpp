// checkpoint_batch_host.cpp -- TEST ONLY.  The rules of the batched range read (power-gzip_amd/csrc/nxz_checkpoint_batch.h), the code
// the device runs, compiled for the host.  Every array a request brings is copied to a heap block of exactly its size, so that
// AddressSanitizer sees a read behind any of them.  One request per line on stdin (numbers decimal, up to 2^64 - 1):
//   shape n_jobs cp_cap                     -> "0" / "1" (nxz_cpb_shape_ok)
//   slot row k cp_cap                       -> "entry row_of k_of window_slot window_at"
//   extmax count                            -> nxz_cpb_extent_max
//   row status count cp_cap have_src src_len with_state N cbit_0 .. uoff_0 .. [(tbit resume dhtlen)_0 ..]   (N entries of each)
//                                           -> "0" / "1" (nxz_cpb_row_ok)
//   map job begin end n_jobs bad_0 .. base_0 ..  (n_jobs words, n_jobs + 1 bases)   -> "status fb fe"
//   batch n_jobs cp_cap n with_state, then per row "status count have_src src_len", then cbit and uoff (n_jobs * (cp_cap + 1) each),
//        with_state: as many (tbit resume dhtlen), then n ranges "job begin end"
//        -> what the kernels make of it, in their order: "bad.. base.. fuoff.. seg.. (status fb fe).."  (seg: nxz_cpb_segment_ok of
//           every flat segment)
#include <cinttypes>
#include <cstdio>
#include <sstream>
#include <string>
#include <vector>
#include "nxz_checkpoint_batch.h"

static std::vector<nxz_checkpoint_state_t> states(const std::vector<uint64_t> &a, size_t at, size_t n)
{
	std::vector<nxz_checkpoint_state_t> st(n);
	for (size_t j = 0; j < n; j++) { st[j].tbit = a[at + 3 * j]; st[j].resume = (uint32_t)a[at + 3 * j + 1]; st[j].dhtlen = (uint32_t)a[at + 3 * j + 2]; }
	return st;
}

int main()
{
	static char line[1 << 22];
	while (fgets(line, sizeof line, stdin)) {
		std::istringstream in(line);
		std::string what;
		if (!(in >> what)) continue;
		std::vector<uint64_t> a;
		for (uint64_t v; in >> v;) a.push_back(v);
		auto need = [&](size_t n) { return a.size() >= n; };
		if (what == "shape") {
			if (!need(2)) return 2;
			printf("%d\n", nxz_cpb_shape_ok(a[0], (uint32_t)a[1]) ? 1 : 0);
		} else if (what == "slot") {
			if (!need(3)) return 2;
			const uint32_t k = (uint32_t)a[1], cap = (uint32_t)a[2];
			const uint64_t e = nxz_cpb_entry(a[0], k, cap);
			printf("%" PRIu64 " %" PRIu64 " %u %" PRIu64 " %" PRIu64 "\n", e, nxz_cpb_row_of(e, cap), nxz_cpb_k_of(e, cap), nxz_cpb_window_slot(a[0], k, cap),
			       nxz_cpb_window_at(a[0], k, cap));
		} else if (what == "extmax") {
			if (!need(1)) return 2;
			printf("%" PRIu64 "\n", nxz_cpb_extent_max((uint32_t)a[0]));
		} else if (what == "row") {
			if (!need(7)) return 2;
			const size_t n = (size_t)a[6];
			const bool with_state = a[5] != 0;
			if (a.size() != 7 + (with_state ? 5 : 2) * n) return 2;
			std::vector<uint64_t> cbit(a.begin() + 7, a.begin() + 7 + n), uoff(a.begin() + 7 + n, a.begin() + 7 + 2 * n);
			std::vector<nxz_checkpoint_state_t> st = states(a, 7 + 2 * n, with_state ? n : 0);
			printf("%d\n", nxz_cpb_row_ok((uint32_t)a[0], (uint32_t)a[1], (uint32_t)a[2], a[3] != 0, cbit.data(), uoff.data(), with_state ? st.data() : nullptr, a[4]) ? 1 : 0);
		} else if (what == "map") {
			if (!need(4) || a.size() != 4 + 2 * a[3] + 1) return 2;
			const size_t nj = (size_t)a[3];
			std::vector<uint32_t> bad(a.begin() + 4, a.begin() + 4 + nj);
			std::vector<uint64_t> base(a.begin() + 4 + nj, a.end());
			uint64_t fb, fe;
			const uint32_t st = nxz_cpb_map_range((uint32_t)a[0], a[1], a[2], nj, bad.data(), base.data(), &fb, &fe);
			printf("%u %" PRIu64 " %" PRIu64 "\n", st, fb, fe);
		} else if (what == "batch") {
			if (!need(4)) return 2;
			const size_t nj = (size_t)a[0], n = (size_t)a[2];
			const uint32_t cap = (uint32_t)a[1];
			const bool with_state = a[3] != 0;
			if (!nxz_cpb_shape_ok(nj, cap) || nj == 0) return 2;
			const size_t entries = (size_t)nxz_cpb_entries(nj, cap), at_rows = 4, at_cbit = at_rows + 4 * nj, at_uoff = at_cbit + entries, at_state = at_uoff + entries,
				     at_ranges = at_state + (with_state ? 3 * entries : 0);
			if (a.size() != at_ranges + 3 * n) return 2;
			std::vector<nxz_checkpoint_stream_t> streams(nj);
			std::vector<uint64_t> cbit(a.begin() + at_cbit, a.begin() + at_uoff), uoff(a.begin() + at_uoff, a.begin() + at_state);
			std::vector<nxz_checkpoint_state_t> st = states(a, at_state, with_state ? entries : 0);
			std::vector<uint32_t> bad(nj);
			std::vector<uint64_t> extent(nj), base(nj + 1), fuoff(entries);
			for (size_t i = 0; i < nj; i++) {                                   // rows_kernel, a row at a time
				streams[i] = nxz_checkpoint_stream_t();
				streams[i].status = (uint32_t)a[at_rows + 4 * i]; streams[i].count = (uint32_t)a[at_rows + 4 * i + 1];
				const size_t e0 = (size_t)nxz_cpb_entry(i, 0, cap);
				bad[i] = !nxz_cpb_row_ok(streams[i].status, streams[i].count, cap, a[at_rows + 4 * i + 2] != 0, cbit.data() + e0, uoff.data() + e0,
							 with_state ? st.data() + e0 : nullptr, a[at_rows + 4 * i + 3]);
				extent[i] = nxz_cpb_extent(!bad[i], uoff.data() + e0, bad[i] ? 0 : streams[i].count);   // base_kernel
			}
			nxz_cpb_bases(extent.data(), nj, base.data());
			std::string out;
			for (size_t i = 0; i < nj; i++) out += std::to_string(bad[i]) + " ";
			for (size_t i = 0; i <= nj; i++) out += std::to_string(base[i]) + " ";
			for (size_t e = 0; e < entries; e++) {                              // flat_kernel
				const size_t row = (size_t)nxz_cpb_row_of(e, cap);
				fuoff[e] = nxz_cpb_flat_uoff(!bad[row], base[row], base[row + 1], uoff.data() + nxz_cpb_entry(row, 0, cap), bad[row] ? 0 : streams[row].count,
							     nxz_cpb_k_of(e, cap));
				out += std::to_string(fuoff[e]) + " ";
			}
			for (size_t e = 0; e + 1 < entries; e++) out += std::to_string(nxz_cpb_segment_ok(e, nj, cap, bad.data(), streams.data()) ? 1 : 0) + " ";
			for (size_t r = 0; r < n; r++) {
				uint64_t fb, fe;
				const uint32_t s = nxz_cpb_map_range((uint32_t)a[at_ranges + 3 * r], a[at_ranges + 3 * r + 1], a[at_ranges + 3 * r + 2], nj, bad.data(), base.data(), &fb, &fe);
				out += std::to_string(s) + " " + std::to_string(fb) + " " + std::to_string(fe) + " ";
			}
			printf("%s\n", out.c_str());
		} else return 2;
	}
	return 0;
}
