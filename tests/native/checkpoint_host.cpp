// checkpoint_host.cpp -- TEST ONLY.  The rules of the checkpoint calls (power-gzip_amd/csrc/nxz_checkpoint.h), the code the device
// runs, compiled for the host.  The bit-walking is not here: a request hands the rules the block headers a walk would have
// found, or an index, and gets back what the rules make of it.  One request per line on stdin (numbers decimal):
//   job resume hist_len                                  -> "0" / "1"
//   rule span cp_cap N u_0 .. u_{N-1}                    -> "count k_0 u_0' k_1 u_1' ..." the stored checkpoints (slot, uoff) in order
//        the output bytes in front of the N block headers of a stream, in the walk's order
//   summary count cp_cap format hdr_len frame_status cc final_eob out_len want_windows have_output
//                                                        -> "status count format hdr_len out_len cc frame_status sentinel"
//   seg c0 c1 u0 u1                                      -> "src_begin src_end in_subc resume window_len out_len job_len"
//   valid src_len nidx cbit_0 .. uoff_0 ..               -> "0" / "1" (nxz_cp_index_ok)
//   good cc tpbc expected                                -> "0" / "1"
//   range nidx b e uoff_0 ..                             -> "status ub ue first last" (first / last: the segments of ub and ue - 1, 0 0 when empty)
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>
#include "nxz_checkpoint.h"

int main()
{
	static char line[1 << 20];
	while (fgets(line, sizeof line, stdin)) {
		std::istringstream in(line);
		std::string what;
		if (!(in >> what)) continue;
		std::vector<uint64_t> a;
		for (uint64_t v; in >> v;) a.push_back(v);
		auto need = [&](size_t n) { return a.size() >= n; };
		if (what == "job") {
			if (!need(2)) return 2;
			printf("%d\n", nxz_cp_job_ok((uint32_t)a[0], (uint32_t)a[1]) ? 1 : 0);
		} else if (what == "rule") {
			if (!need(3) || a.size() != 3 + a[2]) return 2;
			const uint64_t span = a[0];
			const uint32_t cp_cap = (uint32_t)a[1];
			nxz_cp_acc_t acc = nxz_cp_begin();
			std::string out;
			for (uint64_t i = 0; i < a[2]; i++) {
				const uint64_t u = a[3 + i];
				if (!nxz_cp_is_checkpoint(&acc, u, span)) continue;
				const uint32_t k = nxz_cp_add(&acc, u, cp_cap);
				if (k < cp_cap) out += " " + std::to_string(k) + " " + std::to_string(u);
			}
			printf("%u%s\n", acc.count, out.c_str());
		} else if (what == "summary") {
			if (!need(10)) return 2;
			nxz_cp_acc_t acc = nxz_cp_begin();
			acc.count = (uint32_t)a[0];
			const nxz_checkpoint_stream_t s = nxz_cp_summary(&acc, (uint32_t)a[1], (uint32_t)a[2], (uint32_t)a[3], (uint32_t)a[4], (uint32_t)a[5],
									 (uint32_t)a[6], a[7], a[8] != 0, a[9] != 0);
			printf("%u %u %u %u %" PRIu64 " %u %u %d\n", s.status, s.count, s.format, s.hdr_len, s.out_len, s.cc, s.frame_status,
			       nxz_cp_has_sentinel(s.status) ? 1 : 0);
		} else if (what == "seg") {
			if (!need(4)) return 2;
			printf("%" PRIu64 " %" PRIu64 " %u %u %u %" PRIu64 " %" PRIu64 "\n", nxz_cp_src_begin(a[0]), nxz_cp_src_end(a[1]), nxz_cp_in_subc(a[0]),
			       nxz_cp_resume(a[0]), nxz_cp_window_len(a[2]), nxz_cp_out_len(a[2], a[3]), nxz_cp_job_len(a[0], a[1], a[2]));
		} else if (what == "valid") {
			if (!need(2) || a.size() != 2 + 2 * a[1]) return 2;
			// (exact-size heap copies: AddressSanitizer sees a read behind either array)
			std::vector<uint64_t> cbit(a.begin() + 2, a.begin() + 2 + a[1]), uoff(a.begin() + 2 + a[1], a.end());
			printf("%d\n", nxz_cp_index_ok(cbit.data(), uoff.data(), a[1], a[0]) ? 1 : 0);
		} else if (what == "good") {
			if (!need(3)) return 2;
			printf("%d\n", nxz_cp_segment_good((uint32_t)a[0], (uint32_t)a[1], a[2]) ? 1 : 0);
		} else if (what == "range") {
			if (!need(3) || a.size() != 3 + a[0] || a[0] < 1) return 2;
			std::vector<uint64_t> uoff(a.begin() + 3, a.end());
			const uint64_t L = a[0] - 1;
			uint64_t ub, ue, first = 0, last = 0;
			const uint32_t st = nxz_cp_resolve(uoff.data(), L, a[1], a[2], &ub, &ue);
			if (ue > ub) { first = nxz_cp_segment_of(uoff.data(), L, ub); last = nxz_cp_segment_of(uoff.data(), L, ue - 1); }
			printf("%u %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", st, ub, ue, first, last);
		} else return 2;
	}
	return 0;
}
