// checkpoint_fine_host.cpp -- TEST ONLY.  The rules of the fine checkpoint calls (power-gzip_amd/csrc/nxz_checkpoint_fine.h), the code
// the device runs, compiled for the host.  The bit-walking is not here: a request hands the rules the tokens a walk would have
// found, or an index, and gets back what the rules make of it.  One request per line on stdin (numbers decimal):
//   span s                                               -> "0" / "1" (nxz_cpf_span_ok)
//   budget last_uoff span cap                            -> the budget (with count 1)
//   rule span cp_cap N n_0 c_0 .. n_{N-1} c_{N-1}        -> "count k_1 u_1 k_2 u_2 ..." the stored checkpoints behind checkpoint 0
//        the tokens of a stream in the walk's order: c_i tokens of n_i bytes each (a stored run: n 1, c its bytes), taken the way the
//        walk takes them: nxz_size_fits against nxz_cpf_budget, a cut and a new budget where a token does not fit
//   state sfbt rem tbit dhtlen                           -> "tbit resume dhtlen"
//   valid src_len nidx cbit_0 .. uoff_0 .. (tbit resume dhtlen)_0 ..   -> "0" / "1" (nxz_cpf_index_ok)
//   job tbit resume dhtlen cbit                          -> "resume flags"
//   dht tbit dhtlen N b_0 .. b_{N-1}                     -> the NXZ_DHT_MAXSZ + 4 bytes of the table slot over a source of N bytes
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>
#include "nxz_checkpoint_fine.h"
#include "nxz_size.h"

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
		if (what == "span") {
			if (!need(1)) return 2;
			printf("%d\n", nxz_cpf_span_ok(a[0]) ? 1 : 0);
		} else if (what == "budget") {
			if (!need(3)) return 2;
			nxz_cp_acc_t acc = nxz_cp_begin();
			(void)nxz_cp_add(&acc, a[0], 1);
			printf("%u\n", nxz_cpf_budget(&acc, a[1], (uint32_t)a[2]));
		} else if (what == "rule") {
			if (!need(3) || a.size() != 3 + 2 * a[2]) return 2;
			const uint64_t span = a[0];
			const uint32_t cp_cap = (uint32_t)a[1];
			nxz_cp_acc_t acc = nxz_cp_begin();
			(void)nxz_cp_add(&acc, 0, cp_cap);                                  // checkpoint 0: the first header
			const uint32_t cap = 0xffffffffu;                                   // (the index kernel's: no limit)
			uint32_t soft = nxz_cpf_budget(&acc, span, cap);
			std::string out;
			uint64_t u = 0;
			for (uint64_t i = 0; i < a[2]; i++) {
				const uint32_t n = (uint32_t)a[3 + 2 * i];
				for (uint64_t c = a[4 + 2 * i]; c; c--, u += n) {
					// the walk's form (nxz_inflate_walk.h, fits_or_cut): the token against the budget; a cut where the budget is not the cap
					if (nxz_size_fits((uint32_t)u, n, soft)) continue;
					if (soft >= cap) return 3;                                     // (the real cap: the requests here never reach it)
					const uint32_t k = nxz_cp_add(&acc, u, cp_cap);
					if (k < cp_cap) out += " " + std::to_string(k) + " " + std::to_string(u);
					soft = nxz_cpf_budget(&acc, span, cap);
					if (!nxz_size_fits((uint32_t)u, n, soft)) return 3;           // (span >= 258: a token fits an empty segment)
				}
			}
			printf("%u%s\n", acc.count, out.c_str());
		} else if (what == "state") {
			if (!need(4)) return 2;
			const nxz_checkpoint_state_t s = nxz_cpf_state((uint32_t)a[0], (uint32_t)a[1], a[2], (uint32_t)a[3]);
			printf("%" PRIu64 " %u %u\n", s.tbit, s.resume, s.dhtlen);
		} else if (what == "valid") {
			if (!need(2) || a.size() != 2 + 5 * a[1]) return 2;
			const size_t n = (size_t)a[1];
			// (exact-size heap copies: AddressSanitizer sees a read behind any of the arrays)
			std::vector<uint64_t> cbit(a.begin() + 2, a.begin() + 2 + n), uoff(a.begin() + 2 + n, a.begin() + 2 + 2 * n);
			std::vector<nxz_checkpoint_state_t> st(n);
			for (size_t j = 0; j < n; j++) { st[j].tbit = a[2 + 2 * n + 3 * j]; st[j].resume = (uint32_t)a[3 + 2 * n + 3 * j]; st[j].dhtlen = (uint32_t)a[4 + 2 * n + 3 * j]; }
			printf("%d\n", nxz_cpf_index_ok(cbit.data(), uoff.data(), st.data(), n, a[0]) ? 1 : 0);
		} else if (what == "job") {
			if (!need(4)) return 2;
			nxz_checkpoint_state_t s;
			s.tbit = a[0]; s.resume = (uint32_t)a[1]; s.dhtlen = (uint32_t)a[2];
			printf("%u %u\n", nxz_cpf_resume(&s, a[3]), nxz_cpf_job_flags());
		} else if (what == "dht") {
			if (!need(3) || a.size() != 3 + a[2]) return 2;
			std::vector<uint8_t> src(a.begin() + 3, a.end());                   // (exact size: a read behind the source is seen)
			std::string out;
			for (uint32_t i = 0; i < NXZ_DHT_MAXSZ + 4; i++) out += (i ? " " : "") + std::to_string(nxz_cpf_dht_byte(src.data(), a[0], (uint32_t)a[1], i));
			printf("%s\n", out.c_str());
		} else return 2;
	}
	return 0;
}
