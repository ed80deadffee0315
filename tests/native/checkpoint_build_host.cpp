// checkpoint_build_host.cpp -- TEST ONLY.  The rules of the one-pass index build (power-gzip_amd/csrc/nxz_checkpoint_build.h), the code
// the device runs, compiled for the host.  One request per line on stdin (numbers decimal):
//   pos u                      -> the ring position of output byte u
//   run u len                  -> "start0 len0 start1 len1": len bytes from output byte u on as pieces of the ring
//   dump u                     -> the same for the window of a checkpoint with u bytes in front of it
//   skip n                     -> the bytes of a run of n that the ring no longer holds
//   src at dist len i          -> the output byte that byte i of the match is a copy of
//   mods                       -> "1" when nxz_cb_mod is i % dist for every dist < 259 and i < 320
//   ring N op ...              -> a ring of 32768 bytes driven through the rules: the ops are  s u len seed  (a stored run of
//                                 bytes seed + k at u),  m at dist len  (a match),  d u  (a dump: prints the sum of byte * (index + 1)
//                                 over the window and the window's length)
#include <cinttypes>
#include <cstdio>
#include <sstream>
#include <string>
#include <vector>
#include "nxz_checkpoint_build.h"

int main()
{
	static char line[1 << 20];
	while (fgets(line, sizeof line, stdin)) {
		std::istringstream in(line);
		std::string what;
		if (!(in >> what)) continue;
		if (what == "ring") {
			std::vector<uint8_t> ring(NXZ_CB_RING);                              // (exact size: a position behind the ring is seen)
			std::string op, out;
			while (in >> op) {
				uint64_t a, b, c;
				if (op == "s") {
					if (!(in >> a >> b >> c)) return 2;
					const uint64_t skip = nxz_cb_run_skip(b);
					const nxz_cb_pieces_t p = nxz_cb_run(a + skip, (uint32_t)(b - skip));
					uint64_t k = skip;
					for (int q = 0; q < 2; q++)
						for (uint32_t i = 0; i < p.len[q]; i++, k++) ring.at(p.start[q] + i) = (uint8_t)(c + k);
				} else if (op == "m") {
					if (!(in >> a >> b >> c)) return 2;
					std::vector<uint8_t> v(c);                                     // all loads, then all stores: the device's order
					for (uint32_t i = 0; i < c; i++) v[i] = ring.at(nxz_cb_ring_pos(nxz_cb_match_src(a, (uint32_t)b, (uint32_t)c, i)));
					for (uint32_t i = 0; i < c; i++) ring.at(nxz_cb_ring_pos(a + i)) = v[i];
				} else if (op == "d") {
					if (!(in >> a)) return 2;
					const nxz_cb_pieces_t p = nxz_cb_dump(a);
					uint64_t sum = 0, k = 0;
					for (int q = 0; q < 2; q++)
						for (uint32_t i = 0; i < p.len[q]; i++, k++) sum += (uint64_t)ring.at(p.start[q] + i) * (k + 1);
					out += (out.empty() ? "" : " ") + std::to_string(sum) + " " + std::to_string(k);
				} else return 2;
			}
			printf("%s\n", out.c_str());
			continue;
		}
		std::vector<uint64_t> a;
		for (uint64_t v; in >> v;) a.push_back(v);
		auto need = [&](size_t n) { return a.size() == n; };
		if (what == "pos") {
			if (!need(1)) return 2;
			printf("%u\n", nxz_cb_ring_pos(a[0]));
		} else if (what == "run" || what == "dump") {
			if (!need(what == "run" ? 2 : 1)) return 2;
			const nxz_cb_pieces_t p = what == "run" ? nxz_cb_run(a[0], (uint32_t)a[1]) : nxz_cb_dump(a[0]);
			printf("%u %u %u %u\n", p.start[0], p.len[0], p.start[1], p.len[1]);
		} else if (what == "skip") {
			if (!need(1)) return 2;
			printf("%" PRIu64 "\n", nxz_cb_run_skip(a[0]));
		} else if (what == "src") {
			if (!need(4)) return 2;
			printf("%" PRIu64 "\n", nxz_cb_match_src(a[0], (uint32_t)a[1], (uint32_t)a[2], (uint32_t)a[3]));
		} else if (what == "mods") {
			int ok = 1;
			for (uint32_t d = 1; d < 259; d++)
				for (uint32_t i = 0; i < 320; i++) ok &= nxz_cb_mod(i, d, nxz_cb_recip(d)) == i % d;
			printf("%d\n", ok);
		} else return 2;
	}
	return 0;
}
