// verify_host.cpp -- TEST ONLY.  The rules of the batched verify (power-gzip_amd/csrc/nxz_verify.h) and the slice arithmetic they use
// (nxz_cksum_slices.h), the code the device runs, compiled for the host and run "as 64 lanes would".  One request per line on stdin
// (numbers decimal):
//   consts                     -> "PASS LANES RING"
//   budget cut cap             -> nxzv::budget
//   slices done u              -> nxzv::pass_slices
//   drive n seed in_crc in_adler win cap tok...
//                              -> a ring of 32768 bytes driven as nxzv::verify_kernel drives it.  The output is n bytes of a
//                                 generator (byte k = lcg(seed, k)); the ring is preloaded with win bytes of another generator at
//                                 its end; every tok is  t<len>  (a token of len bytes, 1..258: all of it or none before a cut)  or
//                                 s<len>  (a stored run: split at the budget) and writes the next len bytes of the output into the
//                                 ring by nxz_checkpoint_build.h's positions.  The walk's cut rule is nxz_inflate_walk.h's: a token
//                                 that does not fit the budget is cut in front of when the budget is below cap, and the stream
//                                 ends there when it is cap.  Prints "u done crc adler" for every pass (at the cut at u: the bytes
//                                 checksummed and the running checksums behind it) and one more for the end (behind the tail).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <string>
#include <vector>
#include "nxz_verify.h"

static uint8_t gen(uint32_t seed, uint32_t k)
{
	uint32_t x = seed * 2654435761u + k * 40503u;
	x ^= x >> 15; x *= 2246822519u; x ^= x >> 13;
	return (uint8_t)(x >> 8);
}

struct Driver {
	uint32_t *ring;                     // 32768 bytes, 64-byte aligned, exact size: a dword behind the ring is seen
	uint32_t T[1024];
	nxzv::State st;
	std::string out;

	void put(uint32_t u, uint8_t b) { ((uint8_t *)ring)[nxz_cb_ring_pos(u)] = b; }
	void pass(uint32_t u)
	{
		const uint32_t ns = nxzv::pass_slices(st.done, u);
		if (st.done > u || u - st.done > NXZ_CB_RING) { fprintf(stderr, "a pass at %u with done %u\n", u, st.done); exit(3); }
		uint32_t c = 0, s1 = 0, s2 = 0;
		for (uint32_t lane = 0; lane < nxzv::LANES; lane++) {
			const nxzv::Part p = nxzv::lane_pass(ring, st.done, ns, st.crc, lane, T);
			c ^= p.crc; s1 += p.s1; s2 += p.s2;
		}
		nxzv::join(st, ns, c, s1, s2);
	}
	void report(uint32_t u)
	{
		char b[96];
		snprintf(b, sizeof b, "%s%u %u %u %u", out.empty() ? "" : " ", u, st.done, nxzv::crc_of(st), nxzv::adler_of(st));
		out += b;
	}
};

int main()
{
	static char line[1 << 22];
	while (fgets(line, sizeof line, stdin)) {
		std::istringstream in(line);
		std::string what;
		if (!(in >> what)) continue;
		if (what == "consts") { printf("%u %u %u\n", nxzv::PASS, nxzv::LANES, NXZ_CB_RING); continue; }
		if (what == "budget") {
			uint64_t a, b;
			if (!(in >> a >> b)) return 2;
			printf("%u\n", nxzv::budget((uint32_t)a, (uint32_t)b));
			continue;
		}
		if (what == "slices") {
			uint64_t a, b;
			if (!(in >> a >> b)) return 2;
			printf("%u\n", nxzv::pass_slices((uint32_t)a, (uint32_t)b));
			continue;
		}
		if (what != "drive") return 2;
		uint64_t n, seed, in_crc, in_adler, win, cap;
		if (!(in >> n >> seed >> in_crc >> in_adler >> win >> cap) || win > NXZ_CB_RING) return 2;
		Driver d;
		d.ring = (uint32_t *)aligned_alloc(64, NXZ_CB_RING);
		for (uint32_t i = 0; i < NXZ_CB_RING; i++) ((uint8_t *)d.ring)[i] = 0xee;
		for (uint32_t k = 1; k <= win; k++) ((uint8_t *)d.ring)[NXZ_CB_RING - k] = gen((uint32_t)seed ^ 0x5bd1e995u, k);    // window byte -k
		for (uint32_t i = 0; i < 256; i++) nxzck::table_column(d.T, i);
		d.st = nxzv::begin((uint32_t)in_crc, (uint32_t)in_adler);
		uint32_t u = 0, soft = nxzv::budget(d.st.cut, (uint32_t)cap);
		auto cut = [&]() { d.pass(u); d.st.cut = u; d.report(u); soft = nxzv::budget(d.st.cut, (uint32_t)cap); };
		std::string tok;
		bool full = false;
		while (!full && in >> tok) {
			uint32_t len = (uint32_t)strtoul(tok.c_str() + 1, nullptr, 10);
			if (tok[0] == 't') {
				if ((uint64_t)u + len > soft && soft < cap) cut();
				if ((uint64_t)u + len > soft) { full = true; break; }
				for (uint32_t i = 0; i < len; i++) d.put(u + i, gen((uint32_t)seed, u + i));
				u += len;
			} else if (tok[0] == 's') {
				while (len) {
					if ((uint64_t)u + len > soft && soft >= cap) { full = true; break; }
					const uint32_t take = (uint64_t)u + len > soft ? soft - u : len;
					for (uint32_t i = 0; i < take; i++) d.put(u + i, gen((uint32_t)seed, u + i));
					u += take; len -= take;
					if (len) cut();
				}
			} else return 2;
		}
		if (!full && u != n) return 4;
		d.pass(u);
		nxzv::tail(d.st, d.ring, u - d.st.done, d.T);
		d.report(u);
		printf("%s\n", d.out.c_str());
		free(d.ring);
	}
	return 0;
}
