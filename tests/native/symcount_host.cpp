// The arithmetic of nxzsc::count_kernel (power-gzip_amd/csrc/nxz_symcount.h) on the host, under AddressSanitizer and UBSan:
//   symbols          every length - 3 in 0..255 and every distance - 1 in 0..32767 against RFC 1951's base tables
//   blocks <seed>    parses of blocks of n positions, n round the edges of the lane's 8 positions, the round of 2048 and the
//                    block: the header's lane functions "as 256 lanes would" against a straightforward count over (bitmaps,
//                    records, source).  The source holds exactly n bytes and the record array exactly its records (the
//                    sanitizer sees a read behind either); the bitmaps' bits behind position n are all set.
// Prints one line per case; exit status 0 when everything agrees.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "nxz_symcount.h"

static const uint32_t LEN_BASE[29] = { 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258 };
static const uint32_t DIST_BASE[30] = { 1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
					8193, 12289, 16385, 24577 };

static uint32_t by_table(const uint32_t *base, int nbase, uint32_t v)
{
	int s = 0;
	while (s + 1 < nbase && base[s + 1] <= v) s++;
	return (uint32_t)s;
}

static int symbols()
{
	int bad = 0;
	for (uint32_t l3 = 0; l3 < 256; l3++)
		if (nxzsc::length_symbol(l3) != by_table(LEN_BASE, 29, l3 + 3)) { printf("length %u: %u\n", l3 + 3, nxzsc::length_symbol(l3)); bad++; }
	for (uint32_t d = 0; d < 32768; d++)
		if (nxzsc::distance_symbol(d) != by_table(DIST_BASE, 30, d + 1)) { printf("distance %u: %u\n", d + 1, nxzsc::distance_symbol(d)); bad++; }
	for (uint32_t l3 = 0; l3 < 256; l3 += 5)
		for (uint32_t d = 0; d < 32768; d += 77) {
			uint32_t ls, ds;
			nxzsc::record_symbols(l3 | (d << 8), ls, ds);
			if (ls != 257 + by_table(LEN_BASE, 29, l3 + 3) || ds != 286 + by_table(DIST_BASE, 30, d + 1)) bad++;
		}
	printf("symbols: %d wrong\n", bad);
	return bad;
}

static uint32_t rnd(uint64_t &s)
{
	s = s * 6364136223846793005ull + 1442695040888963407ull;
	return (uint32_t)(s >> 33);
}

// kind 0: a random parse; 1: literals only; 2: length 258 at distance 1 all the way (what a block of zeros parses to);
// 3: a random parse of a source of 0xff bytes; 4: every length and every distance symbol in turn
static int block(uint32_t n, int kind, uint64_t seed)
{
	uint8_t *src = (uint8_t *)malloc(n ? n : 1);               // exactly n bytes: a read behind them is the sanitizer's
	for (uint32_t i = 0; i < n; i++) src[i] = kind == 3 ? 0xff : (uint8_t)rnd(seed);
	std::vector<uint32_t> litb(2048, 0), tokb(2048, 0), recs;
	uint32_t turn = 0;
	for (uint32_t p = 0; p < n;) {
		uint32_t len = 1;
		const uint32_t left = n - p;
		if (kind == 2) len = left >= 258 ? 258 : left >= 3 ? left : 1;
		else if (kind == 4 && left >= 3) { len = LEN_BASE[turn % 29] + (turn % 3 == 0 && turn % 29 < 28 && turn % 29 >= 8); if (len > left) len = left; }
		else if (kind != 1 && left >= 3 && rnd(seed) % 3 == 0) { len = 3 + rnd(seed) % 256; if (rnd(seed) % 8 == 0) len = 258; if (len > left) len = left; }
		if (len >= 3) {
			const uint32_t d = kind == 2 ? 0 : kind == 4 ? DIST_BASE[turn % 30] - 1 + (turn % 30 >= 4 ? turn % 2 : 0) : (rnd(seed) % 4 == 0 ? rnd(seed) % 8 : rnd(seed) % 32768);
			tokb[p >> 5] |= 1u << (p & 31);
			recs.push_back((len - 3) | (d << 8));
			turn++;
		} else litb[p >> 5] |= 1u << (p & 31);
		p += len;
	}
	// the straightforward count, before what lies behind the block is spoiled
	std::vector<uint32_t> want(nxzsc::NSYM, 0), got(nxzsc::NSYM, 0);
	for (uint32_t p = 0; p < n; p++) if (litb[p >> 5] >> (p & 31) & 1) want[src[p]]++;
	for (uint32_t r : recs) { want[257 + by_table(LEN_BASE, 29, (r & 0xff) + 3)]++; want[286 + by_table(DIST_BASE, 30, (r >> 8) + 1)]++; }
	want[256] = 1;
	for (uint32_t p = n; p < 65536; p++) { litb[p >> 5] |= 1u << (p & 31); tokb[p >> 5] |= 1u << (p & 31); }
	uint32_t *rec = (uint32_t *)malloc(recs.size() ? recs.size() * 4 : 4);
	if (!recs.empty()) memcpy(rec, recs.data(), recs.size() * 4);

	// as the kernel: the record count from the match bitmap, 8 words a lane; the records as they lie; the rounds of 2048
	const uint32_t nwords = (n + 31) >> 5;
	uint32_t nrec = 0;
	for (uint32_t t = 0; t < nxzsc::LANES; t++)
		if (8 * t < nwords)
			for (uint32_t k = 0; k < 8; k++) nrec += (uint32_t)__builtin_popcount(tokb[8 * t + k] & nxzsc::word_mask(8 * t + k, n));
	int bad = nrec != recs.size();
	for (uint32_t i = 0; i < nrec && i < recs.size(); i++) {
		uint32_t ls, ds;
		nxzsc::record_symbols(rec[i], ls, ds);
		got[ls]++; got[ds]++;
	}
	for (uint32_t r0 = 0; r0 < n; r0 += nxzsc::RPOS)
		for (uint32_t t = 0; t < nxzsc::LANES; t++) {
			const uint32_t p0 = r0 + 8 * t;
			if (p0 >= n) continue;
			nxzsc::lane_literals(nxzsc::lane_bytes(src, p0, n), litb[p0 >> 5], p0, n, [&](uint32_t sym) { got[sym]++; });
		}
	got[256] = 1;
	for (uint32_t i = 0; i < nxzsc::NSYM; i++) bad += got[i] != want[i];
	printf("block n %u kind %d: %zu records, %d wrong\n", n, kind, recs.size(), bad);
	free(src); free(rec);
	return bad;
}

int main(int argc, char **argv)
{
	if (argc >= 2 && !strcmp(argv[1], "symbols")) return symbols() != 0;
	if (argc >= 3 && !strcmp(argv[1], "blocks")) {
		static const uint32_t N[] = { 0, 1, 7, 8, 9, 2047, 2048, 2049, 65535, 65536 };
		uint64_t seed = strtoull(argv[2], nullptr, 0);
		int bad = 0;
		for (uint32_t n : N)
			for (int kind = 0; kind < 5; kind++) bad += block(n, kind, seed = seed * 2862933555777941757ull + 3037000493ull);
		return bad != 0;
	}
	fprintf(stderr, "usage: symcount_host symbols | blocks <seed>\n");
	return 2;
}
