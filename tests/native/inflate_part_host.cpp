// The rules of nxz_batch_inflate_streams_part (power-gzip_amd/csrc/nxz_inflate_part.h) compiled for the host: a stand-alone program for
// tests/test_inflate_part_rules_host.py, built with AddressSanitizer and UBSan.  One command a line on stdin, one answer a line:
//   sizes
//   refuse <src> <dst> <prev> <src_len> <dst_cap> <prev_len> <flags> <phase> <tail_len>
//   hdr <fmt> <hex of the bytes> <piece lengths ...>     the bytes through the state machine in those pieces, a fresh carry
//   trailer <fmt> <crc> <adler> <total_out> <hex> <piece lengths ...>
//   stale <fmt> <tail_len> <n>
//   close <told> <hist> <body> <src_len> <cap> <spbc> <subc> <sfbt> <tebc> <cc> <tpbc>   source byte k of [tail][part from body] is k & 0xff
//   cut <scratch> <max_streams> <bound_0> <bound_1> ...   the engine's own cut of a batch into chunks (nxz_streams_plan.h): "m off_0 .. off_m"
//                                                        per chunk, m read back from off[] as the engine reads it, then "max_cnt max_bytes", all on one line joined by " | "
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "nxz_inflate_part.h"
#include "nxz_streams_plan.h"

static std::vector<uint8_t> unhex(const std::string &h)
{
	std::vector<uint8_t> v;
	if (h == "-") return v;
	for (size_t i = 0; i + 1 < h.size(); i += 2) v.push_back((uint8_t)strtoul(h.substr(i, 2).c_str(), nullptr, 16));
	return v;
}

static void print_frame(const nxz_inflate_carry_t &c)
{
	const nxz_batch_frame_t &f = c.frame;
	printf("%u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u", f.status, f.format, f.hdr_len, f.end, f.check, f.isize, f.mtime, f.dictid, f.extra_off,
	       f.extra_len, f.name_off, f.comment_off, f.flg, f.xfl, f.os, f.cinfo);
}

int main()
{
	std::string line;
	while (std::getline(std::cin, line)) {
		std::istringstream in(line);
		std::string cmd;
		in >> cmd;
		if (cmd == "sizes") {
			printf("%zu %zu %zu %d\n", sizeof(nxz_inflate_part_job_t), sizeof(nxz_inflate_carry_t), sizeof(nxz_inflate_part_result_t), NXZ_INFLATE_PART_TAIL);
		} else if (cmd == "refuse") {
			unsigned long long s, d, p; uint32_t sl, dc, pl, fl, ph, tl;
			in >> s >> d >> p >> sl >> dc >> pl >> fl >> ph >> tl;
			nxz_inflate_part_job_t j;
			j.src = (const uint8_t *)(uintptr_t)s; j.dst = (uint8_t *)(uintptr_t)d; j.prev = (const uint8_t *)(uintptr_t)p;
			j.src_len = sl; j.dst_cap = dc; j.prev_len = pl; j.flags = fl;
			printf("%u\n", nxz_inflate_part_refusal(&j, ph, tl));
		} else if (cmd == "hdr") {
			int fmt; std::string hex;
			in >> fmt >> hex;
			const std::vector<uint8_t> b = unhex(hex);
			nxz_inflate_carry_t *c = new nxz_inflate_carry_t;
			memset(c, 0xa5, sizeof(*c));
			nxz_inflate_part_start(c, fmt);
			size_t at = 0, n, taken = 0;
			while (in >> n) {
				// each piece in a buffer of exactly its size: a read beyond it is the sanitizer's
				uint8_t *piece = (uint8_t *)malloc(n ? n : 1);
				if (n) memcpy(piece, b.data() + at, n);
				if (c->phase == NXZ_INFLATE_PHASE_HEADER) taken += nxz_inflate_part_header_run(c, fmt, piece, (uint32_t)n);
				free(piece);
				at += n;
			}
			printf("%u %zu ", c->phase, taken);
			print_frame(*c);
			printf("\n");
			delete c;
		} else if (cmd == "trailer") {
			int fmt; uint32_t crc, adler; unsigned long long total; std::string hex;
			in >> fmt >> crc >> adler >> total >> hex;
			const std::vector<uint8_t> b = unhex(hex);
			nxz_inflate_carry_t *c = new nxz_inflate_carry_t;
			nxz_inflate_part_start(c, fmt);
			c->frame.format = fmt; c->phase = NXZ_INFLATE_PHASE_TRAILER; c->crc = crc; c->adler = adler; c->total_out = total;
			size_t at = 0, n;
			while (in >> n) {
				uint8_t *piece = (uint8_t *)malloc(n ? n : 1);
				if (n) memcpy(piece, b.data() + at, n);
				const uint32_t k = nxz_inflate_part_trailer_take(c, piece, (uint32_t)n);
				free(piece);
				c->total_in += k;
				at += n;
				printf("%u ", k);
				if (nxz_inflate_part_trailer_finish(c)) break;
			}
			printf("| %u %u %u %u %u %u\n", c->phase, c->frame.status, c->frame.check, c->frame.isize, c->frame.end, c->tail_len);
			delete c;
		} else if (cmd == "stale") {
			// a record that was never started and says TRAILER with `tail_len` bytes: a part of n bytes takes nothing beyond a trailer
			int fmt; uint32_t tail_len, n;
			in >> fmt >> tail_len >> n;
			nxz_inflate_carry_t *c = new nxz_inflate_carry_t;
			memset(c, 0xa5, sizeof(*c));
			c->frame.format = fmt; c->phase = NXZ_INFLATE_PHASE_TRAILER; c->tail_len = tail_len;
			uint8_t *piece = (uint8_t *)calloc(n ? n : 1, 1);
			const uint32_t k = nxz_inflate_part_trailer_take(c, piece, n);
			free(piece);
			printf("%u %u\n", k, c->tail_len);
			delete c;
		} else if (cmd == "close") {
			uint32_t told, hist, body, src_len, cap, spbc, subc, sfbt, tebc, cc, tpbc;
			in >> told >> hist >> body >> src_len >> cap >> spbc >> subc >> sfbt >> tebc >> cc >> tpbc;
			const uint32_t L = told + (src_len - body);
			uint8_t *buf = (uint8_t *)malloc(hist + L + 1);
			for (uint32_t k = 0; k < L; k++) buf[hist + k] = (uint8_t)k;
			nxz_inflate_carry_t *c = new nxz_inflate_carry_t;
			nxz_inflate_part_start(c, NXZ_FMT_ZLIB);
			c->phase = NXZ_INFLATE_PHASE_BODY; c->tail_len = told; c->frame.hdr_len = 2; c->total_in = 1000; c->total_out = 5000;
			nxz_inflate_part_job_t j; memset(&j, 0, sizeof(j));
			j.src_len = src_len; j.dst_cap = cap;
			nxz_batch_job_t d; memset(&d, 0, sizeof(d));
			d.src = buf; d.hist_len = hist; d.src_len = hist + L; d.dst_cap = cap;
			nxz_batch_result_t r; memset(&r, 0, sizeof(r));
			r.cc = cc; r.tpbc = tpbc; r.tebc = tebc; r.spbc = spbc; r.subc = subc; r.sfbt = sfbt; r.crc = 7; r.adler = 9;
			nxz_batch_dht_t t; memset(&t, 0, sizeof(t));
			t.dhtlen = 100;
			nxz_inflate_part_result_t o;
			nxz_inflate_part_close(c, &j, body, &d, &r, &t, &o);
			printf("%u %u %u %u | %u %u %u %u %u %u %llu %llu %u |", o.cc, o.status, o.in_used, o.out_len, c->phase, c->frame.status, c->sfbt, c->rem, c->subc,
			       c->dhtlen, (unsigned long long)c->total_in, (unsigned long long)c->total_out, c->tail_len);
			for (uint32_t k = 0; k < c->tail_len; k++) printf(" %u", c->tail[k]);
			printf("\n");
			delete c; free(buf);
		} else if (cmd == "cut") {
			unsigned long long scratch, v; uint32_t max_streams;
			in >> scratch >> max_streams;
			std::vector<uint64_t> bound;
			while (in >> v) bound.push_back(v);
			// off[] in a buffer of exactly the 2 n entries the engine sets aside: a write beyond it is the sanitizer's
			uint64_t *off = (uint64_t *)malloc(2 * bound.size() * sizeof(uint64_t) + 1);
			const nxz_plan_cut p = nxz_plan_inflate_cut(bound.size(), scratch, max_streams, off, [&](size_t i) { return bound[i]; });
			for (size_t e0 = 0; e0 < p.entries;) {
				const uint32_t m = nxz_plan_cut_streams(off, e0, p.entries);
				printf("%u", m);
				for (uint32_t k = 0; k <= m; k++) printf(" %llu", (unsigned long long)off[e0 + k]);
				printf(" | ");
				e0 += m + 1;
			}
			printf("%u %llu\n", p.max_cnt, (unsigned long long)p.max_bytes);
			free(off);
		} else {
			fprintf(stderr, "unknown command: %s\n", cmd.c_str());
			return 2;
		}
	}
	return 0;
}
