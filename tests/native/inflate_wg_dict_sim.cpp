// inflate_wg_dict_sim.cpp -- TEST INFRASTRUCTURE: the dictionary form of the workgroup-per-stream inflate kernel
// (nxzw::inflate_wg_dict_kernel, power-gzip_amd/csrc/nxz_inflate_wg.hip, the product source itself) run on the CPU through
// tests/native/hip_cpu_shim.h, against raw deflate streams that system zlib made with deflateSetDictionary.  One launch per
// dictionary (1, 17, 4 099, 32 768 and 50 000 bytes, and none).  Checks: every stream the kernel takes comes out byte for byte
// with the result record of a finished stream and nothing of the dictionary in the target; every stream it must not decode
// (a distance in front of the window, cut short, target too small) is on the hand-back list, and only those.
//   usage: inflate_wg_dict_sim <file with sample text> [seed] [pmin_bits] [bytes of the long case]
#include "hip_cpu_shim.h"
#include "../../power-gzip_amd/csrc/nxz_inflate_wg.hip"
#include "../../power-gzip_amd/csrc/nxz_dict.h"
#include <zlib.h>
#include <stdio.h>
#include <string>
#include <vector>

typedef std::vector<uint8_t> Bytes;
static uint64_t rng_state = 88172645463325252ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 11); }

static Bytes deflate_raw_dict(const Bytes &in, const Bytes &dict, int level)
{
	z_stream z;
	memset(&z, 0, sizeof(z));
	if (deflateInit2(&z, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) abort();
	if (!dict.empty() && deflateSetDictionary(&z, dict.data(), (uInt)dict.size()) != Z_OK) abort();
	Bytes out(deflateBound(&z, in.size()) + 64);
	z.next_in = (Bytef *)in.data(); z.avail_in = (uInt)in.size();
	z.next_out = out.data(); z.avail_out = (uInt)out.size();
	if (deflate(&z, Z_FINISH) != Z_STREAM_END) abort();
	out.resize(z.total_out);
	deflateEnd(&z);
	return out;
}
// what zlib itself makes of the stream with that dictionary (the independent implementation)
static bool zlib_inflates(const Bytes &stream, const Bytes &dict, const Bytes &plain)
{
	z_stream z;
	memset(&z, 0, sizeof(z));
	if (inflateInit2(&z, -15) != Z_OK) abort();
	if (!dict.empty() && inflateSetDictionary(&z, dict.data(), (uInt)dict.size()) != Z_OK) abort();
	Bytes out(plain.size() + 16);
	z.next_in = (Bytef *)stream.data(); z.avail_in = (uInt)stream.size();
	z.next_out = out.data(); z.avail_out = (uInt)out.size();
	const int rc = inflate(&z, Z_FINISH);
	const bool ok = rc == Z_STREAM_END && z.total_out == plain.size() && memcmp(out.data(), plain.data(), plain.size()) == 0;
	inflateEnd(&z);
	return ok;
}

struct Case { std::string name; Bytes plain, stream; bool expect_taken; uint32_t src_off, cap, flags; };

int main(int argc, char **argv)
{
	if (argc < 2) { fprintf(stderr, "usage: %s <text file> [seed] [pmin_bits] [long bytes]\n", argv[0]); return 2; }
	Bytes text;
	{
		FILE *f = fopen(argv[1], "rb");
		if (!f) { perror(argv[1]); return 2; }
		uint8_t buf[65536]; size_t k;
		while ((k = fread(buf, 1, sizeof(buf), f)) > 0) text.insert(text.end(), buf, buf + k);
		fclose(f);
	}
	if (argc > 2) rng_state ^= (uint64_t)strtoull(argv[2], nullptr, 0) * 0x9E3779B97F4A7C15ull;
	const uint32_t pmin = argc > 3 ? (uint32_t)atoi(argv[3]) : 128;
	const size_t longn = argc > 4 ? (size_t)atoi(argv[4]) : 300 * 1024;
	auto slice = [&](size_t at, size_t n) { return Bytes(text.begin() + at % (text.size() - n), text.begin() + at % (text.size() - n) + n); };
	int bad = 0;
	uint32_t total = 0, total_back = 0;

	const size_t dict_lens[] = { 0, 1, 17, 4099, 32768, 50000 };
	for (size_t dl : dict_lens) {
		// the dictionary: text the records share vocabulary with; its window by the rule of nxz_dict.h
		const Bytes dict(text.begin(), text.begin() + dl);
		const uint32_t win = nxz_dict_inflate_window(dl);
		std::vector<uint8_t> dwin_buf(32768 + 16, 0x5e);                       // (what stands in front of the window must not matter)
		uint8_t *dwin = (uint8_t *)(((uintptr_t)dwin_buf.data() + 15) & ~(uintptr_t)15);
		if (win) memcpy(dwin + 32768 - win, dict.data() + nxz_dict_inflate_start(dl), win);

		std::vector<Case> cases;
		auto add = [&](const char *name, Bytes plain, int level, bool taken = true, uint32_t off = 0, uint32_t cap = 0, uint32_t flags = 0, const Bytes *made_with = nullptr) {
			Case c; c.name = name; c.plain = plain; c.stream = deflate_raw_dict(plain, made_with ? *made_with : dict, level);
			c.expect_taken = taken; c.src_off = off; c.cap = cap; c.flags = flags;
			if (taken && !zlib_inflates(c.stream, (flags & NXZ_JOB_NO_DICT) ? Bytes() : dict, plain)) { printf("FAIL %s: zlib does not take its own stream\n", name); bad++; }
			cases.push_back(c);
		};
		const Bytes none;
		add("one byte", Bytes(1, text[40]), 6);
		add("text 300 -1", slice(rnd(), 300), 1, true, 3);
		add("text 512 -6", Bytes(text.begin() + 40000, text.begin() + 40512), 6);
		add("text 2000 -9", slice(rnd(), 2000), 9, true, 11);
		add("text 20000 -6", slice(rnd(), 20000), 6);
		add("text 40000 -1", slice(rnd(), 40000), 1, true, 5);                  // (with a full window: more than the half of LDS behind it, a flush)
		add("text 65536 -9", slice(rnd(), 65536), 9);
		if (dl) add("the dictionary itself -9", dict, 9);                       // (long matches that span the whole window)
		if (dl) add("the dictionary twice -6", [&] { Bytes v = dict; v.insert(v.end(), dict.begin(), dict.end()); return v; }(), 6, true, 7);
		{
			Bytes v(3000);
			for (auto &b : v) b = (uint8_t)rnd();
			add("random 3000 (no references)", v, 6);
		}
		add("zeros 50000", Bytes(50000, 0), 6);
		add("no dictionary for this job", slice(rnd(), 5000), 6, true, 0, 0, NXZ_JOB_NO_DICT, &none);
		if (dl == 32768) {
			Bytes big;
			while (big.size() < longn) { const Bytes s = slice(rnd(), 50000); big.insert(big.end(), s.begin(), s.end()); }
			add("text long -6", big, 6, true, 9);
		}
		// what the kernel must hand back
		if (dl >= 4099) {
			// a stream that refers to the dictionary, decoded by a job that sees none: a distance in front of the output
			Case c; c.name = "references without the dictionary"; c.plain = Bytes(dict.end() - 3000, dict.end()); c.stream = deflate_raw_dict(c.plain, dict, 6);
			c.expect_taken = false; c.src_off = 0; c.cap = 0; c.flags = NXZ_JOB_NO_DICT;
			cases.push_back(c);
		}
		if (dl == 4099) {
			// ... and one made with more dictionary than this launch holds: 28 669 other bytes in front of the launch's 4 099, and a
			// record that repeats bytes from far in front of them -- distances that reach in front of the window
			Bytes d2(text.begin() + 70000, text.begin() + 70000 + 32768 - 4099);
			const Bytes rec(d2.begin() + 100, d2.begin() + 6100);
			d2.insert(d2.end(), dict.begin(), dict.end());
			Case c; c.name = "made with a 32 KiB dictionary"; c.plain = rec; c.stream = deflate_raw_dict(rec, d2, 9);
			c.expect_taken = false; c.src_off = 0; c.cap = 0; c.flags = 0;
			cases.push_back(c);
		}
		add("target too small", slice(rnd(), 30000), 6, false, 0, 29999);
		{
			Case c = cases[4]; c.name = "cut short"; c.stream.resize(c.stream.size() / 2); c.expect_taken = false; cases.push_back(c);
		}

		const size_t n = cases.size();
		std::vector<nxz_batch_job_t> jobs(n);
		std::vector<nxz_batch_result_t> res(n);
		std::vector<Bytes> srcbuf(n), dstbuf(n);
		for (size_t i = 0; i < n; i++) {
			Case &c = cases[i];
			srcbuf[i].assign(c.stream.size() + 64 + 16, 0xa5);
			uint8_t *base = (uint8_t *)(((uintptr_t)srcbuf[i].data() + 15) & ~(uintptr_t)15) + c.src_off;
			memcpy(base, c.stream.data(), c.stream.size());
			dstbuf[i].assign(c.plain.size() + 5000 + 32, 0xcd);
			uint8_t *dst = (uint8_t *)(((uintptr_t)dstbuf[i].data() + 15) & ~(uintptr_t)15);
			memset(&jobs[i], 0, sizeof(jobs[i]));
			jobs[i].src = base; jobs[i].dst = dst; jobs[i].src_len = (uint32_t)c.stream.size();
			jobs[i].dst_cap = c.cap ? c.cap : (uint32_t)(c.plain.size() + 4096);
			jobs[i].in_adler = 1; jobs[i].reserved = c.flags;
			memset(&res[i], 0xff, sizeof(res[i]));
		}
		std::vector<uint32_t> bail(64 + n, 0), dbg(16, 0);
		uint32_t ctr = 0;
		hipsim_run_block(0, 1, nxzw::NT, [&] { nxzw::inflate_wg_dict_kernel<false>(jobs.data(), (uint32_t)n, res.data(), nullptr, &ctr, bail.data(), pmin | 1024u << 16, 16, dbg.data(), nullptr, dwin, win, 0); });

		std::vector<bool> handed(n, false);
		for (uint32_t k = 0; k < bail[0]; k++) handed[bail[64 + k]] = true;
		for (size_t i = 0; i < n; i++) {
			const Case &c = cases[i];
			if (handed[i] != !c.expect_taken) { printf("FAIL dict %zu, %s: %s\n", dl, c.name.c_str(), handed[i] ? "handed back" : "taken, should have been handed back"); bad++; continue; }
			if (handed[i]) continue;
			const uint8_t *dst = jobs[i].dst;
			if (res[i].tpbc != c.plain.size() || memcmp(dst, c.plain.data(), c.plain.size()) != 0) {
				size_t at = 0;
				while (at < c.plain.size() && at < res[i].tpbc && dst[at] == c.plain[at]) at++;
				printf("FAIL dict %zu, %s: output differs (tpbc %u, expected %zu, first difference at %zu)\n", dl, c.name.c_str(), res[i].tpbc, c.plain.size(), at);
				bad++; continue;
			}
			if (dst[c.plain.size()] != 0xcd && (c.plain.size() & 15) == 0) { printf("FAIL dict %zu, %s: wrote behind the output\n", dl, c.name.c_str()); bad++; }
			if (res[i].cc != 0 || res[i].sfbt != 0x100 || res[i].spbc != jobs[i].src_len || res[i].tebc != 0 || res[i].subc >= 8) {
				printf("FAIL dict %zu, %s: result cc %u sfbt %#x spbc %u subc %u\n", dl, c.name.c_str(), res[i].cc, res[i].sfbt, res[i].spbc, res[i].subc);
				bad++;
			}
		}
		printf("dictionary of %zu bytes: %zu streams, %u handed back, reasons:", dl, n, bail[0]);
		for (int r = 1; r < 12; r++) printf(" %u", dbg[r]);
		printf("\n");
		total += (uint32_t)n; total_back += bail[0];
	}
	printf("%u streams, %u handed back\n%s\n", total, total_back, bad ? "FAILED" : "ok");
	return bad ? 1 : 0;
}
