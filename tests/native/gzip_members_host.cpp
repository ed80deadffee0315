// gzip_members_host.cpp -- TEST ONLY.  The rules of the multi-member gzip calls (power-gzip_amd/csrc/nxz_gzip_members.h), the code
// the device runs, compiled for the host.  The bit-walking is not here: a request hands the walk what the kernel's parser and size
// walk would have found for each member, and gets back what the rules make of it.  One request per line on stdin (numbers decimal):
//   job resume hist_len                             -> "0" / "1"
//   walk member_cap src_len hex N  then N lines     -> N' record lines "uoff coff clen hdr_len isize check status", then
//        "hst hdr_len wcc eob end_byte counted"        "S status members failed consumed out_len cc"
//        hex: the job's bytes ("-": none) -- the trailers and the two bytes behind a member are read from them; a member line is
//        what was found at the member's start: the header's status and length, the walk's cc / final_eob, the deflate bytes it
//        used and the bytes it counted.  The walk stops where the rules stop it; lines it does not get to are ignored.
//   inside status coff clen uoff isize src_len dst_cap -> "0" / "1"
//   plan status out_len failed member_cap dst_cap stale base total -> "status count"
//   join status failed first_bad bad_cc decoded      -> "status failed out_len cc"
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "nxz_frame.h"
#include "nxz_gzip_members.h"

static std::vector<uint8_t> unhex(const char *h)
{
	std::vector<uint8_t> v;
	if (!strcmp(h, "-")) return v;
	for (size_t i = 0; h[i] && h[i + 1]; i += 2) {
		unsigned x;
		sscanf(h + i, "%2x", &x);
		v.push_back((uint8_t)x);
	}
	return v;
}

int main()
{
	static char line[1 << 22];
	while (fgets(line, sizeof line, stdin)) {
		char what[16] = "";
		if (sscanf(line, "%15s", what) < 1) continue;
		uint64_t a[8] = {0};
		if (!strcmp(what, "job")) {
			if (sscanf(line, "%*s %" SCNu64 " %" SCNu64, &a[0], &a[1]) != 2) return 2;
			printf("%d\n", nxz_gzm_job_ok((uint32_t)a[0], (uint32_t)a[1]) ? 1 : 0);
		} else if (!strcmp(what, "walk")) {
			uint32_t cap, src_len, n;
			static char hex[1 << 22];
			if (sscanf(line, "%*s %u %u %s %u", &cap, &src_len, hex, &n) != 4) return 2;
			const std::vector<uint8_t> src = unhex(hex);
			if (src.size() != src_len) return 3;
			nxz_gzm_acc_t acc = nxz_gzm_begin();
			uint32_t pos = 0;
			bool go = true;
			for (uint32_t k = 0; k < n; k++) {
				uint32_t hst, hl, wcc, eob, end_byte, counted;
				if (!fgets(line, sizeof line, stdin) || sscanf(line, "%u %u %u %u %u %u", &hst, &hl, &wcc, &eob, &end_byte, &counted) != 6) return 2;
				if (!go) continue;
				const uint32_t left = src_len - pos;
				nxz_gzip_member_t m = nxz_gzm_member(acc.out_len, pos);
				uint32_t st = hst, cc = 0;
				if (st == NXZ_FRAME_OK) {
					m.hdr_len = hl;
					if (!nxz_gzm_room(left, hl)) st = NXZ_FRAME_TRUNCATED;
				}
				if (st == NXZ_FRAME_OK) {
					st = nxz_gzm_walk_status(wcc, eob);
					cc = nxz_gzm_walk_cc(wcc, eob);
					if (st == NXZ_FRAME_OK) {
						const uint32_t dend = hl + end_byte;
						if ((uint64_t)pos + dend + 8 > src_len) return 4;       // (the walk's source ends 8 bytes before the job's)
						const uint8_t *t = src.data() + pos + dend;
						st = nxz_gzm_trailer(&m, dend, nxz_rd32le(t), nxz_rd32le(t + 4), counted);
					}
				}
				m.status = st;
				if (nxz_gzm_stored(&acc, cap))
					printf("%" PRIu64 " %u %u %u %u %u %u\n", (uint64_t)m.uoff, m.coff, m.clen, m.hdr_len, m.isize, m.check, m.status);
				if (!nxz_gzm_add(&acc, &m, cc)) { go = false; continue; }
				pos = acc.consumed;
				if (!nxz_gzm_more(src.data(), src_len, pos)) go = false;
			}
			const nxz_gzip_stream_t s = nxz_gzm_summary(&acc, cap);
			printf("S %u %u %u %u %" PRIu64 " %u\n", s.status, s.members, s.failed, s.consumed, (uint64_t)s.out_len, s.cc);
		} else if (!strcmp(what, "refused")) {
			const nxz_gzip_stream_t s = nxz_gzm_refused();
			printf("S %u %u %u %u %" PRIu64 " %u\n", s.status, s.members, s.failed, s.consumed, (uint64_t)s.out_len, s.cc);
		} else if (!strcmp(what, "inside")) {
			if (sscanf(line, "%*s %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &a[0], &a[1], &a[2], &a[3], &a[4], &a[5], &a[6]) != 7) return 2;
			nxz_gzip_member_t m = {};
			m.status = (uint32_t)a[0]; m.coff = (uint32_t)a[1]; m.clen = (uint32_t)a[2]; m.uoff = a[3]; m.isize = (uint32_t)a[4];
			printf("%d\n", nxz_gzm_record_inside(&m, (uint32_t)a[5], (uint32_t)a[6]) ? 1 : 0);
		} else if (!strcmp(what, "plan")) {
			if (sscanf(line, "%*s %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &a[0], &a[1], &a[2], &a[3], &a[4], &a[5], &a[6], &a[7]) != 8) return 2;
			uint32_t count = 0;
			const uint32_t st = nxz_gzm_plan((uint32_t)a[0], a[1], (uint32_t)a[2], (uint32_t)a[3], (uint32_t)a[4], a[5] != 0, a[6], a[7], &count);
			printf("%u %u\n", st, count);
		} else if (!strcmp(what, "join")) {
			if (sscanf(line, "%*s %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &a[0], &a[1], &a[2], &a[3], &a[4]) != 5) return 2;
			nxz_gzip_stream_t s = {};
			s.status = (uint32_t)a[0]; s.failed = (uint32_t)a[1];
			nxz_gzm_join(&s, (uint32_t)a[2], (uint32_t)a[3], a[4]);
			printf("%u %u %" PRIu64 " %u\n", s.status, s.failed, (uint64_t)s.out_len, s.cc);
		} else return 2;
	}
	return 0;
}
