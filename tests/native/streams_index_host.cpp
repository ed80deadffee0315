// streams_index_host.cpp -- TEST ONLY.  The rules of nxz_batch_deflate_streams_indexed (power-gzip_amd/csrc/nxz_streams_index.h), the code
// the device runs, compiled for the host.  Requests on stdin (all numbers decimal), answers on stdout:
//   run hdr_len span cp_cap npieces            followed by npieces lines "stored len keep tebc final": the pieces of one stream in
//                                              order, the first laid behind hdr_len bytes of framing
//     -> "H bit u" for every block header in stream order, "C slot bit u" for every checkpoint (slot = cp_cap: counted, not stored),
//        "S bit u" for the sentinel, "N count status", "E stream_bytes" (header + pieces), then "."
//   size stored len keep tebc final            -> the bytes the piece occupies
//   shape n cp_cap                             -> 1 when the call takes such arrays, else 0
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include "nxz_streams_index.h"

static bool read_piece(nxz_si_piece_t *p)
{
	char line[256];
	if (!fgets(line, sizeof line, stdin)) return false;
	return sscanf(line, "%u %u %u %u %u", &p->stored, &p->len, &p->keep, &p->tebc, &p->final) == 5;
}

int main()
{
	char line[256];
	while (fgets(line, sizeof line, stdin)) {
		uint64_t a[5] = {0};
		char what[16] = "";
		const int k = sscanf(line, "%15s %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, what, &a[0], &a[1], &a[2], &a[3], &a[4]);
		if (k < 1) continue;
		if (!strcmp(what, "run") && k == 5) {
			const uint32_t hdr_len = (uint32_t)a[0], cp_cap = (uint32_t)a[2];
			const uint64_t span = a[1], np = a[3];
			// checkpoint 0 is the first header, wherever the pieces go: the prologue writes it
			nxz_cp_acc_t acc = nxz_cp_begin();
			printf("C %u %" PRIu64 " 0\n", nxz_cp_add(&acc, 0, cp_cap), nxz_si_first_bit(hdr_len));
			uint64_t P = hdr_len, u0 = 0, end = nxz_si_empty_end_bit(hdr_len);
			if (!np) printf("H %" PRIu64 " 0\n", nxz_si_first_bit(hdr_len));
			for (uint64_t i = 0; i < np; i++) {
				nxz_si_piece_t p;
				if (!read_piece(&p)) return 3;
				uint64_t bit[2], u[2];
				const uint32_t nh = nxz_si_headers(&p, P, u0, bit, u);
				for (uint32_t h = 0; h < nh; h++) {
					printf("H %" PRIu64 " %" PRIu64 "\n", bit[h], u[h]);
					if (nxz_si_takes(u[h], acc.last_uoff, span)) printf("C %u %" PRIu64 " %" PRIu64 "\n", nxz_cp_add(&acc, u[h], cp_cap), bit[h], u[h]);
				}
				if (i + 1 == np) end = nxz_si_end_bit(&p, P);
				P += nxz_si_piece_size(&p);
				u0 += p.len;
			}
			if (!np) P += NXZ_STREAMS_EMPTY_LEN;
			const nxz_checkpoint_stream_t s = nxz_si_summary(acc.count, cp_cap, NXZ_FMT_RAW, u0);
			if (nxz_cp_has_sentinel(s.status)) printf("S %" PRIu64 " %" PRIu64 "\n", end, u0);
			printf("N %u %u\nE %" PRIu64 "\n.\n", s.count, s.status, P);
		} else if (!strcmp(what, "size") && k == 6) {
			nxz_si_piece_t p = {(uint32_t)a[0], (uint32_t)a[1], (uint32_t)a[2], (uint32_t)a[3], (uint32_t)a[4]};
			printf("%u\n", nxz_si_piece_size(&p));
		} else if (!strcmp(what, "shape") && k == 3) printf("%d\n", nxz_si_shape_ok(a[0], (uint32_t)a[1]) ? 1 : 0);
		else return 2;
	}
	return 0;
}
