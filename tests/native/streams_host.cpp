// streams_host.cpp -- TEST ONLY.  The rules of nxz_batch_deflate_streams (power-gzip_amd/csrc/nxz_streams.h), the code the device
// runs, compiled for the host.  One request per line on stdin (all numbers decimal), answers on stdout:
//   plan src_len hist_max                      -> "blocks B H bound_raw bound_zlib bound_gzip"
//   blks src_len hist_max                      -> "blocks", then one line "start len window" per block
//   crc crc_a crc_b len_b                      -> the CRC-32 of [a][b] (square-and-multiply operator)
//   crcb crc_a crc_b B full tail               -> the same with b = `full` blocks of B bytes and `tail` bytes (precomputed block operator)
//   adler a b len_b                            -> the Adler-32 of [a][b]
//   reset                                      -> "ok": the running values below start over (0, 0, 1)
//   rcrc crc_b len_b / rcrcb crc_b B full tail / radler b len_b
//                                              -> the same joins with the running value as a; it becomes, and is, the answer
//   hdr fmt level                              -> the header bytes in hex ("-" for none)
//   trl fmt crc adler src_len                  -> the trailer bytes in hex ("-" for none)
//   empty fmt level                            -> the whole stream of a buffer of length 0 in hex
//   refuse src dst src_len dst_cap hist_max fmt -> the completion code
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include "nxz_streams.h"

static void hex(const uint8_t *p, uint32_t n, bool nl)
{
	if (!n && nl) printf("-");
	for (uint32_t i = 0; i < n; i++) printf("%02x", p[i]);
	if (nl) printf("\n");
}

int main()
{
	char line[256];
	uint32_t run_crc = 0, run_crcb = 0, run_adler = 1;
	while (fgets(line, sizeof line, stdin)) {
		uint64_t a[6] = {0};
		char what[16] = "";
		const int k = sscanf(line, "%15s %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, what, &a[0], &a[1], &a[2], &a[3], &a[4], &a[5]);
		if (k < 1) continue;
		if (!strcmp(what, "plan") && k == 3) {
			const uint32_t hm = (uint32_t)a[1], B = nxz_streams_block_bytes(hm);
			printf("%" PRIu64 " %u %u %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", nxz_streams_blocks(a[0], B), B, nxz_streams_window(hm),
			       nxz_streams_bound(a[0], hm, NXZ_FMT_RAW), nxz_streams_bound(a[0], hm, NXZ_FMT_ZLIB), nxz_streams_bound(a[0], hm, NXZ_FMT_GZIP));
		} else if (!strcmp(what, "blks") && k == 3) {
			const uint32_t hm = (uint32_t)a[1], B = nxz_streams_block_bytes(hm), H = nxz_streams_window(hm);
			const uint64_t nb = nxz_streams_blocks(a[0], B);
			printf("%" PRIu64 "\n", nb);
			for (uint64_t b = 0; b < nb; b++)
				printf("%" PRIu64 " %u %u\n", nxz_streams_block_start(b, B), nxz_streams_block_len(a[0], b, B), nxz_streams_block_window(b, B, H));
		} else if (!strcmp(what, "crc") && k == 4) printf("%u\n", nxz_crc_join((uint32_t)a[0], (uint32_t)a[1], nxz_crc_shift_op(a[2])));
		else if (!strcmp(what, "crcb") && k == 6)
			printf("%u\n", nxz_crc_join((uint32_t)a[0], (uint32_t)a[1], nxz_crc_blocks_op(nxz_crc_shift_op(a[2]), a[3], (uint32_t)a[4])));
		else if (!strcmp(what, "reset")) { run_crc = run_crcb = 0; run_adler = 1; printf("ok\n"); }
		else if (!strcmp(what, "rcrc") && k == 3) printf("%u\n", run_crc = nxz_crc_join(run_crc, (uint32_t)a[0], nxz_crc_shift_op(a[1])));
		else if (!strcmp(what, "rcrcb") && k == 5)
			printf("%u\n", run_crcb = nxz_crc_join(run_crcb, (uint32_t)a[0], nxz_crc_blocks_op(nxz_crc_shift_op(a[1]), a[2], (uint32_t)a[3])));
		else if (!strcmp(what, "radler") && k == 3) printf("%u\n", run_adler = nxz_adler_join(run_adler, (uint32_t)a[0], a[1]));
		else if (!strcmp(what, "adler") && k == 4) printf("%u\n", nxz_adler_join((uint32_t)a[0], (uint32_t)a[1], a[2]));
		else if (!strcmp(what, "hdr") && k == 3) {
			uint8_t h[10];
			hex(h, nxz_streams_header((int)a[0], (int)(int64_t)a[1], h), true);
		} else if (!strcmp(what, "trl") && k == 5) {
			uint8_t t[8];
			hex(t, nxz_streams_trailer((int)a[0], (uint32_t)a[1], (uint32_t)a[2], a[3], t), true);
		} else if (!strcmp(what, "empty") && k == 3) {
			uint8_t h[10], e[NXZ_STREAMS_EMPTY_LEN], t[8];
			hex(h, nxz_streams_header((int)a[0], (int)(int64_t)a[1], h), false);
			nxz_streams_empty(e);
			hex(e, NXZ_STREAMS_EMPTY_LEN, false);
			hex(t, nxz_streams_trailer((int)a[0], 0, 1, 0, t), false);
			printf("\n");
		} else if (!strcmp(what, "refuse") && k == 7) {
			nxz_stream_job_t j;
			j.src = (const uint8_t *)(uintptr_t)a[0]; j.dst = (uint8_t *)(uintptr_t)a[1]; j.src_len = a[2]; j.dst_cap = a[3];
			printf("%u\n", nxz_streams_refusal(&j, (uint32_t)a[4], (int)a[5]));
		} else return 2;
	}
	return 0;
}
