// csrc/bam_in_core.h as plain C++ under AddressSanitizer and UBSan (tests/test_bam_input.py builds and runs this): every record is a heap block of exactly its
// size -- 4 + block_size, what the host's chain walk hands to a lane --, and the comment is written into a heap block of exactly the size the sizes pass gave, so
// a read or write one byte outside a record or a span is reported.
//   in : u32 n, then n x (u32 size, bytes)
//   out: n x (i32 status of bi_check, then for status 0: u32 role; for a kept role (1, 2): i32 status of bi_check_kept, then for status 0:
//        u32 flag, u32 l_seq, bases, u32 has_qual, qualities (if has_qual), u32 l_name, name, u32 comment bytes, comment, u32 tags left out)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../bwa-mem_gpu_amd/csrc/bam_in_core.h"

static void put32(FILE *f, uint32_t v) { fwrite(&v, 4, 1, f); }

int main(int argc, char **argv)
{
	if (argc != 3) { fprintf(stderr, "usage: %s cases.bin results.bin\n", argv[0]); return 2; }
	FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
	if (!fi || !fo) { fprintf(stderr, "cannot open the files\n"); return 2; }
	uint32_t n = 0;
	if (fread(&n, 4, 1, fi) != 1) return 2;
	for (uint32_t c = 0; c < n; ++c) {
		uint32_t size = 0;
		if (fread(&size, 4, 1, fi) != 1) return 2;
		uint8_t *r = (uint8_t *)malloc(size ? size : 1);
		if (size && fread(r, 1, size, fi) != size) return 2;
		bi_rec_t R;
		const int st = bi_check(r, size, &R);
		put32(fo, (uint32_t)st);
		if (st == BI_OK) {
			const uint32_t role = bi_role(R.flag);
			put32(fo, role);
			if (role == 1 || role == 2) {
				uint32_t hq = 0;
				const int sk = bi_check_kept(r, R, &hq);
				put32(fo, (uint32_t)sk);
				if (sk == BI_OK) {
					put32(fo, R.flag); put32(fo, R.l_seq);
					for (uint32_t i = 0; i < R.l_seq; ++i) fputc(bi_base(r, R, i), fo);
					put32(fo, hq);
					if (hq) for (uint32_t i = 0; i < R.l_seq; ++i) fputc(bi_qual(r, R, i), fo);
					put32(fo, R.l_name); fwrite(r + BI_NAME_OFF, 1, R.l_name, fo);
					uint32_t lo = 0, lo2 = 0;
					const uint32_t cl = bi_comment(r, R, nullptr, 0, &lo);
					uint8_t *cm = (uint8_t *)malloc(cl ? cl : 1);
					const uint32_t cl2 = bi_comment(r, R, cm, cl, &lo2);
					if (cl2 != cl || lo2 != lo) { fprintf(stderr, "case %u: the sizes pass and the write pass disagree\n", c); return 3; }
					put32(fo, cl); fwrite(cm, 1, cl, fo); put32(fo, lo);
					free(cm);
				}
			}
		}
		free(r);
	}
	fclose(fi); fclose(fo);
	return 0;
}
