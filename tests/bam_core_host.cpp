// csrc/bam_core.h as plain C++ for tests/test_bam_core.py, built with -fsanitize=address,undefined: every line and every record live in heap blocks of exactly
// their sizes, so a read or write one byte outside them is a sanitizer report (and a non-zero exit).
//   bam_core_host <cases> <results>
// cases:   u32 n_contigs, u32 blob bytes, the names (NUL-terminated, back to back), u32 off[n_contigs + 1]; u32 n_lines, then per line u32 len, u32 has_eol, the bytes
// results: per line u32 status, u32 bytes, the record when the status is 0
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../bwa-mem_gpu_amd/csrc/bam_core.h"

int main(int argc, char **argv)
{
	if (argc != 3) { fprintf(stderr, "usage: bam_core_host <cases> <results>\n"); return 2; }
	FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
	if (!fi || !fo) { perror("open"); return 2; }
	uint32_t nc = 0, nb = 0, n = 0;
	if (fread(&nc, 4, 1, fi) != 1 || fread(&nb, 4, 1, fi) != 1) return 2;
	char *blob = (char *)malloc(nb ? nb : 1); uint32_t *off = (uint32_t *)malloc(4 * (nc + 1));
	if (nb && fread(blob, 1, nb, fi) != nb) return 2;
	if (fread(off, 4, nc + 1, fi) != nc + 1) return 2;
	bam_refs_t R; R.names = blob; R.off = off; R.n = (int)nc;
	if (fread(&n, 4, 1, fi) != 1) return 2;
	for (uint32_t i = 0; i < n; ++i) {
		uint32_t h[2];
		if (fread(h, 4, 2, fi) != 2) return 2;
		uint8_t *line = (uint8_t *)malloc(h[0] ? h[0] : 1);
		if (h[0] && fread(line, 1, h[0], fi) != h[0]) return 2;
		uint32_t sz = 0, sz2 = 0;
		uint32_t st = bam_record(line, h[0], R, nullptr, 0, &sz);
		if (st == BAM_OK && !h[1]) st = BAM_ENOEOL;
		uint8_t *rec = nullptr;
		if (st == BAM_OK) {
			rec = (uint8_t *)malloc(sz);
			const uint32_t st2 = bam_record(line, h[0], R, rec, sz, &sz2);
			if (st2 != BAM_OK || sz2 != sz) { fprintf(stderr, "line %u: the write pass gives status %u, %u bytes; the sizes pass %u bytes\n", i, st2, sz2, sz); return 3; }
		}
		const uint32_t r[2] = {st, st == BAM_OK ? sz : 0};
		fwrite(r, 4, 2, fo);
		if (st == BAM_OK) fwrite(rec, 1, sz, fo);
		free(rec); free(line);
	}
	free(blob); free(off);
	fclose(fi);
	return fclose(fo) != 0 ? 2 : 0;
}
