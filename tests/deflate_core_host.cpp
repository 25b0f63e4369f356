// csrc/deflate_core.h as plain C++ for tests/test_bam_core.py, built with -fsanitize=address,undefined: every piece lives in a heap block of exactly its
// size and every member in a zeroed block of exactly dfl_bound(size) bytes, so a read or write outside them is a sanitizer report (and a non-zero exit).
//   deflate_core_host <cases> <results> [<trace>]
// cases:   u32 n, then per piece u32 level, u32 len (1 .. 0xff00), the bytes
// results: per piece u32 member bytes, the member
// trace:   per piece u32 form (BTYPE: 0 stored, 2 dynamic), u32 the bits dfl_member estimated for the dynamic block (level 1; it leaves them in u1), then what
//          its state holds behind the call: u8 llen[286], dlen[30], cllen[19], u32 lfreq[286], dfreq[30], clfreq[19] (the tokens' counts)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../bwa-mem_gpu_amd/csrc/deflate_core.h"

int main(int argc, char **argv)
{
	if (argc != 3 && argc != 4) { fprintf(stderr, "usage: deflate_core_host <cases> <results> [<trace>]\n"); return 2; }
	FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb"), *ft = argc == 4 ? fopen(argv[3], "wb") : nullptr;
	if (!fi || !fo || (argc == 4 && !ft)) { perror("open"); return 2; }
	uint32_t n = 0;
	if (fread(&n, 4, 1, fi) != 1) return 2;
	dfl_state_t *sh = new dfl_state_t();
	for (uint32_t i = 0; i < n; ++i) {
		uint32_t h[2];
		if (fread(h, 4, 2, fi) != 2 || h[1] < 1 || h[1] > DFL_PIECE) return 2;
		uint8_t *in = (uint8_t *)malloc(h[1]);
		if (fread(in, 1, h[1], fi) != h[1]) return 2;
		uint32_t *out = (uint32_t *)calloc(dfl_bound(h[1]), 1);
		const uint32_t sz = dfl_member(*sh, in, h[1], out, (int)h[0]);
		if (sz > h[1] + 31) { fprintf(stderr, "piece %u: a member of %u bytes for %u bytes\n", i, sz, h[1]); return 3; }
		fwrite(&sz, 4, 1, fo); fwrite(out, 1, sz, fo);
		if (ft) {
			const uint32_t t[2] = { (uint32_t)(((const uint8_t *)out)[18] >> 1) & 3u, h[0] >= 1 ? sh->u1 : 0u };
			fwrite(t, 4, 2, ft);
			fwrite(sh->llen, 1, 286, ft); fwrite(sh->dlen, 1, 30, ft); fwrite(sh->cllen, 1, 19, ft);
			fwrite(sh->lfreq, 4, 286, ft); fwrite(sh->dfreq, 4, 30, ft); fwrite(sh->clfreq, 4, 19, ft);
		}
		free(in); free(out);
	}
	delete sh;
	fclose(fi);
	if (ft && fclose(ft) != 0) return 2;
	return fclose(fo) != 0 ? 2 : 0;
}
