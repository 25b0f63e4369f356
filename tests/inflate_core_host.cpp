// csrc/inflate_core.h as plain C++ for tests/test_inflate.py, built with -fsanitize=address,undefined: every member's input and output live in heap blocks
// of exactly their sizes, so a read or write one byte outside them is a sanitizer report (and a non-zero exit).
//   inflate_core_host <cases> <results>
// cases:   u32 n, then per member u32 in_len, u32 isize, u32 crc32, in_len bytes of raw deflate data
// results: per member u32 status, u32 bytes produced, u32 crc32 of them (computed here, bit by bit), and the bytes themselves when the status is 0
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../bwa-mem_gpu_amd/csrc/inflate_core.h"

static uint32_t crc_bitwise(const uint8_t *p, uint32_t n)
{
	uint32_t c = 0xffffffffu;
	for (uint32_t i = 0; i < n; ++i) { c ^= p[i]; for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1; }
	return c ^ 0xffffffffu;
}

int main(int argc, char **argv)
{
	if (argc != 3) { fprintf(stderr, "usage: inflate_core_host <cases> <results>\n"); return 2; }
	FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
	if (!fi || !fo) { perror("open"); return 2; }
	uint32_t n = 0;
	if (fread(&n, 4, 1, fi) != 1) return 2;
	inf_host_ws_t *ws = new inf_host_ws_t();
	for (uint32_t i = 0; i < n; ++i) {
		uint32_t h[3];
		if (fread(h, 4, 3, fi) != 3) return 2;
		const uint32_t cap = h[1] < INF_MAX_OUT ? h[1] : INF_MAX_OUT;
		uint8_t *in = (uint8_t *)malloc(h[0] ? h[0] : 1), *out = (uint8_t *)malloc(cap ? cap : 1);
		if (h[0] && fread(in, 1, h[0], fi) != h[0]) return 2;
		uint32_t got = 0;
		const uint32_t st = (uint32_t)inf_member(*ws, in, h[0], out, h[1], h[2], &got);
		if (got > cap) { fprintf(stderr, "member %u: %u bytes produced, %u allowed\n", i, got, cap); return 3; }
		const uint32_t r[3] = {st, got, crc_bitwise(out, got)};
		fwrite(r, 4, 3, fo);
		if (st == 0) fwrite(out, 1, got, fo);
		free(in); free(out);
	}
	delete ws;
	fclose(fi);
	if (fclose(fo) != 0) return 2;
	return 0;
}
