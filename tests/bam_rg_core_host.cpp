// bi_read_group of csrc/bam_in_core.h as plain C++ under AddressSanitizer and UBSan (tests/test_keep_rg.py builds and runs this): every record is a heap block of
// exactly its size, the table's IDs one heap block of exactly their bytes and its offsets one of exactly n + 1 words, so a read one byte outside a record, an ID
// or the offsets is reported.
//   in : u32 n_groups, then n_groups x (u32 len, bytes); u32 n, then n x (u32 size, bytes)
//   out: n x (i32 status of bi_check, then for status 0: i32 status of bi_read_group, u32 group (0 unless that status is 0))
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
	uint32_t ng = 0;
	if (fread(&ng, 4, 1, fi) != 1) return 2;
	std::vector<uint8_t> ids; std::vector<uint32_t> off(1, 0u);
	for (uint32_t g = 0; g < ng; ++g) {
		uint32_t len = 0;
		if (fread(&len, 4, 1, fi) != 1) return 2;
		const size_t at = ids.size();
		ids.resize(at + len);
		if (len && fread(ids.data() + at, 1, len, fi) != len) return 2;
		off.push_back((uint32_t)ids.size());
	}
	uint8_t *hid = (uint8_t *)malloc(ids.size() ? ids.size() : 1);
	uint32_t *hoff = (uint32_t *)malloc(4 * off.size());
	memcpy(hid, ids.data(), ids.size()); memcpy(hoff, off.data(), 4 * off.size());
	const bi_groups_t G = {hid, hoff, ng};
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
			uint32_t g = 0;
			const int sg = bi_read_group(r, R, G, &g);
			put32(fo, (uint32_t)sg); put32(fo, sg == BI_OK ? g : 0u);
		}
		free(r);
	}
	free(hid); free(hoff);
	fclose(fi); fclose(fo);
	return 0;
}
