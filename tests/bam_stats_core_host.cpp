// csrc/bam_stats_core.h and the host form of csrc/bam_stats_host.cpp as plain C++ for tests/test_bam_stats.py, built with -fsanitize=address,undefined: every
// stream sits in an allocation of exactly its size.
//   in : u32 n_cases, per case u32 n_contigs, u32 insert_cap, u32 window (records; 0: all in one), u64 n_bytes and the record stream
//   out: per case i32 status (0, or -2: refused), u64 the refused record's index, i32 its code (both 0 unless a record was refused); for status 0 the
//        accumulator's words: flag [2][16], summary [14], mapq [256], insert_min [3], insert_max [3], unplaced, contig_mapped and contig_unmapped [n_contigs each],
//        insert_hist [3][insert_cap + 1]
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#define BST_STANDALONE
#include "../bwa-mem_gpu_amd/csrc/bam_stats_host.cpp"

static char g_msg[512];
void bmh_set_error(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_msg, sizeof g_msg, fmt, ap); va_end(ap); }

int main(int argc, char **argv)
{
	if (argc != 3) return 2;
	FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
	if (!f || !o) return 2;
	uint32_t n_cases;
	if (fread(&n_cases, 4, 1, f) != 1) return 2;
	for (uint32_t c = 0; c < n_cases; ++c) {
		uint32_t nc, cap, window; uint64_t nb;
		if (fread(&nc, 4, 1, f) != 1 || fread(&cap, 4, 1, f) != 1 || fread(&window, 4, 1, f) != 1 || fread(&nb, 8, 1, f) != 1) return 2;
		uint8_t *all = new uint8_t[nb ? nb : 1];
		if (nb && fread(all, 1, nb, f) != nb) return 2;
		std::vector<uint64_t> off(1, 0);
		int32_t rc = BMH_OK, code = 0; uint64_t index = 0;
		for (uint64_t p = 0; p < nb;) {
			const uint64_t sz = bsr_record_bytes(all + p, nb - p);
			if (!sz) { rc = BMH_EINVAL; break; }
			p += sz; off.push_back(p);
		}
		bst_plan_t P; bst_host_t H;
		if (rc == BMH_OK) rc = bst_plan_make(P, cap, (int)nc, "test");
		if (rc == BMH_OK) {
			H.begin(P);
			const size_t n = off.size() - 1, W = window ? window : (n ? n : 1);
			for (size_t a = 0; a < n && rc == BMH_OK; a += W) rc = H.window(all, off.data() + a, (uint32_t)((a + W < n ? a + W : n) - a), "test");
			if (rc == BMH_OK) H.finish();
			else {                                                       // the record the host form stopped at, and why
				bst_rec_t r;
				index = H.n_seen; code = bst_record(all + off[index], off[index + 1] - off[index], (int)nc, r);
			}
		}
		fwrite(&rc, 4, 1, o); fwrite(&index, 8, 1, o); fwrite(&code, 4, 1, o);
		if (rc == BMH_OK) fwrite(H.R.w.data(), 8, H.R.w.size(), o);
		delete[] all;
	}
	fclose(o); fclose(f);
	return 0;
}
