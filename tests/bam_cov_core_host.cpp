// csrc/bam_cov_core.h and the host form of csrc/bam_cov_host.cpp as plain C++ for tests/test_bam_coverage.py, built with -fsanitize=address,undefined: every
// stream sits in an allocation of exactly its size.
//   in : u32 n_cases, per case i32 min_mapq, i32 deletions, u32 bin, u32 tile, u32 window (records; 0: all in one), u32 n_contigs, i32 length of every contig,
//        u64 n_bytes and the record stream
//   out: per case i32 status (0, or -2: refused); for status 0: u64 n_bins, then n_reads, cov_bases, sum_depth, max_depth, sum_mapq [n_contigs each], hist [1001],
//        bin_sum [n_bins]
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#define BCV_STANDALONE
#include "../bwa-mem_gpu_amd/csrc/bam_cov_host.cpp"

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
		int32_t mq, del; uint32_t bin, tile, window, nc; uint64_t nb;
		if (fread(&mq, 4, 1, f) != 1 || fread(&del, 4, 1, f) != 1 || fread(&bin, 4, 1, f) != 1 || fread(&tile, 4, 1, f) != 1 || fread(&window, 4, 1, f) != 1 || fread(&nc, 4, 1, f) != 1) return 2;
		std::vector<int32_t> len(nc);
		if (nc && fread(len.data(), 4, nc, f) != nc) return 2;
		if (fread(&nb, 8, 1, f) != 1) return 2;
		uint8_t *all = new uint8_t[nb ? nb : 1];
		if (nb && fread(all, 1, nb, f) != nb) return 2;
		std::vector<uint64_t> off(1, 0);
		int32_t rc = BMH_OK;
		for (uint64_t p = 0; p < nb;) {
			const uint64_t sz = bsr_record_bytes(all + p, nb - p);
			if (!sz) { rc = BMH_EINVAL; break; }
			p += sz; off.push_back(p);
		}
		bcv_plan_t P; bcv_host_t H;
		if (rc == BMH_OK) rc = bcv_plan_make(P, mq, del, bin, tile, (int)nc, len.data(), "test");
		if (rc == BMH_OK) {
			H.begin(P);
			const size_t n = off.size() - 1, W = window ? window : (n ? n : 1);
			for (size_t a = 0; a < n && rc == BMH_OK; a += W) rc = H.window(all, off.data() + a, (uint32_t)((a + W < n ? a + W : n) - a), "test");
			if (rc == BMH_OK) rc = H.finish("test");
		}
		fwrite(&rc, 4, 1, o);
		if (rc == BMH_OK) {
			const uint64_t n_bins = P.n_bins();
			fwrite(&n_bins, 8, 1, o);
			for (const std::vector<uint64_t> *v : {&H.R.n_reads, &H.R.cov_bases, &H.R.sum_depth, &H.R.max_depth, &H.R.sum_mapq, &H.R.hist, &H.R.bin_sum})
				if (!v->empty()) fwrite(v->data(), 8, v->size(), o);
		}
		delete[] all;
	}
	fclose(o); fclose(f);
	return 0;
}
