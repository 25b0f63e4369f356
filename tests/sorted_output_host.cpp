// bmh_bam_sorted_file_host and bmh_bam_post_file_host under one bmh_sorted_opt_t with every part on, one refused call per part, and everything released, as a
// stand-alone program for tests/test_sorted_options.py, built from the library's host sources alone (no device code, no HIP runtime) with
// -fsanitize=address,undefined: a record the run writes outside its arrays, an array a failed call leaves behind and one it frees twice are findings.
//   argv[1]: a directory for the SAM file the post-processor reads.  Exit status 0 and "ok" on stdout, or the line that failed on stderr.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../bwa-mem_gpu_amd/csrc/bmh_internal.h"

// what the host sources take from the rest of the library (csrc/c_api.hip, align_pipeline.hip, reads_parse.hip, bam_in_kernels.hip), none of it on the paths run here
static char g_msg[1024];
extern "C" void bmh_set_error(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_msg, sizeof g_msg, fmt, ap); va_end(ap); }
extern "C" const char *bmh_last_error(void) { return g_msg; }
extern "C" int bmh_tune(const char *, int dflt) { return dflt; }
extern "C" int bmh_effective_cpus(void) { return 2; }
void bmh_reads_note_bam_counts(const uint64_t *) {}
void bmh_reads_note_collate_counts(const uint64_t *) {}
int bmh_bam_dev_run(bmh_bam_dev_t *, const bmh_bam_state_t &, const bmh_bam_win_t &, const bmh_batch_alloc_t &, bmh_read_set_t *, bmh_bam_res_t &) { return BMH_ENODEV; }

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "line %d: %s (last message: %s)\n", __LINE__, #c, g_msg); return 1; } } while (0)

static uint8_t *const GARBAGE = (uint8_t *)0xdeadbee0;
static int sink(void *user, const char *b, size_t n) { ((std::string *)user)->append(b, n); return 0; }

// 40 pairs on four positions of contig c, so that most are duplicates; every pair carries NM and an RX barcode (two values a mismatch apart); nm: record 5's NM
static std::string sam_lines(const char *nm)
{
	std::string s;
	const std::string seq(50, 'A'), qual(50, 'I');
	for (int t = 0; t < 40; ++t) {
		char line[512];
		const int pos = 100 + 10 * (t % 4), mate = pos + 150;
		const char *rx = t % 3 ? "ACGTAC" : "ACGTAA";
		snprintf(line, sizeof line, "t%d\t99\tc\t%d\t60\t50M\t=\t%d\t200\t%s\t%s\t%s\tRX:Z:%s\n", t, pos, mate, seq.c_str(), qual.c_str(), t == 2 ? nm : "NM:i:1", rx);
		s += line;
		snprintf(line, sizeof line, "t%d\t147\tc\t%d\t60\t50M\t=\t%d\t-200\t%s\t%s\tNM:i:0\tRX:Z:%s\n", t, mate, pos, seq.c_str(), qual.c_str(), rx);
		s += line;
	}
	return s;
}

struct records_t {
	bmh_markdup_opt_t mo; bmh_coverage_opt_t co; bmh_bam_stats_opt_t so; bmh_sorted_opt_t opt;
	bmh_markdup_counts_t mc; bmh_coverage_t cov; bmh_bam_stats_t st; bmh_sorted_results_t res;
	records_t()
	{
		bmh_markdup_opt_default(&mo); mo.barcode_mode = 1; mo.barcode_tag[0] = 'R'; mo.barcode_tag[1] = 'X'; mo.barcode_edits = 1;
		bmh_coverage_opt_default(&co); co.bin = 10;
		bmh_bam_stats_opt_default(&so); so.insert_cap = 300;
		bmh_sorted_opt_default(&opt); opt.window = 7; opt.index_format = BMH_INDEX_CSI; opt.min_shift = 10; opt.markdup = &mo; opt.coverage = &co; opt.stats = &so;
		memset(&mc, 0xff, sizeof mc); mc.lib_counts = mc.lib_optical = mc.lib_grouped = nullptr;
		memset(&cov, 0xff, sizeof cov); memset(&st, 0xff, sizeof st);          // (a C caller's records are not initialised)
		memset(&res, 0xff, sizeof res); res.markdup = &mc; res.coverage = &cov; res.stats = &st;
	}
	bool all_null() const
	{
		return !cov.n_reads && !cov.cov_bases && !cov.sum_depth && !cov.max_depth && !cov.sum_mapq && !cov.hist && !cov.bin_sum && !st.flag && !st.summary && !st.mapq && !st.contig_mapped &&
		       !st.contig_unmapped && !st.insert_hist && res.parts == 0 && res.coverage_ms == 0 && res.stats_windows == 0;
	}
	void release()
	{
		bmh_free(cov.n_reads); bmh_free(cov.cov_bases); bmh_free(cov.sum_depth); bmh_free(cov.max_depth); bmh_free(cov.sum_mapq); bmh_free(cov.hist); bmh_free(cov.bin_sum);
		bmh_bam_stats_free(&st);
	}
};

// the ways one part each is spoiled: the index, the statistics, the coverage, the marking (a stand-alone file: an optical distance; the post-processor, which has
// an optical step: a barcode mode of 7)
static void spoil(records_t &R, int part, bool post)
{
	if (part == 0) R.opt.min_shift = 9;
	if (part == 1) R.so.insert_cap = 1;
	if (part == 2) R.co.tile = 5000;
	if (part == 3) { if (post) R.mo.barcode_mode = 7; else R.mo.optical_distance = 25; }
}

int main(int argc, char **argv)
{
	if (argc != 2) return 2;
	const char *names[1] = {"c"}; const int32_t lens[1] = {1000};
	const char ctg_blob[] = "c"; const uint32_t ctg_off[2] = {0, 2};
	const std::string good = sam_lines("NM:i:1"), bad = sam_lines("NM:Z:x");
	uint8_t *recs[2] = {nullptr, nullptr}; uint64_t rec_bytes[2] = {0, 0};
	for (int k = 0; k < 2; ++k) {
		const std::string &text = k ? bad : good;
		uint32_t *status = nullptr, n = 0;
		CHECK(bmh_sam_to_bam_host(text.data(), text.size(), 1, ctg_blob, ctg_off, 1, &recs[k], &rec_bytes[k], &status, &n) == BMH_OK && n == 80);
		for (uint32_t i = 0; i < n; ++i) CHECK(status[i] == 0);
		bmh_free(status);
	}

	// the stand-alone file: every part on
	uint64_t flagged = 0;
	{
		records_t R;
		uint8_t *bam = GARBAGE, *index = GARBAGE; uint64_t nb = 7, ni = 7;
		CHECK(bmh_bam_sorted_file_host("@HD\tVN:1.6\n", 1, names, lens, recs[0], rec_bytes[0], &R.opt, &bam, &nb, &index, &ni, &R.res) == BMH_OK);
		CHECK(bam && index && nb > 28 && ni > 28 && R.res.parts == (BMH_SORTED_MARKDUP | BMH_SORTED_BARCODE | BMH_SORTED_GROUPED | BMH_SORTED_COVERAGE | BMH_SORTED_STATS));
		CHECK(R.mc.counts[7] == 40 && R.mc.counts[2] > 20 && R.mc.grouped[1] < R.mc.grouped[0] && R.res.n_libraries == 0 && R.res.markdup_ms[0] == 0 && R.res.coverage_windows == 0);
		flagged = R.mc.counts[4];
		CHECK(R.st.flag[0] == 80 && R.st.flag[4] == flagged && R.st.n_contigs == 1 && R.st.insert_cap == 300);
		CHECK(R.cov.n_contigs == 1 && R.cov.n_bins == 100 && R.cov.n_reads[0] == 80 - flagged);
		bmh_free(bam); bmh_free(index); R.release();
	}
	// ... one refused call per part, and a refused record
	for (int part = 0; part < 5; ++part) {
		records_t R;
		spoil(R, part, false);
		uint8_t *bam = GARBAGE, *index = GARBAGE; uint64_t nb = 7, ni = 7;
		CHECK(bmh_bam_sorted_file_host("@HD\tVN:1.6\n", 1, names, lens, recs[part == 4], rec_bytes[part == 4], &R.opt, &bam, &nb, &index, &ni, &R.res) == BMH_EINVAL);
		CHECK(!bam && !index && R.all_null());
		if (part == 4) CHECK(strstr(g_msg, "has an NM tag that is no count"));
	}
	// ... and a record the options ask for that is not there
	for (int part = 0; part < 3; ++part) {
		records_t R;
		if (part == 0) R.res.markdup = nullptr;
		if (part == 1) R.res.coverage = nullptr;
		if (part == 2) R.res.stats = nullptr;
		uint8_t *bam = GARBAGE, *index = GARBAGE; uint64_t nb = 7, ni = 7;
		CHECK(bmh_bam_sorted_file_host("@HD\tVN:1.6\n", 1, names, lens, recs[0], rec_bytes[0], &R.opt, &bam, &nb, &index, &ni, &R.res) == BMH_EINVAL);
		CHECK(!bam && !index && strstr(g_msg, "null argument (") && (part == 1 || !R.cov.hist) && (part == 2 || !R.st.flag));
	}

	// the post-processor on the same records as SAM text: the same record inside its own
	const std::string header = "@SQ\tSN:c\tLN:1000\n";
	std::string path[2];
	for (int k = 0; k < 2; ++k) {
		path[k] = std::string(argv[1]) + (k ? "/bad.sam" : "/good.sam");
		FILE *f = fopen(path[k].c_str(), "wb");
		CHECK(f);
		const std::string text = header + (k ? bad : good);
		CHECK(fwrite(text.data(), 1, text.size(), f) == text.size());
		fclose(f);
	}
	{
		records_t R;
		bmh_bam_post_opt_t po; bmh_bam_post_opt_default(&po); po.sorted = R.opt; po.batch_bytes = 2000;
		bmh_bam_post_result_t out; memset(&out, 0xff, sizeof out);
		std::string file;
		CHECK(bmh_bam_post_file_host(path[0].c_str(), &po, sink, &file, &out, &R.res) == BMH_OK);
		CHECK(out.index && out.index_bytes > 28 && out.counts.records == 80 && out.counts.batches > 1 && file.size() > 56);
		CHECK(R.mc.counts[7] == 40 && R.mc.counts[4] == flagged && R.st.flag[0] == 80 && R.st.flag[4] == flagged && R.cov.n_reads[0] == 80 - flagged);
		bmh_bam_post_result_free(&out); R.release();
	}
	for (int part = 0; part < 5; ++part) {
		records_t R;
		spoil(R, part, true);
		bmh_bam_post_opt_t po; bmh_bam_post_opt_default(&po); po.sorted = R.opt;
		bmh_bam_post_result_t out; memset(&out, 0xff, sizeof out);
		std::string file;
		CHECK(bmh_bam_post_file_host(part == 4 ? path[1].c_str() : "/nonexistent/never-opened.sam", &po, sink, &file, &out, &R.res) == BMH_EINVAL);
		CHECK(!out.index && !out.header_text && !out.contig_names && !out.contig_len && !out.library_names && R.all_null() && (part == 4 || file.empty()));
	}
	bmh_free(recs[0]); bmh_free(recs[1]);
	printf("ok\n");
	return 0;
}
