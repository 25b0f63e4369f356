// Sort, mark and index a BAM or SAM of any aligner, internal: the input and the run that csrc/bam_post.cpp (the reader, the checks' words, the host
// form) and csrc/bam_post_kernels.hip (the kernels, the device form) share.
#pragma once
#include <stdint.h>
#include <functional>
#include <string>
#include <vector>
#include "bmh_internal.h"
#include "bam_sort.h"
#include "bam_dup.h"
#include "bam_cov.h"
#include "bam_stats.h"
#include "bam_post_core.h"

#define BPO_BATCH_DEFAULT (256ull << 20)
#define BPO_BATCH_MAX (1ull << 30)

// SAM record lines (every line ends with '\n', but perhaps the input's last) -> their records appended to recs; *bad: the first refused line (or ~0u) and *status why
typedef std::function<int(const char *text, size_t n, int n_contigs, const std::string &ctg_blob, const std::vector<uint32_t> &ctg_noff, std::vector<uint8_t> &recs, uint32_t *bad, uint32_t *status)> bpo_convert_t;

// The input: its header, and its records batch by batch in file order.  A batch ends at the first template head (BDP_TPL_NAME: the name differs from the
// predecessor's) at or beyond batch_bytes, found by comparing names forward from there, so no template is split -- across the windows the bytes arrive in either
struct bpo_input_t {
	bmh_text_src_t *src = nullptr; std::string path; bool bam = false, eof = false, src_eof = false;
	std::string header;                                                // the output header's text
	std::vector<std::string> names; std::vector<int32_t> len; std::string ctg_blob; std::vector<uint32_t> ctg_noff;
	std::vector<uint8_t> buf; size_t have = 0, taken = 0;                // record bytes not handed out yet: buf [0, have); the last batch: buf [0, taken)
	std::vector<uint32_t> chain; size_t chunk = 8u << 20;
	std::vector<uint64_t> off; uint32_t n = 0; uint64_t base = 0;       // the batch: records buf + off [i], i < n; base: the file index of its first
	std::string text; uint64_t lines = 0; bpo_convert_t convert;         // SAM: text not converted yet, the lines before it
	uint64_t header_lines = 0;                                         // SAM: the lines of the header (record i is line header_lines + i + 1)
	bool plain = false;                                                // BDP_TPL_FILE: a batch ends at the first record at or beyond batch_bytes, no name is compared
	~bpo_input_t() { if (src) bmh_text_close(src); }
	int open(const char *p, const char *fn, bpo_convert_t conv);
	int next(uint64_t batch_bytes, const char *fn);                    // 1: a batch; 0: the end; < 0: refused
private:
	int fill(const char *fn);
	int sam_header(const char *fn);
	int bam_header(const char *fn);
};

// one run: the options, the sorted output as checked (csrc/bam_sort.h: the plans, the index), the input, the counts
struct bpo_run_t {
	const char *fn = ""; bmh_bam_post_opt_t o; uint32_t mode = 0;
	bmh_markdup_opt_t mo; bmh_rg_table_t rg; std::vector<const char *> rg_ids;
	bsr_out_t J; bpo_input_t in; bmh_bam_post_counts_t counts = {0, 0, 0, 0, 0, 0};
	bool collate = false;                                              // templates by name over the whole file (BDP_TPL_FILE, csrc/bam_tpl_core.h)
	uint64_t sam_line0() const { return in.bam ? 0 : in.header_lines + 1; }      // the SAM line of record 0 (0: a BAM)
	std::vector<const char *> name_ptr;
	// out and res zeroed; every option that needs no contig checked before the input is touched, then the input opened and the rest checked over its contigs
	int begin(const char *path, const bmh_bam_post_opt_t *opt, bmh_sam_sink_t sink, bmh_bam_post_result_t *out, bmh_sorted_results_t *res, const char *f, bpo_convert_t conv);
	int header_members(std::string &members) const;                    // the header as BGZF members of the run's level
	// behind a form's run (rc; base: the header members' bytes): the end-of-file member to the sink, the index bytes, the arrays of res and of out (malloc'd); a
	// failed run, or a step that fails here, leaves out's pointers and every array of res NULL
	int end(int rc, uint64_t base, bmh_sam_sink_t sink, void *user, bmh_bam_post_result_t *out, bmh_sorted_results_t *res);
private:
	int finish(const std::string &index_bytes, bmh_bam_post_result_t *out) const;
};
// the message of the record with file index `index` that bpo_check refuses with `code` (rec: its sz bytes)
int bpo_refused(const char *fn, uint64_t index, int code, const uint8_t *rec, uint64_t sz, int n_ref);
// the first record of the template that holds record i of a batch: the templates before it are whole and can still be judged
uint32_t bpo_template_start(const uint8_t *recs, const uint64_t *off, uint32_t i);
