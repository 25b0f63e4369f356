// Flagstat, idxstats, alignment summary and insert sizes, internal: the plan, the result and the host form (csrc/bam_stats_host.cpp) and what
// csrc/bam_stats_kernels.hip offers csrc/bam_sort_kernels.hip, csrc/align_pipeline.hip and csrc/bam_post_kernels.hip.  Both forms take the sorted file's windows of
// records one after the other; nothing but the accumulators and the number of records seen passes from one window to the next.
#pragma once
#include <stdint.h>
#include <vector>
#ifndef BST_STANDALONE
#include "bmh_internal.h"
#else                                                              // tests/bam_stats_core_host.cpp: the host form alone, without the library
enum { BMH_OK = 0, BMH_EINVAL = -2, BMH_ENOMEM = -4 };
void bmh_set_error(const char *fmt, ...);
#endif
#include "bam_stats_core.h"

// what a statistics run is made under, checked
struct bst_plan_t {
	uint32_t cap = BST_CAP_MAX; int n_contigs = 0;
	size_t hist_words() const { return (size_t)BST_N_ORI * ((size_t)cap + 1); }
	// the accumulator: the fixed words, then mapped [n_contigs], unmapped [n_contigs], then the histograms
	size_t w_contig() const { return (size_t)BST_W_FIXED; }
	size_t w_hist() const { return (size_t)BST_W_FIXED + 2 * (size_t)n_contigs; }
	size_t words() const { return w_hist() + hist_words(); }
};
// insert_cap as the entry points take it.  Refused (BMH_EINVAL, a message): a cap outside 2 .. 65536, a negative number of contigs
int bst_plan_make(bst_plan_t &P, uint32_t insert_cap, int n_contigs, const char *fn);

// the results: the accumulator's words (minima of orientations without a pair: 0 once finished)
struct bst_result_t {
	std::vector<uint64_t> w;
	void init(const bst_plan_t &P);
	void close(const bst_plan_t &P);
};

// the message of the record with index `rec` that bst_record refuses with `code`
int bst_refused(uint64_t rec, int code, const char *fn);

// the host form
struct bst_host_t {
	bst_plan_t P; bst_result_t R; uint64_t n_seen = 0;
	void begin(const bst_plan_t &plan);
	// a window's n records recs + soff[j], in any order; the first record refused ends the run
	int window(const uint8_t *recs, const uint64_t *soff, uint32_t n, const char *fn);
	void finish() { R.close(P); }
};

#ifndef BST_STANDALONE
struct bmh_bam_stats;
// the offsets of a stream's records, whole ones only (a refID out of range is the record's own refusal, in its turn: bsr_walk would name it first)
int bst_walk(const uint8_t *recs, uint64_t n_bytes, std::vector<uint64_t> &off, const char *fn);
// R as the entry points return it (malloc'd arrays; *out zeroed first)
int bst_export(const bst_plan_t &P, const bst_result_t &R, struct bmh_bam_stats *out, const char *fn);

// csrc/bam_stats_kernels.hip
struct bst_dev_t;                                                  // the device form's accumulator and state; one per sorted run
bst_dev_t *bst_dev_create(void);
void bst_dev_free(bst_dev_t *d);
int bst_begin_device(bst_dev_t *d, const bst_plan_t &P, void *stream);
// a window's records d_recs at d_soff [n + 1] (device): one kernel, and the refusal word on its way to the host.  With ms (or NULL) events are recorded around the
// kernel.  Nothing waits here: bst_window_ms, once the caller has waited for the stream, refuses the window by its first refused record (fn names the caller) and,
// with ms, ms[0] += the kernel's milliseconds, ms[1] += 1 (the windows timed)
int bst_window_device(bst_dev_t *d, const uint8_t *d_recs, const uint64_t *d_soff, uint32_t n, void *stream, double *ms);
int bst_window_ms(bst_dev_t *d, double *ms, const char *fn);
// the results: the run's one read of the accumulator
int bst_finish_device(bst_dev_t *d, void *stream, bst_result_t &R, const char *fn);
#endif
