// Sorted BAM output, internal: the index being built over a file's windows, the run store, and what csrc/bam_sort_kernels.hip offers csrc/align_pipeline.hip.
#pragma once
#include <stdint.h>
#include <string>
#include <vector>
#include "bmh_internal.h"
#include "bam_sort_core.h"
#include "bam_dup.h"
#include "bam_tpl.h"
#include "bam_cov.h"
#include "bam_stats.h"
#include "bam_recal.h"

typedef int (*bsr_sink_t)(void *user, const char *bytes, size_t n);

// a chunk's first record: its reference (-1: the group without one), bin and virtual offset (relative to the sink's first byte)
struct bsr_head_t { int32_t ref; uint32_t bin; uint64_t beg; };

// The index of one file, filled window after window (heads in file order; lin, counts: on the host form directly, on the device form copied back at the end)
struct bsr_index_t {
	int n_ref = 0;
	std::vector<uint32_t> n_win; std::vector<uint64_t> lin_off;    // windows of every reference, their places in lin [n_ref + 1]
	std::vector<uint64_t> lin;                                     // smallest begin offset per window, ~0: none
	std::vector<uint64_t> counts;                                  // [2 r]: mapped, [2 r + 1]: unmapped records of reference r; [2 n_ref]: records without one
	std::vector<bsr_head_t> heads;
	uint64_t file_pos = 0;                                         // bytes handed to the sink so far
	int format = BSR_IX_BAI, min_shift = BSR_LIN_SHIFT, depth = BSR_BAI_DEPTH;      // the binning scheme: BAI's (14, 5), or CSI's min_shift and the depth its longest contig asks for
	// BAI: contigs below 2^29 bases; CSI: any length an int32 holds, min_shift in 10 .. 24, and a lin array that fits (counted before it is allocated)
	int init(int n_contigs, const int32_t *contig_len, const char *fn, int format = BSR_IX_BAI, int min_shift = BSR_LIN_SHIFT);
	// one window on the host: its n records recs [soff[n]], its members' offsets moff [n_members + 1]
	void window_host(const uint8_t *recs, const uint64_t *soff, uint32_t n, const uint64_t *moff);
	// the .bai bytes; base_offset: bytes in the file before the sink's first
	void bai(uint64_t base_offset, std::string &out) const;
	// the .csi bytes of a CSI index: the index as BGZF members (level 1) and the end-of-file member
	int csi(uint64_t base_offset, std::string &out) const;
	// the index file of `format`
	int bytes(uint64_t base_offset, std::string &out) const { if (format == BSR_IX_CSI) return csi(base_offset, out); bai(base_offset, out); return 0; }
};

// duplicate marking keeps u + 2^30 in 31 bits (csrc/bam_dup_core.h): every contig at most BDP_MAX_CONTIG bases, else refused naming the first longer one
int bsr_markdup_contigs(int n_contigs, const int32_t *contig_len, const char *const *contig_names, const char *fn);
// format and min_shift as the entry points take them: BMH_EINVAL with a message, or BMH_OK
int bsr_index_format_check(int format, int min_shift, const char *fn);

// One sorted output, checked: what bmh_sorted_opt_t asks for as plans (markdup, coverage, stats: which of them are on), the index being built, and what the run
// leaves behind -- the marking's counts where P points (the caller's bmh_markdup_counts_t), the coverage and the statistics as the device or the host form finished
// them (bsr_out_export makes the caller's arrays of them), and, for a timed run (the aligner's), the milliseconds: dup_ms [3] the decision, the windows' flag steps
// and the bytes of ordinals and entries that came down with the batches; opt_ms the optical step; cov_ms / stats_ms [2] the steps and the windows timed
struct bsr_out_t {
	int level = 1; uint32_t window = 0;
	bool markdup = false, coverage = false, stats = false, timed = false, recal = false, requal = false;
	bdp_plan_t P; bcv_plan_t CP; bst_plan_t SP;
	brc_run_t RU; brc_result_t RR; double recal_ms[2] = {0, 0};    // the recalibration table: its checked run, its words, its windows' milliseconds
	const uint8_t *recal_d_pac = nullptr;                          // ... the reference on the device where the caller holds one (the aligner's index), else RU.pac goes up
	brq_run_t QU; brq_result_t QR; double requal_ms[2] = {0, 0};   // applying a table to the qualities: the checked table, the counts, the windows' milliseconds
	bsr_index_t ix;
	uint64_t *dup_counts = nullptr;                                // [BDP_N_COUNTS], with markdup
	bcv_result_t CR; bst_result_t SR;
	double dup_ms[3] = {0, 0, 0}, opt_ms = 0, cov_ms[2] = {0, 0}, stats_ms[2] = {0, 0};
	uint32_t parts() const;                                        // BMH_SORTED_*: what a run under these plans computes
};
// opt (NULL: the defaults) and the results record as every sorted output takes them, over these contigs -> J.  *res, the records it names and J are zeroed first;
// then, in this order: the level; the index format and the contigs it holds (J.ix: the index of a file without records); marking -- its record in res, the
// options (bdp_plan_make's order), the contigs marking holds; coverage -- its record, bcv_plan_make; the statistics -- their record, bst_plan_make.  BMH_EINVAL
// with a message, or BMH_OK.  res NULL: as a record of NULLs
int bsr_out_make(bsr_out_t &J, const bmh_sorted_opt_t *opt, int n_contigs, const int32_t *contig_len, const char *const *contig_names, bmh_sorted_results_t *res, const char *fn);
// the coverage and the statistics of a finished J -> res's records (malloc'd arrays), J's milliseconds -> res
int bsr_out_export(const bsr_out_t &J, bmh_sorted_results_t *res, const char *fn);
// every array of res's coverage and statistics released, the records zeroed (a failed call's cleanup; res or its records may be NULL)
void bsr_results_release(bmh_sorted_results_t *res);

// Sorted runs kept until the end of the input: the records in host memory up to mem_bytes, beyond that in one unnamed temporary file; keys and offsets
// (16 bytes per record) always in memory.  With duplicate marking (csrc/bam_dup_core.h) a run also keeps every record's template ordinal within its batch (tpl, 4 bytes
// per record, outside the budget like keys and offsets) and the ordinal of its first template in the whole run (tbase); the store keeps the templates' entries
struct bsr_run_t { uint64_t n = 0, bytes = 0; std::vector<uint64_t> keys, off; uint8_t *mem = nullptr; int64_t file_at = -1; std::vector<uint32_t> tpl; uint64_t tbase = 0; };
struct bsr_dup_t { const uint32_t *tpl; const bdp_entry_t *entries; uint32_t n_tpl; uint64_t secsup, unmapped; int lib = -1; const uint32_t *lib3 = nullptr; uint32_t n_lib3 = 0; const bdp_loc_t *locs = nullptr; const uint64_t *bcs = nullptr; };      // what a batch adds when duplicates are marked; lib: the library of the batch's read group (-1: a run without groups); lib3 [3 * n_lib3]: a batch of several libraries -- every library's secondary / supplementary records, unmapped records and templates (lib stays -1); locs [n_tpl] (or NULL): the templates' locations, when optical duplicates are counted; bcs [n_tpl] (or NULL): the templates' barcode words, when barcodes are compared
struct bsr_store_t {
	uint64_t mem_bytes = 4ull << 30, used = 0, spilled = 0; std::string tmp_dir; int fd = -1; uint64_t file_bytes = 0;
	std::vector<bsr_run_t> runs;
	std::vector<bdp_entry_t> entries; uint64_t dup_info[2] = {0, 0};         // duplicate marking: every template's entry in input order; secondary / supplementary and unmapped records
	std::vector<bdp_loc_t> locs;                                             // ... when optical duplicates are counted: every template's location beside its entry (else empty)
	std::vector<uint64_t> bcs;                                               // ... when barcodes are compared: every template's barcode word beside its entry (else empty)
	std::vector<uint64_t> lib_info;                                          // ... with read groups, per library: those two and the templates [3 * libraries]
	// templates by name over the whole file (BDP_TPL_FILE, csrc/bam_tpl_core.h): every record's part in file order -- host memory outside the budget, like the keys:
	// 32 bytes per record (16 and 8 more with locations and barcodes), never spilled.  A run's tpl then holds the records' batch indices in sorted order and tbase
	// the file index of the batch's first record, until retemplate
	btp_parts_t tpl_parts;
	// rec_tpl [records of the file]: every record's template ordinal -> every run's tpl [i] = rec_tpl [tbase + tpl [i]], tbase = 0: what the merge reads
	void retemplate(const std::vector<uint32_t> &rec_tpl);
	~bsr_store_t() { clear(); }
	void clear();
	int append(const uint8_t *recs, uint64_t bytes, const uint64_t *keys, const uint64_t *off, uint64_t n, const bsr_dup_t *dup = nullptr);
	int read(const bsr_run_t &r, uint64_t a, uint64_t b, uint8_t *dst) const;       // bytes [a, b) of the run's records
};

// csrc/bam_sort_host.cpp: records (walked, checked) -> sorted order on the host
int bsr_walk(const uint8_t *recs, uint64_t n_bytes, int n_ref, std::vector<uint64_t> &off, const char *fn);
void bsr_sort_host(const uint8_t *recs, const std::vector<uint64_t> &off, std::vector<uint64_t> &keys, std::vector<uint32_t> &ord);
// the host form of a sorted output's run: records recs at off (flags as marking left them) in the order ord [n] -> the record members of the sorted file, window
// after window, to the sink; J.ix, and with J.coverage / J.stats J.CR / J.SR from the same windows
int bsr_write_host(const uint8_t *recs, const uint64_t *off, const uint32_t *ord, uint64_t n, bsr_out_t &J, bsr_sink_t sink, void *user, const char *fn);

// A stand-alone sorted file in the making: what bmh_bam_sorted_file_device and _host share.  begin: *bam and *index NULL before anything can be refused, the
// options (bsr_out_make; an optical distance is refused: a stand-alone file has no optical step), the arguments, the stream walked (off), the header members
// (file).  end: behind a form's records -- the end-of-file member, the index bytes, the results' arrays, the caller's copies; a failed call (rc, or a step of
// end itself) leaves *bam, *index and every array of the results NULL
struct bsr_file_t {
	const char *fn = ""; bsr_out_t J; std::vector<uint64_t> off; std::string file; uint64_t base = 0;
	uint8_t **bam = nullptr, **index = nullptr; uint64_t *bam_bytes = nullptr, *index_bytes = nullptr;
	int begin(const char *f, const char *header_text, int n_contigs, const char *const *contig_names, const int32_t *contig_len, const uint8_t *recs, uint64_t n_bytes,
	          const bmh_sorted_opt_t *opt, uint8_t **bam_, uint64_t *bam_bytes_, uint8_t **index_, uint64_t *index_bytes_, bmh_sorted_results_t *res);
	int end(int rc, bmh_sorted_results_t *res);
};
inline int bsr_sink_string(void *user, const char *b, size_t n) { ((std::string *)user)->append(b, n); return 0; }

// csrc/bam_sort_kernels.hip
struct bsr_dev_t;                                                 // device buffers of the sort, the gather and the index pass; kept between calls
bsr_dev_t *bsr_dev_create(void);
void bsr_dev_free(bsr_dev_t *d);
// a batch's records d_recs with offsets d_off [n + 1] (device) -> the sorted run: *d_sorted (total bytes), *d_keys [n], *d_soff [n + 1], all in d until its next call
// d_side [n] (device, or NULL): a word per record that follows it through the sort -> *d_side_sorted [n]
int bsr_sort_run_device(bsr_dev_t *d, const uint8_t *d_recs, const uint64_t *d_off, uint32_t n, uint64_t total, void *stream,
                        const uint8_t **d_sorted, const uint64_t **d_keys, const uint64_t **d_soff, const uint32_t *d_side = nullptr, const uint32_t **d_side_sorted = nullptr);
// every run's keys (host) -> ord [n]: the records' global ordinals (run after run) in sorted order
int bsr_sort_keys_device(bsr_dev_t *d, const uint64_t *keys, uint64_t n, void *stream, uint32_t *ord);
// one window of the final file.  src (host, pinned or not) [src_bytes]: the records of the window as the runs hold them; src_off / size [n] (host): record j of the
// window in src.  The records are gathered into order, compressed (ws), indexed (ix: heads appended; lin and counts stay on the device until bsr_index_finish) and
// the members handed to the sink
// cov (or NULL): the run's coverage (csrc/bam_cov_kernels.hip, begun by the caller) takes the window behind the flag step; cov_ms (or NULL) += its device milliseconds
// stats (or NULL): the run's statistics (csrc/bam_stats_kernels.hip, begun by the caller) take the window beside it; stats_ms (or NULL) [2] += their milliseconds, the windows
// recal (or NULL): the run's recalibration table (csrc/bam_recal_kernels.hip, begun by the caller) takes it beside them; recal_ms as stats_ms
// requal (or NULL): the table applied to the window's qualities (csrc/bam_requal_kernels.hip, begun by the caller) behind the flag step and in front of all of them, which read the qualities as written; requal_ms as stats_ms
// dup, tord [n] (host), flag_ms (or NULL, all three): the decided duplicates (bdp_decide_device) and every record's global template ordinal -- the flags are set between the gather and the compressor
int bsr_window_device(bsr_dev_t *d, bmh_bam_ws_t *ws, const uint8_t *src, uint64_t src_bytes, const uint64_t *src_off, const uint32_t *size, uint32_t n, int level,
                      void *stream, bsr_index_t &ix, bsr_sink_t sink, void *user, struct bdp_dev_t *dup, const uint32_t *tord, double *flag_ms,
                      struct bcv_dev_t *cov = nullptr, double *cov_ms = nullptr, struct bst_dev_t *stats = nullptr, double *stats_ms = nullptr,
                      struct brc_dev_t *recal = nullptr, double *recal_ms = nullptr, struct brq_dev_t *requal = nullptr, double *requal_ms = nullptr);
// every run of the store -> the record members of the sorted file (to the sink, in windows of J.window records; 0: about 64 MiB of records) and its index J.ix
// J.markdup: mark the duplicates among the store's templates first, as J.P says (csrc/bam_dup_kernels.hip: the store keeps the locations and the barcode words
// J.P's optical step and barcodes ask for), and flag every window's records; the counts of bam_dup.h go to J.dup_counts
// cov, stats (or NULL): every window goes through the run's coverage and statistics (begun before, finished behind: bsr_write_device's)
// J.timed: J.dup_ms [0 .. 1] += the decision's milliseconds (host clock around bdp_decide_device) and the windows' flag steps' (events around the upload of the
// ordinals and the flag kernel), J.opt_ms += the optical step's, J.cov_ms and J.stats_ms += the windows'
int bsr_merge_device(bsr_dev_t *d, bmh_bam_ws_t *ws, const bsr_store_t &S, bsr_out_t &J, void *stream, bsr_sink_t sink, void *user, struct bcv_dev_t *cov, struct bst_dev_t *stats, struct brc_dev_t *recal = nullptr, struct brq_dev_t *requal = nullptr);
// the device form of a sorted output's run, whole: the coverage and the statistics begun (their device state lives here), the store's runs merged to the sink,
// both finished into J.CR / J.SR, the marking's counts complete (the templates without a barcode, every library's line counts as the batches counted them)
int bsr_write_device(bsr_dev_t *d, bmh_bam_ws_t *ws, const bsr_store_t &S, bsr_out_t &J, void *stream, bsr_sink_t sink, void *user, const char *fn);
int bsr_index_begin(bsr_dev_t *d, const bsr_index_t &ix, void *stream);
int bsr_index_finish(bsr_dev_t *d, bsr_index_t &ix, void *stream);
