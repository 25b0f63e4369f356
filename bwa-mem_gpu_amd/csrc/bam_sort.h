// Sorted BAM output, internal: the index being built over a file's windows, the run store, and what csrc/bam_sort_kernels.hip offers csrc/align_pipeline.hip.
#pragma once
#include <stdint.h>
#include <string>
#include <vector>
#include "bmh_internal.h"
#include "bam_sort_core.h"
#include "bam_dup.h"
#include "bam_tpl.h"

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
	bool valid = false;                                            // the index of a whole file (init: of one without records); false while a run builds it and after it failed
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
// opt and res as the sorted-file entry points take them -> o: opt or its defaults, the index format checked; with o.markdup the plan P (bdp_plan_make; an optical
// distance is refused: a stand-alone file has no optical step), its counts going to *res
int bsr_file_opt_check(const bmh_sorted_file_opt_t *opt, bmh_markdup_counts_t *res, const char *fn, bmh_sorted_file_opt_t &o, bdp_plan_t &P);

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

// csrc/bam_sort_kernels.hip
struct bsr_dev_t;                                                  // device buffers of the sort, the gather and the index pass; kept between calls
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
// dup, tord [n] (host), flag_ms (or NULL, all three): the decided duplicates (bdp_decide_device) and every record's global template ordinal -- the flags are set between the gather and the compressor
int bsr_window_device(bsr_dev_t *d, bmh_bam_ws_t *ws, const uint8_t *src, uint64_t src_bytes, const uint64_t *src_off, const uint32_t *size, uint32_t n, int level,
                      void *stream, bsr_index_t &ix, bsr_sink_t sink, void *user, struct bdp_dev_t *dup, const uint32_t *tord, double *flag_ms,
                      struct bcv_dev_t *cov = nullptr, double *cov_ms = nullptr, struct bst_dev_t *stats = nullptr, double *stats_ms = nullptr);
// every run of the store -> the record members of the sorted file (to the sink, in windows of `window` records; 0: about 64 MiB of records) and its index
// dup_counts (or NULL) [8]: mark the duplicates among the store's templates first, as P says (csrc/bam_dup_kernels.hip: the store keeps the locations and the barcode
// words P's optical step and barcodes ask for), and flag every window's records; the counts of bam_dup.h
// cov, cov_ms (or NULL): every window goes through the run's coverage (bcv_begin_device before, bcv_finish_device behind: the caller's)
// stats, stats_ms (or NULL): every window goes through the run's statistics (bst_begin_device before, bst_finish_device behind: the caller's)
// dup_ms (or NULL) [2]: += the decision's milliseconds (host clock around bdp_decide_device) and the windows' flag steps' (events around the upload of the ordinals
// and the flag kernel); opt_ms (or NULL) += the optical step's milliseconds
int bsr_merge_device(bsr_dev_t *d, bmh_bam_ws_t *ws, const bsr_store_t &S, uint32_t window, int level, void *stream, bsr_index_t &ix, bsr_sink_t sink, void *user,
                     uint64_t *dup_counts, const bdp_plan_t &P, double *dup_ms = nullptr, double *opt_ms = nullptr, struct bcv_dev_t *cov = nullptr, double *cov_ms = nullptr,
                     struct bst_dev_t *stats = nullptr, double *stats_ms = nullptr);
int bsr_index_begin(bsr_dev_t *d, const bsr_index_t &ix, void *stream);
int bsr_index_finish(bsr_dev_t *d, bsr_index_t &ix, void *stream);
