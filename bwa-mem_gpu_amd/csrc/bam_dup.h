// Duplicate marking, internal: the host forms (csrc/bam_dup_host.cpp) and what csrc/bam_dup_kernels.hip offers csrc/bam_sort_kernels.hip and csrc/align_pipeline.hip.
#pragma once
#include <stdint.h>
#include <string>
#include <vector>
#ifndef BDP_STANDALONE
#include "bmh_internal.h"
#else                                                              // tests/bam_dup_core_host.cpp: the host forms alone, without the library
enum { BMH_OK = 0, BMH_EINVAL = -2, BMH_ENOMEM = -4 };
void bmh_set_error(const char *fmt, ...);
#endif
#include "bam_dup_core.h"

// counts of a run: [0] pairs examined [1] fragments examined [2] duplicate pairs [3] duplicate fragments [4] records flagged [5] secondary or supplementary
// records [6] unmapped records [7] templates
enum { BDP_PAIRS = 0, BDP_FRAGS, BDP_DUP_PAIRS, BDP_DUP_FRAGS, BDP_FLAGGED, BDP_SECSUP, BDP_UNMAPPED, BDP_TEMPLATES, BDP_N_COUNTS };

// csrc/bam_dup_host.cpp
struct bdp_plan_t;
// a run's read groups as the entry points take them (ids [n], lib [n]: every group's library index) -> the table of csrc/bam_dup_core.h; n_lib: 1 + the largest
// index.  Refused (BMH_EINVAL, the row named): no rows, an empty ID, two rows with one ID, a library index outside 0 .. BDP_MAX_LIBS - 1
struct bdp_table_t {
	std::string ids; std::vector<uint32_t> id_off; std::vector<uint8_t> lib; uint32_t n_lib = 0;
	bool empty() const { return lib.empty(); }
	bdp_groups_t view() const { return {ids.data(), id_off.data(), lib.data(), (uint32_t)lib.size()}; }
};
int bdp_table_make(bdp_table_t &T, const char *const *ids, const int32_t *lib, int n, const char *fn);
// with a table every record's refID stays below BDP_MAX_REF (the library takes the end words' top byte): the first that does not is refused by its index
int bdp_refs_fit(const uint8_t *recs, const uint64_t *off, uint32_t n, const char *fn);
// the message of a template bdp_entry_lib refuses (st: BDP_E_NO_RG or BDP_E_RG_UNKNOWN) that begins at record `rec`
int bdp_group_refused(uint32_t rec, int st, const char *fn);
// records in the writer's order with offsets off [n + 1] -> tpl [n]: every record's template ordinal in the stream; entries: one per template; info [2] += the
// secondary or supplementary and the unmapped records.  Not BMH_OK (message set): the first record begins no template, or a paired template lacks a primary line
// with P's read groups the entries carry their templates' libraries; a first record without RG:Z, or with an ID the table does not hold, is refused too
// locs (or NULL): every template's location (csrc/bam_dup_core.h) beside its entry -- what the optical step reads
// bcs (or NULL): with P's barcodes every template's barcode word beside its entry; a first record whose barcode tag is of another type than Z, or whose tags cannot
// be walked, is refused by its index
// tpl_rule: BDP_TPL_WRITER, or BDP_TPL_NAME -- a template is a run of adjacent records under one name (csrc/bam_post_core.h); the first record always heads one
int bdp_entries_host(const uint8_t *recs, const uint64_t *off, uint32_t n, std::vector<uint32_t> &tpl, std::vector<bdp_entry_t> &entries, uint64_t info[2], const char *fn,
                     const bdp_plan_t &P, std::vector<bdp_loc_t> *locs = nullptr, std::vector<uint64_t> *bcs = nullptr, int tpl_rule = BDP_TPL_WRITER, uint64_t rec_base = 0);
// under BDP_TPL_NAME the stream is a batch of a file: rec_base is the file index of its first record, which the messages name; a refused template is worded by
// bdp_name_refused (rec: the file index of its first record)
int bdp_name_refused(uint64_t rec, const char *fn);
// barcode_mode and tag as the entry points take them -> *bc; BMH_EINVAL with a message: a mode other than 0, 1, 2; a tag that is not [A-Za-z][A-Za-z0-9], RG, or one
// the writer produces itself (NM MD AS XS SA XA pa)
int bdp_barcode_check(int barcode_mode, const char *tag, const char *fn, bdp_bc_t *bc);
// the message of a template whose first record `rec` bdp_barcode refuses (st: BDP_E_BC_TYPE, BDP_E_BC_WALK or BDP_E_BC_PACK)
int bdp_barcode_refused(uint32_t rec, int st, const char *fn);
// the templates without a barcode among B [T]
uint64_t bdp_no_barcode(const uint64_t *B, uint64_t T);
// grouping barcodes by edits (csrc/bam_dup_core.h): the mismatches that still join (0 .. BDP_BC_MAX_EDITS), the most distinct words of a key that are clustered,
// and where the three counts go (BDP_GRP_*): out [3], lib_out [3 * n_lib] or NULL.  The barcode words of such a run are packed (bdp_bc_t.pack)
struct bdp_group_t { uint32_t edits, max_set; uint64_t *out, *lib_out; };
// edits and max_set as the entry points take them (edits -1: no grouping; max_set 0: BDP_BC_MAX_SET) -> BMH_EINVAL with a message (edits outside 0 .. 21, edits
// without a barcode source, a max_set of 2^31 and more), or BMH_OK and bc->pack set when edits >= 0
int bdp_group_check(int edits, uint64_t max_set, const char *fn, bdp_bc_t *bc);
// the canonical words of one pass, single-threaded through the clustering core (its invariant asserted).  frag false: the pair pass -- words [T], a barcoded pair's
// the smallest word of its component, every other template's its own; the three counts go to G.out / G.lib_out (zeroed first).  frag true: the fragment pass --
// words [2 T] by item id (template << 1 | end); only the keys over the cap are counted (added)
void bdp_group_host(const bdp_entry_t *E, uint64_t T, const uint64_t *B, const bdp_group_t &G, uint32_t n_lib, bool frag, std::vector<uint64_t> &words);
// the optical step of a run: the distance (0 .. 2^31 - 1), the largest set examined, and where its three counts go (BDP_OPT_*): out [3], lib_out [3 * n_lib] or NULL
struct bdp_optical_t { int64_t distance; uint32_t max_set; uint64_t *out, *lib_out; };
// distance and max_set as the entry points take them (max_set 0: BDP_OPT_MAX_SET) -> BMH_EINVAL with a message, or BMH_OK
int bdp_optical_check(int64_t distance, uint64_t max_set, const char *fn);
// What a marking run is made under, checked and normal: the read groups (an empty table: none), the barcode source, the optical step (a distance of -1: none) and the
// grouping by edits (read with bc.pack only, so never without a source); the caps hold their defaults.  Where the counts beyond a run's eight go: lib_counts
// [BDP_N_COUNTS * n_lib] and the steps' lib_out (or NULL; read with groups only), *no_barcode (or NULL).  A plan made by default marks plainly
struct bdp_plan_t {
	bdp_table_t table; bdp_bc_t bc = {BDP_BC_OFF, 0, 0};
	bdp_optical_t opt = {-1, (uint32_t)BDP_OPT_MAX_SET, nullptr, nullptr}; bdp_group_t grp = {0, (uint32_t)BDP_BC_MAX_SET, nullptr, nullptr};
	uint64_t *lib_counts = nullptr, *no_barcode = nullptr;
	const bdp_table_t *groups() const { return table.empty() ? nullptr : &table; }
	const bdp_optical_t *optical() const { return opt.distance >= 0 ? &opt : nullptr; }
	const bdp_bc_t *barcode() const { return bc.mode != BDP_BC_OFF ? &bc : nullptr; }
	const bdp_group_t *grouping() const { return barcode() && bc.pack ? &grp : nullptr; }
	uint32_t n_lib() const { return table.empty() ? 0 : table.n_lib; }
};
#ifndef BDP_STANDALONE
// the options and the counts record as the entry points take them (opt NULL: plain marking) -> the plan, its counts going to *res (zeroed).  The one place the
// arguments are checked, in this order: the barcode source, the edits and their cap, the optical step, the read groups, the groups an optical step can hold
int bdp_plan_make(bdp_plan_t &P, const bmh_markdup_opt_t *opt, bmh_markdup_counts_t *res, const char *fn);
// the plan of the two probes (bdp_probe_t): read groups as the locations carry their rows (barcode_mode 0), or a barcode source with plain or packed words
int bdp_probe_plan(bdp_plan_t &P, const char *const *rg_ids, const int32_t *rg_lib, int n_groups, int barcode_mode, const char tag[2], int packed, const char *fn);
#endif
// the optical duplicates among the pairs of E [T] with locations L [T], single-threaded through the clustering core of csrc/bam_dup_core.h (its invariant asserted);
// n_lib 0: no libraries, lib_out unused
// B [T] (or NULL): the barcode words -- a set is the pairs of one (lo, hi, word); with grouping the pair pass's canonical words
void bdp_optical_host(const bdp_entry_t *E, const bdp_loc_t *L, uint64_t T, const bdp_optical_t &O, uint32_t n_lib, const uint64_t *B = nullptr);
// the decision: bits [(T + 31) / 32]: bit t set when template t is a duplicate; counts [0 .. 4]; P.lib_counts (with read groups): every library's own counts, of
// which the decision fills (and zeroes the rest of) words 0 .. 4
// B [T] (or NULL): the barcode words, part of the pairs' and the fragments' keys; with P's grouping they are grouped by edits first
// pair_words (or NULL): the pair pass's canonical words, for the optical step
void bdp_decide_host(const bdp_entry_t *entries, uint64_t T, std::vector<uint32_t> &bits, uint64_t counts[5], const bdp_plan_t &P, const uint64_t *B = nullptr,
                     std::vector<uint64_t> *pair_words = nullptr);
// words 5 .. 7 of every library's counts += the secondary or supplementary records, the unmapped records and the templates of the stream (off [n + 1], tpl [n]: the
// records' template ordinals, E [T]: entries made with read groups)
void bdp_lib_tally_host(const uint8_t *recs, const uint64_t *off, uint32_t n, const uint32_t *tpl, const bdp_entry_t *E, uint64_t T, uint32_t n_lib, uint64_t *lib_counts);
// the whole of it on a walked stream, as P says: flags set in place
int bdp_markdup_host(uint8_t *recs, const std::vector<uint64_t> &off, uint64_t counts[BDP_N_COUNTS], const char *fn, const bdp_plan_t &P);
// the stand-alone calls beside marking: stop at the templates' locations, or at their barcode words -- *out takes them, counts [BDP_TEMPLATES] their number
enum bdp_probe_t { BDP_MARK = 0, BDP_PROBE_LOCS, BDP_PROBE_BCS };

// csrc/bam_dup_kernels.hip
struct bdp_dev_t;                                                  // device buffers of the batches' entries, the decision and the bitmap; kept between calls
bdp_dev_t *bdp_dev_create(void);
void bdp_dev_free(bdp_dev_t *d);
// a batch's records d_recs with offsets d_off [n + 1] (device, writer's order) -> *d_tpl [n], *d_entries [up to n], *d_info [4]: templates, the first bad record + 1
// (0: none; n + 1: the first record begins no template), secondary or supplementary records, unmapped records -- all in d until its next call
// With read groups (bdp_dev_set_groups) *d_info has BDP_INFO_WORDS words: [4], [5] the first template's first record + 1 without an RG:Z tag / with an ID the
// table does not hold (0xffffffff: none)
// With packed barcodes (bc->pack) *d_info has BDP_INFO_WORDS_PACK words: [8] the first template's first record + 1 whose barcode does not pack
enum { BDP_INFO_WORDS = 8, BDP_INFO_WORDS_PACK = 9 };
inline uint32_t bdp_info_words(const bdp_bc_t *bc) { return bc && bc->mode != BDP_BC_OFF && bc->pack ? BDP_INFO_WORDS_PACK : BDP_INFO_WORDS; }
// d_locs (or NULL): *d_locs [as many as entries]: every template's location, written by the lane that makes its entry
// bc, d_bcs (or NULL): barcodes are compared -- *d_bcs [as many as entries]: every template's barcode word, written by the lane that makes its entry; *d_info [6],
// [7]: the first template's first record + 1 whose barcode tag is of another type than Z / whose tags cannot be walked (0xffffffff: none)
// tpl_rule: BDP_TPL_WRITER, or BDP_TPL_NAME -- the heads come from a lane-per-record name compare against the predecessor; the scan and the entries are the same
int bdp_batch_device(bdp_dev_t *d, const uint8_t *d_recs, const uint64_t *d_off, uint32_t n, uint64_t total, void *stream, const uint32_t **d_tpl,
                     const bdp_entry_t **d_entries, const uint32_t **d_info, const bdp_loc_t **d_locs, const bdp_bc_t *bc, const uint64_t **d_bcs, int tpl_rule = BDP_TPL_WRITER);
// the heads of BDP_TPL_NAME for bdp_batch_device's scan (csrc/bam_post_kernels.hip): d_head [n], and d_info [2], [3] counted as the writer's rule counts them
int bpo_heads_device(const uint8_t *d_recs, const uint64_t *d_off, uint32_t n, uint64_t total, uint32_t *d_head, uint32_t *d_info, void *stream);
// a batch whose templates are of several libraries (a run that keeps its input's read groups), after bdp_batch_device on the same batch: *d_lib3 [3 * n_lib] -- every
// library's secondary / supplementary records, unmapped records and templates, a record counted under the library of its template's entry (bdp_lib_tally_host's
// three, per batch) -- in d until its next call.  n_lib <= BDP_MAX_LIBS.
int bdp_batch_lib_counts_device(bdp_dev_t *d, const uint8_t *d_recs, const uint64_t *d_off, uint32_t n, uint64_t total, uint32_t n_lib, void *stream, const uint32_t **d_lib3);
// the run's read groups go to the device (T NULL or empty: none, the entries are made without libraries); the batches that follow use them
int bdp_dev_set_groups(bdp_dev_t *d, const bdp_table_t *T, void *stream);
// the message of a batch whose info [1] is not 0
int bdp_batch_refused(uint32_t n, uint32_t bad, const char *fn);
// the verdict on a batch's info words (n records; groups, barcode: all BDP_INFO_WORDS were read): BMH_OK, or the message of the first refused record
// pack: BDP_INFO_WORDS_PACK were read
int bdp_batch_check(uint32_t n, const uint32_t *info, bool groups, const char *fn, bool barcode = false, bool pack = false);
// the same verdict without the message: BDP_E_OK, or the status of the first refused record and *bad = its index + 1 (n + 1: the first record begins no template)
int bdp_batch_verdict(uint32_t n, const uint32_t *info, bool groups, bool barcode, bool pack, uint32_t *bad);
// every template's entry (host) -> the bitmap, kept in d for bdp_flag_device, and counts [0 .. 4], as P says
// n_records: the records of the final sort that follows (csrc/bam_sort_kernels.hip: 24 bytes each and the sort's work space) -- the decision's buffers are freed
// before that sort allocates, so one check of the larger of the two needs refuses here what either would refuse
// P.lib_counts (with read groups): words 0 .. 4 of every library's counts, from the entries' library bytes and the bitmap (the other words zeroed)
// locs [T] (host; read with P's optical step): the optical step after the pair pass, on the pairs as that pass left them -- sets of equal keys next to each other.  opt_ms (or NULL)
// += its milliseconds (events around its kernels, the upload of the locations included)
// bcs [T] (host; or NULL: no barcodes are compared): the templates' barcode words -- one more stable radix pass on them in the pair pass and in the fragment pass, and the word compared where
// keys are: 8 bytes per template more on the device
// with P's grouping (and bcs, packed): the words are grouped by edits before the pair decision and before the fragment pass's run heads -- the passes then compare the canonical
// words: 56 bytes per template more on the device (16 the canonical words, 40 the clustering's heads, members and union-find)
int bdp_decide_device(bdp_dev_t *d, const bdp_entry_t *entries, const bdp_loc_t *locs, const uint64_t *bcs, uint64_t T, void *stream, uint64_t counts[5], const bdp_plan_t &P,
                      uint64_t n_records = 0, double *opt_ms = nullptr);
// records d_recs at d_off [n] (device; all inside `total` bytes) whose global template ordinals are tord [n] (host): byte 19 |= 0x04 where the bitmap says so
int bdp_flag_device(bdp_dev_t *d, uint8_t *d_recs, const uint64_t *d_off, const uint32_t *tord, uint32_t n, uint64_t total, void *stream);
