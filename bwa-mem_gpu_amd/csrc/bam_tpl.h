// Whole-file templates by name, internal (BDP_TPL_FILE; csrc/bam_tpl_core.h has the rules): the parts of a file's records, what the grouping
// makes of them, and what csrc/bam_tpl_host.cpp and csrc/bam_tpl_kernels.hip offer the drivers of csrc/bam_post.cpp and csrc/bam_post_kernels.hip.
#pragma once
#include <stdint.h>
#include <vector>
#include "bam_dup.h"
#include "bam_tpl_core.h"

// every record's part in file order; locs / bcs beside them only when the run counts optical duplicates / compares barcodes (else empty).  Host memory: 32 bytes
// per record, 16 and 8 more with the options
struct btp_parts_t {
	std::vector<btp_part_t> parts; std::vector<bdp_loc_t> locs; std::vector<uint64_t> bcs;
	void clear() { parts.clear(); locs.clear(); bcs.clear(); }
};

// what the grouping gives: every record's template ordinal, the templates' entries in ordinal order (locs, bcs with the options), the secondary or supplementary
// and the unmapped records and -- with read groups -- those two and the templates per library (lib3 [3 * n_lib]); word: the smallest refusal (BPO_NONE: none;
// nothing else is then meaningful)
struct btp_result_t {
	std::vector<uint32_t> rec_tpl; std::vector<bdp_entry_t> E; std::vector<bdp_loc_t> locs; std::vector<uint64_t> bcs; std::vector<uint64_t> lib3;
	uint64_t info[2] = {0, 0}, word = BPO_NONE;
};

// csrc/bam_tpl_host.cpp
// a record's part appended to S as P says (its groups, its barcode source, locations with its optical step)
void btp_append_host(btp_parts_t &S, const uint8_t *rec, uint64_t sz, const bdp_plan_t &P, uint32_t hash_bits);
// the grouping on the host: std::stable_sort by (h1, h0), the fold of every set
int btp_group_host(const btp_parts_t &S, const bdp_plan_t &P, btp_result_t &R, const char *fn);
// the message of the refusal `word` of a file with parts S; sam_line0: the number of the SAM line that holds record 0 (0: the input is a BAM)
int btp_refused(const btp_parts_t &S, uint64_t word, const bdp_plan_t &P, uint64_t sam_line0, const char *fn);

// the step on its own, what its two forms share: the arguments checked, the plan (locations always, the rest as opt says), the stream walked and every record
// passed through bpo_check -> off [n + 1]; and the result's arrays (malloc'd)
int btp_templates_begin(const uint8_t *recs, uint64_t n_bytes, const bmh_markdup_opt_t *opt, int32_t hash_bits, bmh_bam_templates_t *out, const char *fn, bdp_plan_t &P, std::vector<uint64_t> &off);
int btp_templates_export(const btp_result_t &R, const bdp_plan_t &P, bmh_bam_templates_t *out, const char *fn);

// csrc/bam_tpl_kernels.hip
struct btp_dev_t;                                                 // device buffers of the parts kernel and the grouping; kept between calls
btp_dev_t *btp_dev_create(void);
void btp_dev_free(btp_dev_t *d);
// the run's read groups go to the device (T NULL or empty: none)
int btp_dev_set_groups(btp_dev_t *d, const bdp_table_t *T, void *stream);
// a batch's records d_recs with offsets d_off [n + 1] (device; bpo_check_fix has passed them) -> their parts appended to S (host), and *d_iota [n]: 0 .. n - 1, the
// side word of the batch sort, in d until its next call
int btp_parts_device(btp_dev_t *d, const uint8_t *d_recs, const uint64_t *d_off, uint32_t n, uint64_t total, const bdp_plan_t &P, uint32_t hash_bits, void *stream, btp_parts_t &S,
                     const uint32_t **d_iota);
// the grouping on the device; its buffers are freed before it returns (the decision allocates next).  BMH_ENOMEM with the need named when the device has no room
int btp_group_device(btp_dev_t *d, const btp_parts_t &S, const bdp_plan_t &P, void *stream, btp_result_t &R, const char *fn);
