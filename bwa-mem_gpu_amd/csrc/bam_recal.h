// The covariate table of base quality score recalibration, internal: the checked run, the result, the host form -- inline here, so that the sorted
// output's host sources (csrc/bam_sort_host.cpp) need no other object for it --, the mask's parser (csrc/bam_recal_host.cpp) and what csrc/bam_recal_kernels.hip offers
// csrc/bam_sort_kernels.hip.  Both forms take the sorted file's windows of records one after the other; nothing but the
// accumulator and the number of records seen passes from one window to the next.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#ifndef BRC_STANDALONE
#include "bmh_internal.h"
#else                                                              // tests/bam_recal_core_host.cpp: the host form and the mask parser alone, without the library
enum { BMH_OK = 0, BMH_EINVAL = -2, BMH_ENOMEM = -4 };
void bmh_set_error(const char *fmt, ...);
#endif
#include "bam_recal_core.h"
#include "bam_requal.h"                                            // the step that follows: its counts are exported into the same record

// what a run is made under, checked: the layout (P), the host's copies of the contigs' places and of the group IDs, and the caller's reference and mask
struct brc_run_t {
	brc_plan_t P;
	std::vector<uint64_t> coff; std::vector<int32_t> clen;
	std::string rg; std::vector<uint32_t> rg_off;
	const uint8_t *pac = nullptr; uint64_t l_pac = 0; const uint64_t *mask = nullptr; uint64_t masked = 0;
	brc_ref_t host_ref() const { return brc_ref_t{pac, mask, coff.data(), clen.data(), rg.data(), rg_off.data()}; }
};
// the options as the entry points take them (min_qual, max_cycle, pac, l_pac, contig_offset, mask, mask_words, n_groups, rg_ids) over these contigs.  need_pac: a
// host pac is required (the aligner's runs bring the index's).  Refused (BMH_EINVAL, a message): min_qual outside 0 .. 93, max_cycle outside 1 .. 65535, more
// than 255 groups, an empty or repeated ID, contigs that do not lie inside l_pac, a mask of another size, an accumulator beyond 2^28 words
inline int brc_run_make(brc_run_t &U, int32_t min_qual, int32_t max_cycle, const uint8_t *pac, uint64_t l_pac, const uint64_t *contig_offset, const uint64_t *mask, uint64_t mask_words,
                 int32_t n_groups, const char *const *rg_ids, int n_contigs, const int32_t *contig_len, bool need_pac, const char *fn)
{
	if (min_qual < 0 || min_qual >= (int32_t)BRC_NQ) { bmh_set_error("%s: recal_min_qual %d (0 .. %d)", fn, min_qual, (int)BRC_NQ - 1); return BMH_EINVAL; }
	if (max_cycle < 1 || max_cycle > (int32_t)BRC_CYCLE_LIMIT) { bmh_set_error("%s: recal_max_cycle %d (1 .. %d)", fn, max_cycle, (int)BRC_CYCLE_LIMIT); return BMH_EINVAL; }
	if (n_contigs < 0 || (n_contigs && !contig_len)) { bmh_set_error("%s: the recalibration table needs the contigs' lengths", fn); return BMH_EINVAL; }
	if (n_groups < 0 || n_groups > (int32_t)BRC_MAX_GROUPS) { bmh_set_error("%s: %d read groups: the recalibration table holds at most %d", fn, n_groups, (int)BRC_MAX_GROUPS); return BMH_EINVAL; }
	if (n_groups && !rg_ids) { bmh_set_error("%s: null argument (the read groups' IDs)", fn); return BMH_EINVAL; }
	if (need_pac && !pac && l_pac) { bmh_set_error("%s: the recalibration table needs the reference (pac, l_pac)", fn); return BMH_EINVAL; }
	U.P.n_contigs = n_contigs; U.P.has_groups = n_groups > 0; U.P.n_groups = n_groups ? n_groups : 1; U.P.min_qual = min_qual; U.P.max_cycle = max_cycle;
	if (U.P.words() > BRC_MAX_WORDS) {
		bmh_set_error("%s: %d read groups at recal_max_cycle %d ask for a table of %llu words (at most 2^28): lower recal_max_cycle", fn, U.P.n_groups, max_cycle, (unsigned long long)U.P.words());
		return BMH_EINVAL;
	}
	U.coff.assign((size_t)n_contigs + 1, 0); U.clen.assign((size_t)n_contigs + 1, 0);
	uint64_t at = 0;
	for (int c = 0; c < n_contigs; ++c) {
		if (contig_len[c] < 0) { bmh_set_error("%s: contig %d has a negative length", fn, c); return BMH_EINVAL; }
		const uint64_t o = contig_offset ? contig_offset[c] : at;
		if (o > l_pac || (uint64_t)contig_len[c] > l_pac - o) { bmh_set_error("%s: contig %d (%llu bases from %llu) lies outside the reference's %llu bases", fn, c, (unsigned long long)contig_len[c], (unsigned long long)o, (unsigned long long)l_pac); return BMH_EINVAL; }
		U.coff[(size_t)c] = o; U.clen[(size_t)c] = contig_len[c]; at = o + (uint64_t)contig_len[c];
	}
	U.rg.clear(); U.rg_off.assign(1, 0);
	for (int g = 0; g < n_groups; ++g) {
		if (!rg_ids[g] || !rg_ids[g][0]) { bmh_set_error("%s: read group %d has no ID", fn, g); return BMH_EINVAL; }
		for (int h = 0; h < g; ++h) if (!strcmp(rg_ids[h], rg_ids[g])) { bmh_set_error("%s: read group ID %s twice", fn, rg_ids[g]); return BMH_EINVAL; }
		U.rg.append(rg_ids[g]); U.rg.push_back('\0'); U.rg_off.push_back((uint32_t)U.rg.size());
	}
	if (!n_groups) { U.rg.assign(1, '\0'); U.rg_off.push_back(1); }
	if (mask && mask_words != (l_pac + 63) / 64) { bmh_set_error("%s: a mask of %llu words for %llu bases ((l_pac + 63) / 64 words)", fn, (unsigned long long)mask_words, (unsigned long long)l_pac); return BMH_EINVAL; }
	U.pac = pac; U.l_pac = l_pac; U.mask = mask; U.masked = 0;
	if (mask) for (uint64_t k = 0; k < mask_words; ++k) U.masked += (uint64_t)__builtin_popcountll(mask[k]);
	return BMH_OK;
}

// the results: the accumulator's words
struct brc_result_t { std::vector<uint64_t> w; };

// the message of the record with index `rec` that brc_prep refuses with `code`
inline int brc_refused(uint64_t rec, int code, const char *fn)
{
	const unsigned long long i = (unsigned long long)rec;
	switch (code) {
	case BRC_E_SUM: bmh_set_error("%s: record %llu has operations whose M I S = X lengths do not sum to its l_seq: the recalibration table walks them base by base", fn, i); break;
	case BRC_E_PLACEHOLDER: bmh_set_error("%s: record %llu holds the long-CIGAR placeholder (its operations are in its CG tag): the recalibration table reads the record's own operations", fn, i); break;
	case BRC_E_SPAN: bmh_set_error("%s: record %llu begins or ends outside its contig: the recalibration table compares it with the reference", fn, i); break;
	case BRC_E_TAGS: bmh_set_error("%s: record %llu has tags that cannot be walked to the record's end: the recalibration table reads RG and CG from them", fn, i); break;
	case BRC_E_RG_NONE: bmh_set_error("%s: record %llu has no RG tag: the recalibration table is kept per read group", fn, i); break;
	case BRC_E_RG_TYPE: bmh_set_error("%s: record %llu has an RG tag of another type than Z", fn, i); break;
	case BRC_E_RG_ID: bmh_set_error("%s: record %llu names a read group the table does not hold", fn, i); break;
	default: bmh_set_error("%s: record %llu is not whole: its bytes do not hold the fields, the name, the operations, the bases and the qualities it announces", fn, i); break;
	}
	return BMH_EINVAL;
}

// the host form
struct brc_host_t {
	const brc_run_t *U = nullptr; brc_result_t R; uint64_t n_seen = 0;
	void begin(const brc_run_t &run);
	// a window's n records recs + soff[j], in any order; the first record refused ends the run
	int window(const uint8_t *recs, const uint64_t *soff, uint32_t n, const char *fn);
	void finish() { R.w[BRC_MASKED] = U->masked; }
};

// (inline, like everything of the host form that csrc/bam_sort_host.cpp calls: the sorted output's host sources link without csrc/bam_recal_host.cpp)
inline void brc_host_t::begin(const brc_run_t &run) { U = &run; R.w.assign((size_t)run.P.words(), 0); n_seen = 0; }

inline int brc_host_t::window(const uint8_t *recs, const uint64_t *soff, uint32_t n, const char *fn)
{
	const brc_plan_t &P = U->P; const brc_ref_t F = U->host_ref();
	uint64_t *w = R.w.data();
	for (uint32_t j = 0; j < n; ++j, ++n_seen) {
		brc_rec_t r;
		const uint8_t *rec = recs + soff[j];
		const int st = brc_prep(rec, soff[j + 1] - soff[j], P, F, r);
		++w[BRC_SEEN];
		if (st >= BRC_FILTERED) { ++w[BRC_F_REF + (st - BRC_FILTERED)]; continue; }
		if (st != BRC_OK) return brc_refused(n_seen, st, fn);
		++w[BRC_COUNTED]; w[BRC_KEPT] += r.n;
		brc_cur_t C; brc_cur_begin(C);
		for (uint64_t i = r.s0; i < (uint64_t)r.s0 + r.n; ++i) {
			brc_obs_t o;
			brc_cur_seek(rec, r, i, C);
			const int sk = brc_base(rec, r, P, F, i, C, o);
			if (sk) { ++w[BRC_SK_BASE + sk - 1]; continue; }
			if (o.capped) ++w[BRC_CAPPED];
			uint64_t *a = w + P.at_cy_m(r.group, o.q, o.ci); ++a[0]; a[1] += o.snp;
			a = w + P.at_cy_id(r.group, o.ci); ++a[0]; a[1] += o.ins; a[2] += o.del;
			a = w + P.at_cx_m(r.group, o.q, o.mctx); ++a[0]; a[1] += o.snp;
			a = w + P.at_cx_id(r.group, o.ictx); ++a[0]; a[1] += o.ins; a[2] += o.del;
		}
	}
	return BMH_OK;
}

// the mask's parser: a text in pieces (feed), its last line (finish).  Lines are counted from 1; the format is taken from the first line that is not empty
struct brc_contig_t { std::string name; uint64_t off; int64_t len; };
struct brc_mask_parser_t {
	std::string file; const std::vector<brc_contig_t> *contigs = nullptr; uint64_t *mask = nullptr;
	std::string carry; uint64_t line_no = 0; int format = -1;      // -1: not known yet, 0: BED, 1: VCF
	int feed(const char *text, size_t n);
	int finish();
	int line(const char *s, size_t n);
};

#ifndef BRC_STANDALONE
// bmh_recal_t as it was before the apply step's members: a record is read and written beyond these bytes only where the caller has set the options' `apply`, or the
// record says itself (summary [15] = BRC_WIDE, set by the export) that it holds them
enum { BRC_WIDE = 1 };
#define BRC_RECAL_OLD_BYTES offsetof(bmh_recal_t, apply_summary)
// every array released, the record zeroed (bmh_recal_free, and a failed call's cleanup)
inline void brc_release(bmh_recal_t *r)
{
	if (!r) return;
	const bool wide = r->summary[BRC_N_SUM - 1] == (uint64_t)BRC_WIDE;
	free(r->cycle_m); free(r->cycle_id); free(r->context_m); free(r->context_id);
	if (wide) free(r->qual_hist);
	memset(r, 0, wide ? sizeof *r : BRC_RECAL_OLD_BYTES);
}
inline int brc_run_from_opt(brc_run_t &U, const bmh_recal_opt_t *o, int n_contigs, const int32_t *contig_len, bool need_pac, const char *fn)
{
	bmh_recal_opt_t d;
	if (!o) { memset(&d, 0, sizeof d); d.min_qual = BRC_MIN_QUAL; d.max_cycle = BRC_MAX_CYCLE; o = &d; }
	return brc_run_make(U, o->min_qual, o->max_cycle, o->pac, o->l_pac, o->contig_offset, o->mask, o->mask_words, o->n_groups, o->rg_ids, n_contigs, contig_len, need_pac, fn);
}
// R as the entry points return it (malloc'd arrays; *out zeroed first).  U and R NULL: no table was counted.  A (or NULL): the apply step's counts, with its
// milliseconds and windows timed -- the only case in which the record's bytes beyond BRC_RECAL_OLD_BYTES are written
inline int brc_export(const brc_run_t *U, const brc_result_t *R, bmh_recal_t *out, const char *fn, const brq_result_t *A = nullptr, const double *apply_ms = nullptr)
{
	memset(out, 0, A ? sizeof *out : BRC_RECAL_OLD_BYTES);
	out->n_qual = BRC_NQ;
	bool ok = true;
	if (U && R) {
		const brc_plan_t &P = U->P;
		const uint64_t *w = R->w.data();
		auto dup = [w](uint64_t at, uint64_t n) { uint64_t *p = (uint64_t *)malloc(8 * (size_t)n + 8); if (p && n) memcpy(p, w + at, 8 * (size_t)n); return p; };
		out->n_groups = P.n_groups; out->min_qual = P.min_qual; out->max_cycle = P.max_cycle;
		out->cycle_m = dup(P.w_cy_m(), P.w_cy_id() - P.w_cy_m()); out->cycle_id = dup(P.w_cy_id(), P.w_cx_m() - P.w_cy_id());
		out->context_m = dup(P.w_cx_m(), P.w_cx_id() - P.w_cx_m()); out->context_id = dup(P.w_cx_id(), P.words() - P.w_cx_id());
		ok = out->cycle_m && out->cycle_id && out->context_m && out->context_id;
		for (int k = 0; k < BRC_N_SUM; ++k) out->summary[k] = w[k];
	}
	if (A) {
		out->summary[BRC_N_SUM - 1] = BRC_WIDE;
		for (int k = 0; k < BRQ_N_SUM; ++k) out->apply_summary[k] = A->w[(size_t)k];
		out->qual_hist = (uint64_t *)malloc(8 * (size_t)BRQ_HIST);
		if (out->qual_hist) memcpy(out->qual_hist, A->w.data() + BRQ_N_SUM, 8 * (size_t)BRQ_HIST); else ok = false;
		if (apply_ms) { out->apply_ms = apply_ms[0]; out->apply_windows = (uint64_t)apply_ms[1]; }
	}
	if (!ok) {
		brc_release(out);
		bmh_set_error("%s: out of memory", fn); return BMH_ENOMEM;
	}
	return BMH_OK;
}

// csrc/bam_recal_kernels.hip
struct brc_dev_t;                                                  // the device form's accumulator, reference and state; one per sorted run
brc_dev_t *brc_dev_create(void);
void brc_dev_free(brc_dev_t *d);
// the accumulator cleared, the contigs, the groups, the mask and -- d_pac NULL -- U's pac uploaded.  d_pac: a pac body already on the device (the aligner's index)
int brc_begin_device(brc_dev_t *d, const brc_run_t &U, const uint8_t *d_pac, void *stream);
// a window's records d_recs at d_soff [n + 1] (device): one kernel, and the refusal word on its way to the host.  With ms (or NULL) events are recorded around the
// kernel.  Nothing waits here: brc_window_ms, once the caller has waited for the stream, refuses the window by its first refused record (fn names the caller) and,
// with ms, ms[0] += the kernel's milliseconds, ms[1] += 1 (the windows timed)
int brc_window_device(brc_dev_t *d, const uint8_t *d_recs, const uint64_t *d_soff, uint32_t n, void *stream, double *ms);
int brc_window_ms(brc_dev_t *d, double *ms, const char *fn);
// the results: the run's one read of the accumulator
int brc_finish_device(brc_dev_t *d, void *stream, brc_result_t &R, const char *fn);
#endif
