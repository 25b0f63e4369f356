// Applying a recalibration table to the base qualities, internal: the checked table and its int16 deltas, the host form -- inline here, as
// csrc/bam_recal.h's is, so that the sorted output's host sources need no other object for it -- and what csrc/bam_requal_kernels.hip offers
// csrc/bam_sort_kernels.hip.  Included by csrc/bam_recal.h behind the status codes and bmh_set_error.  Both forms take the sorted file's windows of records one
// after the other and rewrite them in place; nothing but the counts and the number of records seen passes from one window to the next.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>
#include "bam_requal_core.h"

// the table, checked, as the deltas both forms read
struct brq_run_t {
	brq_plan_t P;
	std::vector<int16_t> t;
	std::string rg; std::vector<uint32_t> rg_off;
	brq_tab_t host_tab() const { return brq_tab_t{t.data(), rg.data(), rg_off.data()}; }
};

inline double brq_emp(uint64_t o, uint64_t e)
{
	const double q = -10.0 * log10(((double)e + 1.0) / ((double)o + 2.0));
	return q < 93.0 ? q : 93.0;
}
inline int16_t brq_fixed(double v) { return (int16_t)rint(256.0 * v); }

// the counts of a table (cycle_m [groups][94][2 max_cycle][2], context_m [groups][94][17][2]; rg_ids NULL or the one ID `*`: every record belongs to the one group)
// -> U.  Refused (BMH_EINVAL, a message naming the row): min_qual outside 0 .. 93, max_cycle outside 1 .. 65535, groups outside 1 .. 255, an empty or repeated ID,
// errors above observations, a (group, quality) whose cycle rows and context rows do not sum to the same observations and errors
inline int brq_run_make(brq_run_t &U, int32_t n_groups, int32_t min_qual, int32_t max_cycle, int32_t n_qual, const uint64_t *cycle_m, const uint64_t *context_m, const char *const *rg_ids, const char *fn)
{
	if (min_qual < 0 || min_qual >= (int32_t)BRC_NQ) { bmh_set_error("%s: the table to apply has min_qual %d (0 .. %d)", fn, min_qual, (int)BRC_NQ - 1); return BMH_EINVAL; }
	if (max_cycle < 1 || max_cycle > (int32_t)BRC_CYCLE_LIMIT) { bmh_set_error("%s: the table to apply has max_cycle %d (1 .. %d)", fn, max_cycle, (int)BRC_CYCLE_LIMIT); return BMH_EINVAL; }
	if (n_groups < 1 || n_groups > (int32_t)BRC_MAX_GROUPS) { bmh_set_error("%s: the table to apply has %d read groups (1 .. %d)", fn, n_groups, (int)BRC_MAX_GROUPS); return BMH_EINVAL; }
	if (n_qual != (int32_t)BRC_NQ) { bmh_set_error("%s: the table to apply has %d qualities (%d)", fn, n_qual, (int)BRC_NQ); return BMH_EINVAL; }
	if (!cycle_m || !context_m) { bmh_set_error("%s: null argument (the table to apply needs cycle_m and context_m)", fn); return BMH_EINVAL; }
	const bool one = !rg_ids || (n_groups == 1 && rg_ids[0] && !strcmp(rg_ids[0], "*"));
	brq_plan_t &P = U.P;
	P.n_groups = n_groups; P.has_groups = !one; P.min_qual = min_qual; P.max_cycle = max_cycle;
	if (one && n_groups != 1) { bmh_set_error("%s: the table to apply has %d read groups and no IDs", fn, n_groups); return BMH_EINVAL; }
	U.rg.clear(); U.rg_off.assign(1, 0);
	for (int g = 0; g < n_groups; ++g) {
		const char *id = one ? "*" : rg_ids[g];
		if (!id || !id[0]) { bmh_set_error("%s: read group %d of the table to apply has no ID", fn, g); return BMH_EINVAL; }
		for (int h = 0; h < g; ++h) if (!strcmp(rg_ids[h], id)) { bmh_set_error("%s: read group ID %s twice in the table to apply", fn, id); return BMH_EINVAL; }
		U.rg.append(id); U.rg.push_back('\0'); U.rg_off.push_back((uint32_t)U.rg.size());
	}
	const uint32_t C = (uint32_t)max_cycle, ncy = 2 * C;
	auto id_of = [&U](int g) { return U.rg.c_str() + U.rg_off[(size_t)g]; };
	auto cycle_of = [C](uint32_t s) { return s >= C ? (int)(s - C + 1) : (int)s - (int)C; };
	U.t.assign((size_t)P.entries(), 0);
	std::vector<uint64_t> oq((size_t)BRC_NQ), eq((size_t)BRC_NQ);
	for (int g = 0; g < n_groups; ++g) {
		const uint64_t *cy = cycle_m + (uint64_t)g * BRC_NQ * ncy * 2, *cx = context_m + (uint64_t)g * BRC_NQ * BRC_MCTX * 2;
		uint64_t og = 0, eg = 0; double expected = 0;
		for (uint32_t q = 0; q < (uint32_t)BRC_NQ; ++q) {
			uint64_t o = 0, e = 0, ox = 0, ex = 0;
			for (uint32_t s = 0; s < ncy; ++s) {
				const uint64_t a = cy[((uint64_t)q * ncy + s) * 2], b = cy[((uint64_t)q * ncy + s) * 2 + 1];
				if (b > a) { bmh_set_error("%s: the table to apply holds %llu errors among %llu observations (group %s, quality %u, cycle %d)", fn, (unsigned long long)b, (unsigned long long)a, id_of(g), q, cycle_of(s)); return BMH_EINVAL; }
				o += a; e += b;
			}
			for (uint32_t x = 0; x < (uint32_t)BRC_MCTX; ++x) {
				const uint64_t a = cx[((uint64_t)q * BRC_MCTX + x) * 2], b = cx[((uint64_t)q * BRC_MCTX + x) * 2 + 1];
				if (b > a) { bmh_set_error("%s: the table to apply holds %llu errors among %llu observations (group %s, quality %u, context %u)", fn, (unsigned long long)b, (unsigned long long)a, id_of(g), q, x); return BMH_EINVAL; }
				ox += a; ex += b;
			}
			if (o != ox || e != ex) {
				bmh_set_error("%s: the table to apply counts %llu observations and %llu errors by cycle, %llu and %llu by context (group %s, quality %u)", fn, (unsigned long long)o, (unsigned long long)e,
				              (unsigned long long)ox, (unsigned long long)ex, id_of(g), q);
				return BMH_EINVAL;
			}
			oq[q] = o; eq[q] = e; og += o; eg += e;
			expected += (double)o * pow(10.0, -(double)q / 10.0);
		}
		const double dg = og ? brq_emp(og, eg) - -10.0 * log10(expected / (double)og) : 0.0;
		for (uint32_t q = 0; q < (uint32_t)BRC_NQ; ++q) {
			double B = oq[q] ? brq_emp(oq[q], eq[q]) : (double)q + dg;
			B = B < 1.0 ? 1.0 : B > 93.0 ? 93.0 : B;
			int16_t *r = U.t.data() + P.at((uint32_t)g, q);
			r[0] = brq_fixed(B);
			for (uint32_t s = 0; s < ncy; ++s) {
				const uint64_t a = cy[((uint64_t)q * ncy + s) * 2], b = cy[((uint64_t)q * ncy + s) * 2 + 1];
				r[1 + s] = a ? brq_fixed(brq_emp(a, b) - B) : 0;
			}
			for (uint32_t x = 0; x < (uint32_t)BRQ_CTX; ++x) {
				const uint64_t a = cx[((uint64_t)q * BRC_MCTX + x) * 2], b = cx[((uint64_t)q * BRC_MCTX + x) * 2 + 1];
				r[1 + ncy + x] = a ? brq_fixed(brq_emp(a, b) - B) : 0;
			}
		}
	}
	return BMH_OK;
}

// the message of the record with index `rec` that brq_prep refuses with `code`
inline int brq_refused(uint64_t rec, int code, const char *fn)
{
	const unsigned long long i = (unsigned long long)rec;
	switch (code) {
	case BRC_E_TAGS: bmh_set_error("%s: record %llu has tags that cannot be walked to the record's end: the qualities are recalibrated by the read group its RG tag names", fn, i); break;
	case BRC_E_RG_NONE: bmh_set_error("%s: record %llu has no RG tag: the table to apply is kept per read group", fn, i); break;
	case BRC_E_RG_TYPE: bmh_set_error("%s: record %llu has an RG tag of another type than Z", fn, i); break;
	case BRC_E_RG_ID: bmh_set_error("%s: record %llu names a read group the table to apply does not hold", fn, i); break;
	default: bmh_set_error("%s: record %llu is not whole: its bytes do not hold the fields, the name, the operations, the bases and the qualities it announces", fn, i); break;
	}
	return BMH_EINVAL;
}

// the counts: the summary words (BRQ_*), then the histograms of the qualities before and after [2][94] (a quality above 93 in bin 93)
struct brq_result_t { std::vector<uint64_t> w; };

// the host form
struct brq_host_t {
	const brq_run_t *U = nullptr; brq_result_t R; uint64_t n_seen = 0;
	void begin(const brq_run_t &run) { U = &run; R.w.assign((size_t)BRQ_WORDS, 0); n_seen = 0; }
	// a window's n records recs + soff[j], rewritten in place; the first record refused ends the run
	int window(uint8_t *recs, const uint64_t *soff, uint32_t n, const char *fn)
	{
		const brq_plan_t &P = U->P; const brq_tab_t T = U->host_tab();
		uint64_t *w = R.w.data();
		for (uint32_t j = 0; j < n; ++j, ++n_seen) {
			brq_rec_t r;
			uint8_t *rec = recs + soff[j];
			const int st = soff[j + 1] >= soff[j] ? brq_prep(rec, soff[j + 1] - soff[j], P, T, r) : (int)BRC_E_CUT;
			++w[BRQ_SEEN];
			if (st == BRQ_SKIP) { ++w[BRQ_NOQUAL]; continue; }
			if (st != BRC_OK) return brq_refused(n_seen, st, fn);
			++w[BRQ_REWRITTEN]; w[BRQ_BASES] += r.l_seq;
			// (sequencing-order neighbours are bases, which do not change: the qualities can be rewritten as the walk goes)
			for (uint64_t i = 0; i < r.l_seq; ++i) {
				brq_obs_t o;
				const uint32_t q0 = rec[r.qual_at + i], q1 = brq_base(rec, r, P, T.t, i, q0, o);
				++w[BRQ_N_SUM + (q0 < (uint32_t)BRQ_MAX_Q ? q0 : (uint32_t)BRQ_MAX_Q)]; ++w[BRQ_N_SUM + BRC_NQ + (q1 < (uint32_t)BRQ_MAX_Q ? q1 : (uint32_t)BRQ_MAX_Q)];
				if (o.low) { ++w[BRQ_LOW]; continue; }
				++w[q1 != q0 ? BRQ_CHANGED : BRQ_UNCHANGED]; w[BRQ_CAPPED] += o.capped; w[BRQ_NOCTX] += o.noctx;
				rec[r.qual_at + i] = (uint8_t)q1;
			}
		}
		return BMH_OK;
	}
};

#ifndef BRC_STANDALONE
// the table of the options' apply record -> U
inline int brq_run_from_opt(brq_run_t &U, const bmh_recal_apply_opt_t *a, const char *fn)
{
	if (!a || !a->table) { bmh_set_error("%s: null argument (the table to apply)", fn); return BMH_EINVAL; }
	const bmh_recal_t *t = a->table;
	return brq_run_make(U, t->n_groups, t->min_qual, t->max_cycle, t->n_qual, t->cycle_m, t->context_m, a->rg_ids, fn);
}

// csrc/bam_requal_kernels.hip
struct brq_dev_t;                                                  // the device form's tables, counts and state; one per sorted run
brq_dev_t *brq_dev_create(void);
void brq_dev_free(brq_dev_t *d);
// the counts cleared, the tables and the group IDs uploaded
int brq_begin_device(brq_dev_t *d, const brq_run_t &U, void *stream);
// a window's records d_recs at d_soff [n + 1] (device), rewritten in place: one kernel, and the refusal word on its way to the host.  With ms (or NULL) events are
// recorded around the kernel.  Nothing waits here: brq_window_ms, once the caller has waited for the stream, refuses the window by its first refused record and,
// with ms, ms[0] += the kernel's milliseconds, ms[1] += 1 (the windows timed)
int brq_window_device(brq_dev_t *d, uint8_t *d_recs, const uint64_t *d_soff, uint32_t n, void *stream, double *ms);
int brq_window_ms(brq_dev_t *d, double *ms, const char *fn);
// the results: the run's one read of the counts
int brq_finish_device(brq_dev_t *d, void *stream, brq_result_t &R, const char *fn);
#endif
