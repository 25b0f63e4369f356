// Flagstat, idxstats, alignment summary and insert sizes on the host (csrc/bam_stats_core.h's rules): the plan, the host form -- the same
// accumulator as csrc/bam_stats_kernels.hip, added to record by record in plain C++ --, the export, the refusals' words and bmh_bam_stats_host.
#include <stdlib.h>
#include <string.h>
#include <stddef.h>
#include <algorithm>
#include <new>
#include "bam_stats.h"

int bst_plan_make(bst_plan_t &P, uint32_t insert_cap, int n_contigs, const char *fn)
{
	if (insert_cap < (uint32_t)BST_CAP_MIN || insert_cap > (uint32_t)BST_CAP_MAX) { bmh_set_error("%s: insert_cap %u (%d .. %d)", fn, insert_cap, (int)BST_CAP_MIN, (int)BST_CAP_MAX); return BMH_EINVAL; }
	if (n_contigs < 0) { bmh_set_error("%s: %d contigs", fn, n_contigs); return BMH_EINVAL; }
	P.cap = insert_cap; P.n_contigs = n_contigs;
	return BMH_OK;
}

void bst_result_t::init(const bst_plan_t &P)
{
	w.assign(P.words(), 0);
	for (int o = 0; o < BST_N_ORI; ++o) w[(size_t)BST_W_MIN + o] = ~0ull;
}

void bst_result_t::close(const bst_plan_t &P)
{
	(void)P;
	for (int o = 0; o < BST_N_ORI; ++o) if (w[(size_t)BST_W_MIN + o] == ~0ull) w[(size_t)BST_W_MIN + o] = 0;
}

int bst_refused(uint64_t rec, int code, const char *fn)
{
	const unsigned long long i = (unsigned long long)rec;
	switch (code) {
	case BST_E_REF: bmh_set_error("%s: record %llu names a reference outside the header's (refID below -1 or not below the number of contigs)", fn, i); break;
	case BST_E_TAGS: bmh_set_error("%s: record %llu has tags that cannot be walked to the record's end: the statistics read NM from them", fn, i); break;
	case BST_E_NM: bmh_set_error("%s: record %llu has an NM tag that is no count (a type other than c C s S i I, or a negative value)", fn, i); break;
	case BST_E_PLACEHOLDER: bmh_set_error("%s: record %llu holds the long-CIGAR placeholder (its operations are in its CG tag): the statistics read the record's own operations", fn, i); break;
	default: bmh_set_error("%s: record %llu is not whole: its bytes do not hold the fields, the name and the operations it announces", fn, i); break;
	}
	return BMH_EINVAL;
}

void bst_host_t::begin(const bst_plan_t &plan) { P = plan; R.init(P); n_seen = 0; }

int bst_host_t::window(const uint8_t *recs, const uint64_t *soff, uint32_t n, const char *fn)
{
	uint64_t *w = R.w.data();
	for (uint32_t j = 0; j < n; ++j, ++n_seen) {
		bst_rec_t r;
		const int st = bst_record(recs + soff[j], soff[j + 1] - soff[j], P.n_contigs, r);
		if (st != BST_OK) return bst_refused(n_seen, st, fn);
		for (int k = 0; k < BST_N_FLAG; ++k) if (r.flags >> k & 1u) ++w[(size_t)BST_W_FLAG + BST_N_FLAG * r.qc + k];
		if (r.ref < 0) ++w[BST_W_UNPLACED];
		else ++w[P.w_contig() + (r.placed_mapped ? 0 : (size_t)P.n_contigs) + (size_t)r.ref];
		if (!r.primary) continue;
		for (int k = 0; k < BST_N_SUM; ++k) {
			uint64_t &a = w[(size_t)BST_W_SUM + k];
			if (k == BST_MAX_LEN) a = std::max(a, r.sum[k]); else a += r.sum[k];
		}
		if (r.mapped) ++w[(size_t)BST_W_MAPQ + r.mapq];
		if (r.ori >= 0) {
			++w[P.w_hist() + bst_hist_at(r.ori, r.size, P.cap)];
			w[(size_t)BST_W_MIN + r.ori] = std::min(w[(size_t)BST_W_MIN + r.ori], r.size); w[(size_t)BST_W_MAX + r.ori] = std::max(w[(size_t)BST_W_MAX + r.ori], r.size);
		}
	}
	return BMH_OK;
}

#ifndef BST_STANDALONE
#include "bam_sort.h"

extern "C" void bmh_bam_stats_opt_default(bmh_bam_stats_opt_t *o) { if (o) o->insert_cap = BST_CAP_MAX; }

extern "C" void bmh_bam_stats_free(bmh_bam_stats_t *s)
{
	if (!s) return;
	free(s->flag); free(s->summary); free(s->mapq); free(s->contig_mapped); free(s->contig_unmapped); free(s->insert_hist);
	s->flag = s->summary = s->mapq = s->contig_mapped = s->contig_unmapped = s->insert_hist = nullptr;
}

int bst_export(const bst_plan_t &P, const bst_result_t &R, bmh_bam_stats_t *out, const char *fn)
{
	memset(out, 0, sizeof *out);
	const uint64_t *w = R.w.data();
	auto dup = [w](size_t at, size_t n) { uint64_t *p = (uint64_t *)malloc(8 * n + 8); if (p && n) memcpy(p, w + at, 8 * n); return p; };
	const size_t n = (size_t)P.n_contigs;
	out->n_contigs = P.n_contigs; out->insert_cap = P.cap;
	out->flag = dup(BST_W_FLAG, 2 * BST_N_FLAG); out->summary = dup(BST_W_SUM, BST_N_SUM); out->mapq = dup(BST_W_MAPQ, 256);
	out->contig_mapped = dup(P.w_contig(), n); out->contig_unmapped = dup(P.w_contig() + n, n); out->insert_hist = dup(P.w_hist(), P.hist_words());
	if (!out->flag || !out->summary || !out->mapq || !out->contig_mapped || !out->contig_unmapped || !out->insert_hist) {
		bmh_bam_stats_free(out);
		memset(out, 0, sizeof *out);
		bmh_set_error("%s: out of memory", fn); return BMH_ENOMEM;
	}
	out->unplaced = w[BST_W_UNPLACED];
	for (int o = 0; o < BST_N_ORI; ++o) { out->insert_min[o] = w[(size_t)BST_W_MIN + o]; out->insert_max[o] = w[(size_t)BST_W_MAX + o]; }
	return BMH_OK;
}

int bst_walk(const uint8_t *recs, uint64_t n_bytes, std::vector<uint64_t> &off, const char *fn)
{
	off.assign(1, 0);
	for (uint64_t p = 0; p < n_bytes;) {
		const uint64_t sz = bsr_record_bytes(recs + p, n_bytes - p);
		if (!sz) { bmh_set_error("%s: the bytes at %llu begin no whole BAM record (the stream is cut, or is no record stream)", fn, (unsigned long long)p); return BMH_EINVAL; }
		p += sz; off.push_back(p);
		if (off.size() > 0xfffffff0ull) { bmh_set_error("%s: 2^32 records", fn); return BMH_EINVAL; }
	}
	return BMH_OK;
}

// the records of a stream, in any order
extern "C" int bmh_bam_stats_host(const uint8_t *recs, uint64_t n_bytes, int n_contigs, const bmh_bam_stats_opt_t *opt, bmh_bam_stats_t *out)
{
	const char *fn = "bmh_bam_stats_host";
	if (!out || (n_bytes && !recs)) { bmh_set_error("%s: null argument", fn); return BMH_EINVAL; }
	memset(out, 0, sizeof *out);
	bmh_bam_stats_opt_t o; bmh_bam_stats_opt_default(&o);
	if (opt) o = *opt;
	bst_plan_t P;
	int rc = bst_plan_make(P, o.insert_cap, n_contigs, fn);
	if (rc != BMH_OK) return rc;
	std::vector<uint64_t> off;
	if ((rc = bst_walk(recs, n_bytes, off, fn)) != BMH_OK) return rc;
	try {
		bst_host_t H; H.begin(P);
		const size_t n = off.size() - 1;
		for (size_t a = 0; a < n; a += 1u << 20) {
			const size_t b = std::min(n, a + (1u << 20));
			if ((rc = H.window(recs, off.data() + a, (uint32_t)(b - a), fn)) != BMH_OK) return rc;
		}
		H.finish();
		return bst_export(P, H.R, out, fn);
	} catch (const std::bad_alloc &) { bmh_set_error("%s: out of memory", fn); return BMH_ENOMEM; }
}
#endif
