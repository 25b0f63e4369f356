// Whole-file templates by name on the host (BDP_TPL_FILE; csrc/bam_tpl_core.h has the rules): the parts of a record, the grouping with
// std::stable_sort and the fold of every set, the refusals' words, and the step on its own -- bmh_bam_templates_host and what it shares with
// bmh_bam_templates_device (csrc/bam_tpl_kernels.hip).
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <new>
#include <numeric>
#include "bam_tpl.h"
#include "bam_post.h"

void btp_append_host(btp_parts_t &S, const uint8_t *rec, uint64_t sz, const bdp_plan_t &P, uint32_t hash_bits)
{
	const bdp_groups_t G = P.table.view();
	uint64_t w = 0; bdp_loc_t l;
	S.parts.push_back(btp_part(rec, sz, P.groups() ? &G : nullptr, P.barcode(), &w, P.optical() ? &l : nullptr, hash_bits));
	if (P.optical()) S.locs.push_back(l);
	if (P.barcode()) S.bcs.push_back(w);
}

int btp_group_host(const btp_parts_t &S, const bdp_plan_t &P, btp_result_t &R, const char *fn)
{
	const size_t n = S.parts.size();
	const bool groups = P.groups() != nullptr, barcode = P.barcode() != nullptr, optical = P.optical() != nullptr;
	const uint32_t n_lib = P.n_lib();
	R = btp_result_t();
	if (n > 0xfffffff0ull) { bmh_set_error("%s: 2^32 records", fn); return BMH_EINVAL; }
	const btp_part_t *Pt = S.parts.data();
	std::vector<uint32_t> idx(n), ord(n, 0);
	std::iota(idx.begin(), idx.end(), 0u);
	std::stable_sort(idx.begin(), idx.end(), [Pt](uint32_t a, uint32_t b) { return Pt[a].h1 != Pt[b].h1 ? Pt[a].h1 < Pt[b].h1 : Pt[a].h0 < Pt[b].h0; });
	for (size_t j = 0; j < n; ++j) if (j == 0 || !btp_key_equal(Pt[idx[j]], Pt[idx[j - 1]])) ord[idx[j]] = 1;       // a set's first member is its smallest index: the sort is stable
	uint64_t T = 0;
	for (size_t i = 0; i < n; ++i) { const uint32_t f = ord[i]; ord[i] = (uint32_t)T; T += f; }
	if (T >= 1ull << 31) { bmh_set_error("%s: duplicate marking: 2^31 templates", fn); return BMH_EINVAL; }
	R.rec_tpl.resize(n); R.E.resize((size_t)T);
	if (optical) R.locs.resize((size_t)T);
	if (barcode) R.bcs.resize((size_t)T);
	for (size_t j = 0; j < n;) {
		size_t k = j + 1;
		while (k < n && btp_key_equal(Pt[idx[k]], Pt[idx[j]])) ++k;
		const uint32_t f = idx[j], t = ord[f]; uint32_t role = 0;
		const int st = btp_fold(Pt, idx.data() + j, (uint32_t)(k - j), groups, barcode, &R.E[t], &role);
		if (st != BDP_E_OK) R.word = std::min(R.word, bpo_refusal(f, st));
		if (optical) R.locs[t] = btp_location(S.locs[f], role, Pt[f], groups);
		if (barcode) R.bcs[t] = S.bcs[f];
		for (size_t q = j; q < k; ++q) R.rec_tpl[idx[q]] = t;
		j = k;
	}
	if (R.word != BPO_NONE) return BMH_OK;
	if (groups) R.lib3.assign(3 * (size_t)n_lib, 0);
	for (size_t i = 0; i < n; ++i) {
		const uint32_t b = Pt[i].bits, t = R.rec_tpl[i];
		R.info[0] += (b & BTP_SECSUP) != 0; R.info[1] += (b & BTP_UNMAPPED) != 0;
		const uint32_t lib = groups ? bdp_lib_of(R.E[t]) : n_lib;
		if (lib < n_lib) { R.lib3[3 * lib] += (b & BTP_SECSUP) != 0; R.lib3[3 * lib + 1] += (b & BTP_UNMAPPED) != 0; }
	}
	for (size_t t = 0; t < (size_t)T && groups; ++t) { const uint32_t lib = bdp_lib_of(R.E[t]); if (lib < n_lib) ++R.lib3[3 * lib + 2]; }
	return BMH_OK;
}

int btp_refused(const btp_parts_t &S, uint64_t word, const bdp_plan_t &P, uint64_t sam_line0, const char *fn)
{
	const uint64_t index = word >> 3; const int code = (int)(word & 7u);
	if (index >= S.parts.size()) { bmh_set_error("%s: internal error: record %llu of %zu refused", fn, (unsigned long long)index, S.parts.size()); return BMH_EINVAL; }
	if (code >= BDP_E_BC_TYPE) return bdp_barcode_refused((uint32_t)index, code, fn);
	if (code != BDP_E_TEMPLATE) return bdp_group_refused((uint32_t)index, code, fn);
	std::vector<uint32_t> mem;
	for (size_t i = 0; i < S.parts.size(); ++i) if (btp_key_equal(S.parts[i], S.parts[(size_t)index])) mem.push_back((uint32_t)i);
	bdp_entry_t e; btp_lines_t ln;
	(void)btp_fold(S.parts.data(), mem.data(), (uint32_t)mem.size(), P.groups() != nullptr, P.barcode() != nullptr, &e, nullptr, &ln);
	char where[64] = "";
	if (sam_line0) snprintf(where, sizeof where, " (line %llu)", (unsigned long long)(sam_line0 + index));
	bmh_set_error("%s: duplicate marking: the %zu records of the whole file under the read name of record %llu%s hold %u primary lines (%u with 0x40, %u with 0x80; %s): a paired name "
	              "needs exactly one 0x40 and one 0x80 primary line and an unpaired one exactly one primary line -- two templates under one name, or a template that lacks a record",
	              fn, mem.size(), (unsigned long long)index, where, ln.n_pri, ln.n_first, ln.n_second, ln.paired ? "paired" : "unpaired");
	return BMH_EINVAL;
}

// ---------------------------------------------------------------------------------------------------------------- the step on its own

int btp_templates_begin(const uint8_t *recs, uint64_t n_bytes, const bmh_markdup_opt_t *opt, int32_t hash_bits, bmh_bam_templates_t *out, const char *fn, bdp_plan_t &P, std::vector<uint64_t> &off)
{
	if (out) memset(out, 0, sizeof *out);
	if (!out || (!recs && n_bytes)) { bmh_set_error("%s: null argument", fn); return BMH_EINVAL; }
	if (hash_bits < 1 || hash_bits > 128) { bmh_set_error("%s: hash_bits %d (1 .. 128)", fn, hash_bits); return BMH_EINVAL; }
	bmh_markdup_opt_t o; bmh_markdup_counts_t res; memset(&res, 0, sizeof res);
	if (opt) o = *opt; else bmh_markdup_opt_default(&o);
	if (o.optical_distance == -1) o.optical_distance = 0;             // (the locations are part of what the step gives)
	const int rc = bdp_plan_make(P, &o, &res, fn);
	P.opt.out = P.grp.out = P.no_barcode = nullptr; P.lib_counts = nullptr;      // (res ends here: the step counts nothing of the decision's)
	if (rc != BMH_OK) return rc;
	off.assign(1, 0);
	for (uint64_t p = 0; p < n_bytes;) {
		const uint64_t i = off.size() - 1, sz = bsr_record_bytes(recs + p, n_bytes - p);
		if (!sz) { bmh_set_error("%s: record %llu is cut: the stream ends inside it", fn, (unsigned long long)i); return BMH_EINVAL; }
		const int st = bpo_check(recs + p, sz, 0x7fffffff, BPO_MARKDUP);
		if (st != BPO_OK) return bpo_refused(fn, i, st, recs + p, sz, 0x7fffffff);
		p += sz; off.push_back(p);
	}
	if (off.size() - 1 > 0xfffffff0ull) { bmh_set_error("%s: 2^32 records", fn); return BMH_EINVAL; }
	return BMH_OK;
}

template <class T> static T *copy_of(const std::vector<T> &v)
{
	T *p = (T *)malloc(sizeof(T) * v.size() + 8);
	if (p && !v.empty()) memcpy(p, v.data(), sizeof(T) * v.size());
	return p;
}

int btp_templates_export(const btp_result_t &R, const bdp_plan_t &P, bmh_bam_templates_t *out, const char *fn)
{
	bmh_bam_templates_t r; memset(&r, 0, sizeof r);
	r.n_records = R.rec_tpl.size(); r.n_templates = R.E.size();
	r.tpl = copy_of(R.rec_tpl); r.entries = (uint8_t *)copy_of(R.E); r.locs = (uint8_t *)copy_of(R.locs);
	if (P.barcode()) r.barcodes = copy_of(R.bcs);
	if (P.groups()) { r.lib_counts = copy_of(R.lib3); r.n_libraries = (int32_t)P.n_lib(); }
	if (!r.tpl || !r.entries || !r.locs || (P.barcode() && !r.barcodes) || (P.groups() && !r.lib_counts)) { bmh_bam_templates_free(&r); bmh_set_error("%s: out of memory", fn); return BMH_ENOMEM; }
	r.counts[0] = R.info[0]; r.counts[1] = R.info[1]; r.counts[2] = R.E.size();
	*out = r;
	return BMH_OK;
}

extern "C" void bmh_bam_templates_free(bmh_bam_templates_t *r)
{
	if (!r) return;
	free(r->tpl); free(r->entries); free(r->locs); free(r->barcodes); free(r->lib_counts);
	memset(r, 0, sizeof *r);
}

extern "C" int bmh_bam_templates_host(const uint8_t *records, uint64_t n_bytes, const bmh_markdup_opt_t *opt, int32_t hash_bits, bmh_bam_templates_t *out)
{
	const char *fn = "bmh_bam_templates_host";
	try {
		bdp_plan_t P; std::vector<uint64_t> off;
		int rc = btp_templates_begin(records, n_bytes, opt, hash_bits, out, fn, P, off);
		if (rc != BMH_OK) return rc;
		btp_parts_t S; btp_result_t R;
		for (size_t i = 0; i + 1 < off.size(); ++i) btp_append_host(S, records + off[i], off[i + 1] - off[i], P, (uint32_t)hash_bits);
		if ((rc = btp_group_host(S, P, R, fn)) != BMH_OK) return rc;
		if (R.word != BPO_NONE) return btp_refused(S, R.word, P, 0, fn);
		return btp_templates_export(R, P, out, fn);
	} catch (const std::bad_alloc &) { bmh_set_error("%s: out of memory", fn); return BMH_ENOMEM; }
}
