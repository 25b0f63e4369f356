// The covariate table of base quality score recalibration on the host (csrc/bam_recal_core.h's rules): the mask's parser (known sites as VCF or BED
// text, the reference's holes) and the entry points of the host form, which csrc/bam_recal.h holds inline -- the same accumulator as csrc/bam_recal_kernels.hip,
// added to base by base in plain C++.
#include <stdlib.h>
#include <string.h>
#include <stddef.h>
#include <algorithm>
#include <new>
#include "bam_recal.h"

// ---------------------------------------------------------------------------------------------------------------- the mask

namespace {
// the fields of a line: at tabs (VCF), at tabs and blanks (BED)
size_t split(const char *s, size_t n, bool blanks, const char **f, size_t *fl, size_t max)
{
	size_t k = 0, a = 0;
	for (size_t i = 0; i <= n && k < max; ++i)
		if (i == n || s[i] == '\t' || (blanks && s[i] == ' ')) {
			if (i > a || !blanks) { f[k] = s + a; fl[k] = i - a; ++k; }
			a = i + 1;
		}
	return k;
}
bool number(const char *s, size_t n, uint64_t *v)
{
	if (!n || n > 18) return false;
	uint64_t x = 0;
	for (size_t i = 0; i < n; ++i) { if (s[i] < '0' || s[i] > '9') return false; x = 10 * x + (uint64_t)(s[i] - '0'); }
	*v = x;
	return true;
}
bool begins(const char *s, size_t n, const char *w) { const size_t l = strlen(w); return n >= l && !memcmp(s, w, l); }
}   // namespace

int brc_mask_parser_t::line(const char *s, size_t n)
{
	++line_no;
	while (n && (s[n - 1] == '\r' || s[n - 1] == '\n')) --n;
	if (!n) return BMH_OK;
	const unsigned long long ln = (unsigned long long)line_no;
	if (format < 0) format = begins(s, n, "##fileformat=VCF") || begins(s, n, "#CHROM") ? 1 : 0;
	if (s[0] == '#') return BMH_OK;
	if (format == 0 && (begins(s, n, "track") || begins(s, n, "browser"))) return BMH_OK;
	const char *f[4]; size_t fl[4];
	const size_t nf = split(s, n, format == 0, f, fl, 4), want = format ? 4 : 3;
	if (nf < want) { bmh_set_error("known sites: %s line %llu: %zu fields where a %s line has at least %zu", file.c_str(), ln, nf, format ? "VCF" : "BED", want); return BMH_EINVAL; }
	const brc_contig_t *c = nullptr;
	for (const brc_contig_t &t : *contigs) if (t.name.size() == fl[0] && !memcmp(t.name.data(), f[0], fl[0])) { c = &t; break; }
	if (!c) { bmh_set_error("known sites: %s line %llu: contig %.*s is not among the reference's", file.c_str(), ln, (int)std::min<size_t>(fl[0], 200), f[0]); return BMH_EINVAL; }
	uint64_t a, b;
	if (format) {
		if (!number(f[1], fl[1], &a)) { bmh_set_error("known sites: %s line %llu: POS %.*s is no number", file.c_str(), ln, (int)std::min<size_t>(fl[1], 40), f[1]); return BMH_EINVAL; }
		if (!a || !fl[3]) { bmh_set_error("known sites: %s line %llu: POS %llu with a REF of %zu bases lies outside contig %s", file.c_str(), ln, (unsigned long long)a, fl[3], c->name.c_str()); return BMH_EINVAL; }
		--a; b = a + fl[3];
	} else {
		if (!number(f[1], fl[1], &a)) { bmh_set_error("known sites: %s line %llu: start %.*s is no number", file.c_str(), ln, (int)std::min<size_t>(fl[1], 40), f[1]); return BMH_EINVAL; }
		if (!number(f[2], fl[2], &b)) { bmh_set_error("known sites: %s line %llu: end %.*s is no number", file.c_str(), ln, (int)std::min<size_t>(fl[2], 40), f[2]); return BMH_EINVAL; }
	}
	if (a > b || b > (uint64_t)c->len) { bmh_set_error("known sites: %s line %llu: [%llu, %llu) lies outside contig %s of %lld bases", file.c_str(), ln, (unsigned long long)a, (unsigned long long)b, c->name.c_str(), (long long)c->len); return BMH_EINVAL; }
	for (uint64_t i = c->off + a; i < c->off + b; ++i) mask[i >> 6] |= 1ull << (i & 63u);
	return BMH_OK;
}

int brc_mask_parser_t::feed(const char *text, size_t n)
{
	size_t a = 0;
	for (size_t i = 0; i < n; ++i) {
		if (text[i] != '\n') continue;
		int rc;
		if (!carry.empty()) { carry.append(text + a, i - a); rc = line(carry.data(), carry.size()); carry.clear(); }
		else rc = line(text + a, i - a);
		if (rc != BMH_OK) return rc;
		a = i + 1;
	}
	carry.append(text + a, n - a);
	return BMH_OK;
}

int brc_mask_parser_t::finish()
{
	if (carry.empty()) return BMH_OK;
	const int rc = line(carry.data(), carry.size());
	carry.clear();
	return rc;
}

#ifndef BRC_STANDALONE
extern "C" void bmh_recal_opt_default(bmh_recal_opt_t *o)
{
	if (!o) return;
	memset(o, 0, sizeof *o);
	o->min_qual = BRC_MIN_QUAL; o->max_cycle = BRC_MAX_CYCLE;
}

extern "C" void bmh_recal_free(bmh_recal_t *r)
{
	brc_release(r);
}

extern "C" int bmh_known_sites_mask(const char *const *paths, int n_paths, int n_contigs, const char *const *contig_names, const int32_t *contig_len, const uint64_t *contig_offset,
                                    uint64_t *mask, uint64_t mask_words)
{
	const char *fn = "bmh_known_sites_mask";
	if (n_paths < 0 || (n_paths && !paths) || n_contigs < 0 || (n_contigs && (!contig_names || !contig_len)) || (mask_words && !mask)) { bmh_set_error("%s: null argument", fn); return BMH_EINVAL; }
	try {
		std::vector<brc_contig_t> contigs;
		uint64_t at = 0;
		for (int c = 0; c < n_contigs; ++c) {
			const uint64_t o = contig_offset ? contig_offset[c] : at;
			if (contig_len[c] < 0 || o + (uint64_t)contig_len[c] > 64 * mask_words) { bmh_set_error("%s: contig %d lies outside the mask's %llu words", fn, c, (unsigned long long)mask_words); return BMH_EINVAL; }
			contigs.push_back(brc_contig_t{contig_names[c] ? contig_names[c] : "", o, contig_len[c]});
			at = o + (uint64_t)contig_len[c];
		}
		std::vector<uint8_t> buf(1u << 20);
		for (int k = 0; k < n_paths; ++k) {
			if (!paths[k]) { bmh_set_error("%s: null argument", fn); return BMH_EINVAL; }
			bmh_text_src_t *s = bmh_text_open(paths[k], 1);
			if (!s) return BMH_EINVAL;
			brc_mask_parser_t M; M.file = paths[k]; M.contigs = &contigs; M.mask = mask;
			int rc = BMH_OK;
			for (;;) {
				const int64_t g = bmh_text_read(s, buf.data(), buf.size());
				if (g < 0) { rc = BMH_EINVAL; break; }
				if ((rc = M.feed((const char *)buf.data(), (size_t)g)) != BMH_OK || (size_t)g < buf.size()) break;
			}
			if (rc == BMH_OK) rc = M.finish();
			bmh_text_close(s);
			if (rc != BMH_OK) return rc;
		}
	} catch (const std::bad_alloc &) { bmh_set_error("%s: out of memory", fn); return BMH_ENOMEM; }
	return BMH_OK;
}

extern "C" int bmh_recal_mask_holes(const uint64_t *hole_offset, const uint64_t *hole_len, int n_holes, uint64_t *mask, uint64_t mask_words)
{
	const char *fn = "bmh_recal_mask_holes";
	if (n_holes < 0 || (n_holes && (!hole_offset || !hole_len || !mask))) { bmh_set_error("%s: null argument", fn); return BMH_EINVAL; }
	for (int h = 0; h < n_holes; ++h) {
		if (hole_offset[h] > 64 * mask_words || hole_len[h] > 64 * mask_words - hole_offset[h]) { bmh_set_error("%s: hole %d lies outside the mask's %llu words", fn, h, (unsigned long long)mask_words); return BMH_EINVAL; }
		for (uint64_t i = hole_offset[h]; i < hole_offset[h] + hole_len[h]; ++i) mask[i >> 6] |= 1ull << (i & 63u);
	}
	return BMH_OK;
}

#include "bam_stats.h"

// the records of a stream, in any order
extern "C" int bmh_bam_recal_host(const uint8_t *recs, uint64_t n_bytes, int n_contigs, const int32_t *contig_len, const bmh_recal_opt_t *opt, bmh_recal_t *out)
{
	const char *fn = "bmh_bam_recal_host";
	if (!out || (n_bytes && !recs)) { bmh_set_error("%s: null argument", fn); return BMH_EINVAL; }
	memset(out, 0, BRC_RECAL_OLD_BYTES);
	try {
		brc_run_t U;
		int rc = brc_run_from_opt(U, opt, n_contigs, contig_len, true, fn);
		if (rc != BMH_OK) return rc;
		std::vector<uint64_t> off;
		if ((rc = bst_walk(recs, n_bytes, off, fn)) != BMH_OK) return rc;
		brc_host_t H; H.begin(U);
		const size_t n = off.size() - 1;
		for (size_t a = 0; a < n; a += 1u << 20) {
			const size_t b = std::min(n, a + (1u << 20));
			if ((rc = H.window(recs, off.data() + a, (uint32_t)(b - a), fn)) != BMH_OK) return rc;
		}
		H.finish();
		return brc_export(&U, &H.R, out, fn);
	} catch (const std::bad_alloc &) { bmh_set_error("%s: out of memory", fn); return BMH_ENOMEM; }
}

// ---------------------------------------------------------------------------------------------------------------- applying a table

extern "C" int bmh_recal_apply_tables(const bmh_recal_apply_opt_t *apply, int16_t **tables, uint64_t *n_entries)
{
	const char *fn = "bmh_recal_apply_tables";
	if (tables) *tables = nullptr;
	if (!tables || !n_entries) { bmh_set_error("%s: null argument", fn); return BMH_EINVAL; }
	*n_entries = 0;
	try {
		brq_run_t U;
		const int rc = brq_run_from_opt(U, apply, fn);
		if (rc != BMH_OK) return rc;
		int16_t *t = (int16_t *)malloc(2 * U.t.size() + 2);
		if (!t) { bmh_set_error("%s: out of memory", fn); return BMH_ENOMEM; }
		memcpy(t, U.t.data(), 2 * U.t.size());
		*tables = t; *n_entries = U.t.size();
		return BMH_OK;
	} catch (const std::bad_alloc &) { bmh_set_error("%s: out of memory", fn); return BMH_ENOMEM; }
}

extern "C" int bmh_bam_requal_host(const uint8_t *recs, uint64_t n_bytes, const bmh_recal_apply_opt_t *apply, uint8_t **out, bmh_recal_t *counts)
{
	const char *fn = "bmh_bam_requal_host";
	if (out) *out = nullptr;
	if (!out || !counts || (n_bytes && !recs)) { bmh_set_error("%s: null argument", fn); return BMH_EINVAL; }
	memset(counts, 0, sizeof *counts);
	try {
		brq_run_t U;
		int rc = brq_run_from_opt(U, apply, fn);
		if (rc != BMH_OK) return rc;
		std::vector<uint64_t> off;
		if ((rc = bst_walk(recs, n_bytes, off, fn)) != BMH_OK) return rc;
		uint8_t *res = (uint8_t *)malloc((size_t)n_bytes + 1);
		if (!res) { bmh_set_error("%s: out of memory", fn); return BMH_ENOMEM; }
		if (n_bytes) memcpy(res, recs, (size_t)n_bytes);
		brq_host_t H; H.begin(U);
		const size_t n = off.size() - 1;
		for (size_t a = 0; a < n && rc == BMH_OK; a += 1u << 20) rc = H.window(res, off.data() + a, (uint32_t)(std::min(n, a + (1u << 20)) - a), fn);
		if (rc == BMH_OK) rc = brc_export(nullptr, nullptr, counts, fn, &H.R);
		if (rc != BMH_OK) { free(res); return rc; }
		*out = res;
		return BMH_OK;
	} catch (const std::bad_alloc &) { bmh_set_error("%s: out of memory", fn); return BMH_ENOMEM; }
}
#endif
