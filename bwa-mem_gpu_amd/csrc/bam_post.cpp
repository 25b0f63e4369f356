// Sort, mark duplicates and index a BAM or SAM that any aligner wrote, on the host (csrc/bam_post_core.h has the rules): the input -- its
// header, its records in batches that end where a read name ends --, the words of the refusals, the run's options, and bmh_bam_post_file_host, which does with the
// host forms of every step (bsr_sort_host, bdp_entries_host, bdp_decide_host, bcv_host_t, the host window and index path) what csrc/bam_post_kernels.hip does on
// the device.  The host form holds the whole record stream in memory.  With collate (BDP_TPL_FILE, csrc/bam_tpl_core.h) batches are cut at record boundaries, a
// batch leaves its records' parts instead of entries, and the templates of the whole file are formed behind the last batch (btp_group_host).
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <new>
#include "bam_post.h"

// ---------------------------------------------------------------------------------------------------------------- the input

static void hd_first(const std::string &text, std::string &out)
{
	out = "@HD\tVN:1.6\tSO:coordinate\n";
	for (size_t a = 0; a < text.size();) {
		size_t e = text.find('\n', a);
		e = e == std::string::npos ? text.size() : e + 1;
		const bool hd = text.compare(a, 3, "@HD") == 0 && (a + 3 >= text.size() || text[a + 3] == '\t' || text[a + 3] == '\n' || text[a + 3] == '\r');
		if (!hd) out.append(text, a, e - a);
		a = e;
	}
}

int bpo_input_t::open(const char *p, const char *fn, bpo_convert_t conv)
{
	path = p; convert = conv;
	const int tune = bmh_tune("BAM_POST_CHUNK", 0);                 // (the bytes asked of the source at a time; for the tests, which make records straddle them)
	if (tune > 0) chunk = (size_t)tune;
	if (!(src = bmh_text_open(p, 0))) return BMH_EINVAL;
	const int kind = bmh_text_bam(src);
	if (kind < 0) return BMH_EINVAL;
	if (kind == 2) { bmh_set_error("%s: %s holds a BAM inside a plain gzip stream: BAM is BGZF", fn, p); return BMH_EINVAL; }
	bam = kind == 1;
	const int rc = bam ? bam_header(fn) : sam_header(fn);
	if (rc != BMH_OK) return rc;
	ctg_blob.clear(); ctg_noff.assign(1, 0);
	for (const std::string &nm : names) { ctg_blob += nm; ctg_blob.push_back('\0'); ctg_noff.push_back((uint32_t)ctg_blob.size()); }
	chain.assign(1, 0u);
	return BMH_OK;
}

int bpo_input_t::bam_header(const char *fn)
{
	int64_t hb = 0;
	while (!(hb = bmh_bam_header_bytes(buf.data(), have)) && !eof) {
		buf.resize(have + chunk);
		const int64_t g = bmh_text_read(src, buf.data() + have, chunk);
		if (g < 0) return BMH_EINVAL;
		if ((size_t)g < chunk) eof = true;
		have += (size_t)g;
	}
	if (hb <= 0) { bmh_set_error("%s: %s: the BAM header is %s", fn, path.c_str(), hb < 0 ? "not one (no magic bytes)" : "cut"); return BMH_EINVAL; }
	const uint8_t *b = buf.data();
	const uint32_t l_text = bsr_u32(b + 4);
	std::string text((const char *)b + 8, l_text);
	text.resize(strlen(text.c_str()));                              // (the text ends at its first NUL)
	hd_first(text, header);
	size_t p = 8 + (size_t)l_text;
	const uint32_t n_ref = bsr_u32(b + p);
	p += 4;
	for (uint32_t i = 0; i < n_ref; ++i) {
		const uint32_t ln = bsr_u32(b + p);
		std::string nm((const char *)b + p + 4, ln);
		nm.resize(strlen(nm.c_str()));
		names.push_back(nm); len.push_back((int32_t)bsr_u32(b + p + 4 + ln));
		p += 8 + (size_t)ln;
	}
	memmove(buf.data(), buf.data() + hb, have - (size_t)hb); have -= (size_t)hb;
	return BMH_OK;
}

int bpo_input_t::sam_header(const char *fn)
{
	// the header ends at the first line that does not begin with '@': whole lines are taken until one is there, or the text ends
	std::string raw; size_t a = 0; bool done = false;
	std::vector<uint8_t> tmp(chunk);
	while (!done) {
		for (size_t e; a < text.size() && (e = text.find('\n', a)) != std::string::npos; a = e + 1) {
			if (text[a] != '@') { done = true; break; }
			raw.append(text, a, e + 1 - a); ++lines;
		}
		if (done || (a < text.size() && text[a] != '@')) break;
		if (src_eof) { if (a < text.size()) { raw.append(text, a, std::string::npos); a = text.size(); ++lines; } break; }
		const int64_t g = bmh_text_read(src, tmp.data(), chunk);
		if (g < 0) return BMH_EINVAL;
		if ((size_t)g < chunk) src_eof = true;
		text.append((const char *)tmp.data(), (size_t)g);
	}
	text.erase(0, a);
	header_lines = lines;
	eof = src_eof && text.empty();
	hd_first(raw, header);
	uint64_t line = 0;
	for (size_t s = 0; s < raw.size();) {
		size_t e = raw.find('\n', s);
		if (e == std::string::npos) e = raw.size();
		++line;
		if (raw.compare(s, 4, "@SQ\t") == 0) {
			std::string sn; long long ln = -1; bool has_ln = false;
			for (size_t f = s + 4; f <= e;) {
				size_t t = raw.find('\t', f);
				if (t == std::string::npos || t > e) t = e;
				size_t fe = t;
				if (fe > f && raw[fe - 1] == '\r') --fe;
				if (raw.compare(f, 3, "SN:") == 0) sn.assign(raw, f + 3, fe - f - 3);
				else if (raw.compare(f, 3, "LN:") == 0) {
					has_ln = fe > f + 3 && fe - f - 3 <= 10; ln = 0;
					for (size_t k = f + 3; k < fe && has_ln; ++k) { if (raw[k] < '0' || raw[k] > '9') has_ln = false; else ln = 10 * ln + (raw[k] - '0'); }
				}
				f = t + 1;
			}
			if (sn.empty() || !has_ln || ln < 1 || ln > 0x7fffffffll) { bmh_set_error("%s: %s: line %llu: an @SQ line needs SN and LN (1 .. 2^31 - 1)", fn, path.c_str(), (unsigned long long)line); return BMH_EINVAL; }
			names.push_back(sn); len.push_back((int32_t)ln);
		}
		s = e + 1;
	}
	if (names.empty()) { bmh_set_error("%s: %s: the SAM header has no @SQ line: the references of the BAM come from them", fn, path.c_str()); return BMH_EINVAL; }
	return BMH_OK;
}

// more record bytes behind buf [0, have): a window of the BAM's text, or the records of the SAM lines of one
int bpo_input_t::fill(const char *fn)
{
	if (bam) {
		if (buf.size() < have + chunk) buf.resize(have + chunk + have / 2);
		const int64_t g = bmh_text_read(src, buf.data() + have, chunk);
		if (g < 0) return BMH_EINVAL;
		if ((size_t)g < chunk) eof = true;
		have += (size_t)g;
		return BMH_OK;
	}
	if (!src_eof) {
		std::vector<uint8_t> tmp(chunk);
		const int64_t g = bmh_text_read(src, tmp.data(), chunk);
		if (g < 0) return BMH_EINVAL;
		if ((size_t)g < chunk) src_eof = true;
		text.append((const char *)tmp.data(), (size_t)g);
	}
	size_t e = src_eof ? text.size() : text.rfind('\n') == std::string::npos ? 0 : text.rfind('\n') + 1;
	if (e) {
		std::vector<uint8_t> recs; uint32_t bad = ~0u, status = 0;
		const int rc = convert(text.data(), e, (int)names.size(), ctg_blob, ctg_noff, recs, &bad, &status);
		if (rc != BMH_OK) return rc;
		if (bad != ~0u) {
			bmh_set_error("%s: %s: line %llu: its SAM record cannot be written as BAM: %s", fn, path.c_str(), (unsigned long long)(lines + bad + 1), bmh_bam_status_name(status));
			return BMH_EINVAL;
		}
		lines += (uint64_t)std::count(text.begin(), text.begin() + (ptrdiff_t)e, '\n');
		if (buf.size() < have + recs.size()) buf.resize(have + recs.size() + have / 2);
		if (!recs.empty()) memcpy(buf.data() + have, recs.data(), recs.size());
		have += recs.size();
		text.erase(0, e);
	}
	eof = src_eof;
	return BMH_OK;
}

int bpo_input_t::next(uint64_t batch_bytes, const char *fn)
{
	if (taken) {                                                       // the last batch leaves; the chain starts anew on what is left
		memmove(buf.data(), buf.data() + taken, have - taken);
		have -= taken; taken = 0; base += n; n = 0; chain.assign(1, 0u);
	}
	size_t k = 1;
	for (;;) {
		if (have >= 0xf0000000ull) { bmh_set_error("%s: %s: record %llu begins 3.75 GiB of records without a template's end", fn, path.c_str(), (unsigned long long)base); return BMH_EINVAL; }
		if (have) bmh_bam_chain_extend(buf.data(), have, chain);
		const size_t nrec = chain.size() - 1;
		if (nrec) {
			// the first record at or beyond batch_bytes, then the first head from there on: records k - 1 and k are both whole
			if (k < nrec && chain[k] < batch_bytes)
				k = (size_t)(std::lower_bound(chain.begin() + (ptrdiff_t)k, chain.begin() + (ptrdiff_t)nrec, batch_bytes, [](uint32_t a, uint64_t b) { return a < b; }) - chain.begin());
			while (!plain && k < nrec && bpo_name_equal(buf.data() + chain[k], chain[k + 1] - chain[k], buf.data() + chain[k - 1], chain[k] - chain[k - 1])) ++k;
			if (k < nrec || eof) {                                   // (at the end of the input the batch is what is left; bytes behind its last whole record wait for the next call)
				n = (uint32_t)k; taken = chain[k];
				off.resize(k + 1);
				for (size_t i = 0; i <= k; ++i) off[i] = chain[i];
				return 1;
			}
		} else if (eof) {
			if (have) { bmh_set_error("%s: %s: record %llu is cut: the input ends inside it", fn, path.c_str(), (unsigned long long)base); return BMH_EINVAL; }
			return 0;
		}
		const int rc = fill(fn);
		if (rc != BMH_OK) return rc;
	}
}

// ---------------------------------------------------------------------------------------------------------------- the run

extern "C" void bmh_bam_post_opt_default(bmh_bam_post_opt_t *o)
{
	if (!o) return;
	memset(o, 0, sizeof *o);
	bmh_sorted_opt_default(&o->sorted);
}

extern "C" void bmh_bam_post_result_free(bmh_bam_post_result_t *r)
{
	if (!r) return;
	free(r->index); free(r->header_text); free(r->contig_names); free(r->contig_len); free(r->library_names);
	r->index = nullptr; r->header_text = r->contig_names = r->library_names = nullptr; r->contig_len = nullptr;
}

int bpo_refused(const char *fn, uint64_t index, int code, const uint8_t *rec, uint64_t sz, int n_ref)
{
	const unsigned long long i = (unsigned long long)index;
	const bool fixed = sz >= BSR_FIXED;
	switch (code) {
	case BPO_E_CUT: bmh_set_error("%s: record %llu is not whole: its %llu bytes do not hold the fields, the name, the operations, the bases and the qualities it announces", fn, i, (unsigned long long)sz); break;
	case BPO_E_REF: bmh_set_error("%s: record %llu names reference %d and next reference %d of %d", fn, i, fixed ? bsr_ref(rec) : 0, fixed ? (int32_t)bsr_u32(rec + 24) : 0, n_ref); break;
	case BPO_E_PLACE: bmh_set_error("%s: duplicate marking: record %llu is a primary line without 0x4 and has no place (refID %d, pos %d)", fn, i, fixed ? bsr_ref(rec) : 0, fixed ? bsr_pos(rec) : 0); break;
	case BPO_E_END: bmh_set_error("%s: duplicate marking: record %llu has its unclipped 5' end at %lld: the duplicate key holds ends of -2^30 .. 2^30 - 1 (a clip this long is no alignment's)", fn, i, (long long)bpo_unclipped(rec)); break;
	case BPO_E_LONG: bmh_set_error("%s: record %llu holds the long-CIGAR placeholder (its operations are in its CG tag): duplicate marking and coverage read the record's own operations; a plain sort takes it", fn, i); break;
	default: return bdp_name_refused(index, fn);
	}
	return BMH_EINVAL;
}

uint32_t bpo_template_start(const uint8_t *recs, const uint64_t *off, uint32_t i)
{
	while (i > 0 && !bpo_head(recs, off, i)) --i;
	return i;
}

int bpo_run_t::begin(const char *path, const bmh_bam_post_opt_t *opt, bmh_sam_sink_t sink, bmh_bam_post_result_t *out, bmh_sorted_results_t *res, const char *f, bpo_convert_t conv)
{
	fn = f;
	if (out) memset(out, 0, sizeof *out);
	if (opt) o = *opt; else bmh_bam_post_opt_default(&o);
	int rc = bsr_out_make(J, &o.sorted, 0, nullptr, nullptr, res, fn);
	if (rc != BMH_OK) return rc;
	if (!path || !sink || !out) { bmh_set_error("%s: null argument", fn); return BMH_EINVAL; }
	if (!o.batch_bytes) o.batch_bytes = BPO_BATCH_DEFAULT;
	if (o.batch_bytes > BPO_BATCH_MAX) { bmh_set_error("%s: batch_bytes %llu (at most 2^30; 0: 2^28)", fn, (unsigned long long)o.batch_bytes); return BMH_EINVAL; }
	collate = o.collate != 0; in.plain = collate;
	if (collate && !J.markdup) { bmh_set_error("%s: collate needs marking: templates by name over the whole file are formed where duplicates are marked", fn); return BMH_EINVAL; }
	if (o.libraries && !J.markdup) { bmh_set_error("%s: libraries need marking: the header's @RG lines say which templates may be duplicates of each other", fn); return BMH_EINVAL; }
	if (J.markdup) mo = *o.sorted.markdup;
	if (o.libraries && (mo.rg_ids || mo.rg_lib || mo.n_groups)) { bmh_set_error("%s: libraries come from the header's @RG lines or from the options' read groups, not both", fn); return BMH_EINVAL; }
	if ((rc = in.open(path, fn, conv)) != BMH_OK) return rc;
	const int n_ref = (int)in.names.size();
	for (const std::string &nm : in.names) name_ptr.push_back(nm.c_str());
	if (o.libraries) {
		if ((rc = bmh_bam_header_groups(fn, in.header.data(), in.header.size(), true, rg)) != BMH_OK) return rc;
		for (const std::string &id : rg.ids) rg_ids.push_back(id.c_str());
		mo.rg_ids = rg_ids.data(); mo.rg_lib = rg.lib.data(); mo.n_groups = (int32_t)rg_ids.size();
		o.sorted.markdup = &mo;
	}
	if ((rc = bsr_out_make(J, &o.sorted, n_ref, in.len.data(), name_ptr.data(), res, fn)) != BMH_OK) return rc;
	mode = (J.markdup ? (uint32_t)BPO_MARKDUP : 0u) | (J.coverage ? (uint32_t)BPO_COVERAGE : 0u);
	if (J.P.groups() && n_ref > (int)BDP_MAX_REF) { bmh_set_error("%s: %d references: with read groups a run holds at most 2^24 (the library takes the duplicate key's top byte)", fn, n_ref); return BMH_EINVAL; }
	return BMH_OK;
}

int bpo_run_t::header_members(std::string &members) const
{
	uint8_t *hdr = nullptr, *hm = nullptr; uint64_t hb = 0, hmb = 0;
	int rc = bmh_bam_header(in.header.c_str(), (int)in.names.size(), name_ptr.data(), in.len.data(), &hdr, &hb);
	if (rc != BMH_OK) return rc;
	rc = bmh_bgzf_deflate_host(hdr, hb, J.level, 0, &hm, &hmb);
	bmh_free(hdr);
	if (rc != BMH_OK) return rc;
	members.assign((const char *)hm, hmb); bmh_free(hm);
	return BMH_OK;
}

static char *blob_of(const std::vector<std::string> &v)
{
	size_t n = 1;
	for (const std::string &s : v) n += s.size() + 1;
	char *b = (char *)malloc(n), *p = b;
	if (!b) return nullptr;
	for (const std::string &s : v) { memcpy(p, s.c_str(), s.size() + 1); p += s.size() + 1; }
	*p = 0;
	return b;
}

int bpo_run_t::finish(const std::string &index_bytes, bmh_bam_post_result_t *out) const
{
	bmh_bam_post_result_t r; memset(&r, 0, sizeof r);
	r.index = (uint8_t *)malloc(index_bytes.size() + 1); r.header_text = (char *)malloc(in.header.size() + 1);
	r.contig_names = blob_of(in.names); r.contig_len = (int32_t *)malloc(4 * in.len.size() + 4); r.library_names = blob_of(rg.lib_names);
	if (!r.index || !r.header_text || !r.contig_names || !r.contig_len || !r.library_names) { bmh_bam_post_result_free(&r); bmh_set_error("%s: out of memory", fn); return BMH_ENOMEM; }
	memcpy(r.index, index_bytes.data(), index_bytes.size()); r.index_bytes = index_bytes.size();
	memcpy(r.header_text, in.header.c_str(), in.header.size() + 1); r.header_bytes = in.header.size();
	r.n_contigs = (int32_t)in.names.size();
	if (!in.len.empty()) memcpy(r.contig_len, in.len.data(), 4 * in.len.size());
	r.n_libraries = (int32_t)rg.lib_names.size();
	r.counts = counts;
	*out = r;
	return BMH_OK;
}

int bpo_run_t::end(int rc, uint64_t base, bmh_sam_sink_t sink, void *user, bmh_bam_post_result_t *out, bmh_sorted_results_t *res)
{
	std::string ib;
	if (rc == BMH_OK && sink(user, (const char *)bmh_bgzf_eof, 28) != 0) { bmh_set_error("the sink refused the text"); rc = BMH_EINVAL; }
	if (rc == BMH_OK) rc = J.ix.bytes(base, ib);
	if (rc == BMH_OK) rc = bsr_out_export(J, res, fn);
	if (rc == BMH_OK) rc = finish(ib, out);
	if (rc != BMH_OK) bsr_results_release(res);
	return rc;
}

// ---------------------------------------------------------------------------------------------------------------- the host form

static int convert_host(const char *text, size_t n, int n_contigs, const std::string &blob, const std::vector<uint32_t> &noff, std::vector<uint8_t> &recs, uint32_t *bad, uint32_t *status)
{
	uint8_t *bam = nullptr; uint64_t bb = 0; uint32_t *st = nullptr, nrec = 0;
	const int rc = bmh_sam_to_bam_host(text, n, n_contigs, blob.data(), noff.data(), 0, &bam, &bb, &st, &nrec);
	if (rc != BMH_OK) return rc;
	*bad = ~0u;
	for (uint32_t r = 0; r < nrec; ++r) if (st[r]) { *bad = r; *status = st[r]; break; }
	if (*bad == ~0u) recs.assign(bam, bam + bb);
	bmh_free(bam); bmh_free(st);
	return BMH_OK;
}

namespace {
struct host_state_t {
	std::vector<uint8_t> recs; std::vector<uint64_t> off = std::vector<uint64_t>(1, 0);
	std::vector<uint32_t> tpl; std::vector<bdp_entry_t> E; std::vector<bdp_loc_t> locs; std::vector<uint64_t> bcs; uint64_t info[2] = {0, 0};
	btp_parts_t parts;                                                  // BDP_TPL_FILE: every record's part, until the grouping behind the last batch
};

int host_batch(bpo_run_t &R, host_state_t &S)
{
	bpo_input_t &in = R.in;
	uint8_t *recs = in.buf.data(); const uint64_t *off = in.off.data(); const uint32_t n = in.n;
	const int n_ref = (int)in.names.size();
	uint32_t bad = n; int code = BPO_OK;
	for (uint32_t i = 0; i < n; ++i) {
		uint32_t ch = 0;
		const int st = bpo_fix(recs + off[i], off[i + 1] - off[i], n_ref, R.mode, &ch);
		if (st != BPO_OK) { bad = i; code = st; break; }
		R.counts.bins_changed += ch & 1u; R.counts.dup_flags_cleared += ch >> 1;
		if (bpo_head(recs, off, i)) ++R.counts.templates;
	}
	// a refused record: the templates before the one that holds it are whole, and a refusal among them comes first
	const uint32_t n_ok = code == BPO_OK ? n : R.collate ? 0 : bpo_template_start(recs, off, bad);
	if (R.collate && code == BPO_OK) for (uint32_t i = 0; i < n; ++i) btp_append_host(S.parts, recs + off[i], off[i + 1] - off[i], R.J.P, 128);
	if (R.J.markdup && n_ok && !R.collate) {
		std::vector<uint32_t> tpl; std::vector<bdp_entry_t> E; std::vector<bdp_loc_t> locs; std::vector<uint64_t> bcs;
		const bool optical = R.J.P.optical() != nullptr, barcode = R.J.P.barcode() != nullptr;
		const int rc = bdp_entries_host(recs, off, n_ok, tpl, E, S.info, R.fn, R.J.P, optical ? &locs : nullptr, barcode ? &bcs : nullptr, BDP_TPL_NAME, in.base);
		if (rc != BMH_OK) return rc;
		const uint32_t tbase = (uint32_t)S.E.size();
		for (uint32_t t : tpl) S.tpl.push_back(tbase + t);
		S.E.insert(S.E.end(), E.begin(), E.end()); S.locs.insert(S.locs.end(), locs.begin(), locs.end()); S.bcs.insert(S.bcs.end(), bcs.begin(), bcs.end());
	}
	if (code != BPO_OK) return bpo_refused(R.fn, in.base + bad, code, recs + off[bad], off[bad + 1] - off[bad], n_ref);
	const uint64_t at = S.recs.size();
	S.recs.insert(S.recs.end(), recs, recs + off[n]);
	for (uint32_t i = 1; i <= n; ++i) S.off.push_back(at + off[i]);
	R.counts.records += n; ++R.counts.batches;
	return BMH_OK;
}
}   // namespace

// every batch checked and kept, the duplicates decided and flagged, the records sorted and written: everything of the host form before bpo_run_t::end
static int post_host(bpo_run_t &R, bmh_sam_sink_t sink, void *user, uint64_t *base)
{
	const char *fn = R.fn;
	int rc;
	host_state_t S;
	while ((rc = R.in.next(R.o.batch_bytes, fn)) == 1) if ((rc = host_batch(R, S)) != BMH_OK) return rc;
	if (rc < 0) return rc;
	if (S.off.size() > 0xfffffff0ull) { bmh_set_error("%s: 2^32 records", fn); return BMH_EINVAL; }
	const uint32_t n = (uint32_t)(S.off.size() - 1);
	uint8_t *recs = S.recs.data();
	if (R.J.markdup) {                                               // the decision over every template of the file, the flags set before the sort
		const bdp_plan_t &P = R.J.P; uint64_t *counts = R.J.dup_counts;
		const bool barcode = P.barcode() != nullptr;
		std::vector<uint32_t> bits; std::vector<uint64_t> Bp;
		if (R.collate) {                                           // the templates of the whole file by name, from the records' parts
			btp_result_t G;
			if ((rc = btp_group_host(S.parts, P, G, fn)) != BMH_OK) return rc;
			if (G.word != BPO_NONE) return btp_refused(S.parts, G.word, P, R.sam_line0(), fn);
			S.tpl.swap(G.rec_tpl); S.E.swap(G.E); S.locs.swap(G.locs); S.bcs.swap(G.bcs); S.info[0] = G.info[0]; S.info[1] = G.info[1];
			R.counts.templates = S.E.size();
		}
		if (S.E.size() >= 1ull << 31) { bmh_set_error("%s: duplicate marking: 2^31 templates", fn); return BMH_EINVAL; }
		if (P.no_barcode) *P.no_barcode = barcode ? bdp_no_barcode(S.bcs.data(), S.bcs.size()) : 0;
		bdp_decide_host(S.E.data(), S.E.size(), bits, counts, P, barcode ? S.bcs.data() : nullptr, &Bp);
		counts[BDP_SECSUP] = S.info[0]; counts[BDP_UNMAPPED] = S.info[1]; counts[BDP_TEMPLATES] = S.E.size();
		if (P.optical()) bdp_optical_host(S.E.data(), S.locs.data(), S.E.size(), *P.optical(), P.n_lib(), P.grouping() ? Bp.data() : barcode ? S.bcs.data() : nullptr);
		if (P.groups() && P.lib_counts) bdp_lib_tally_host(recs, S.off.data(), n, S.tpl.data(), S.E.data(), S.E.size(), P.n_lib(), P.lib_counts);
		for (uint32_t i = 0; i < n; ++i) if (bits[S.tpl[i] >> 5] >> (S.tpl[i] & 31) & 1u) recs[S.off[i] + 19] |= 0x04;
	}
	std::vector<uint64_t> keys; std::vector<uint32_t> ord;
	bsr_sort_host(recs, S.off, keys, ord);
	std::string members;
	if ((rc = R.header_members(members)) != BMH_OK) return rc;
	if (sink(user, members.data(), members.size()) != 0) { bmh_set_error("the sink refused the text"); return BMH_EINVAL; }
	*base = members.size();
	return bsr_write_host(recs, S.off.data(), ord.data(), n, R.J, sink, user, fn);
}

extern "C" int bmh_bam_post_file_host(const char *path, const bmh_bam_post_opt_t *opt, bmh_sam_sink_t sink, void *user, bmh_bam_post_result_t *out, bmh_sorted_results_t *res)
{
	const char *fn = "bmh_bam_post_file_host";
	bpo_run_t R; uint64_t base = 0;
	int rc;
	try {
		rc = R.begin(path, opt, sink, out, res, fn, convert_host);
		if (rc == BMH_OK) rc = post_host(R, sink, user, &base);
	} catch (const std::bad_alloc &) { bmh_set_error("%s: out of memory", fn); rc = BMH_ENOMEM; }
	return R.end(rc, base, sink, user, out, res);
}
