// Sorted BAM output on the host: the walk over a record stream, the host form of the sort (std::stable_sort), the index pass over a window and the .bai or .csi
// bytes (csrc/bam_sort_core.h's rules), the run store of csrc/align_pipeline.hip, the checked record of a sorted output, and bmh_bam_sort_host /
// bmh_bam_sorted_file_host.
#include <errno.h>
#include <fcntl.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <algorithm>
#include <map>
#include <new>
#include <numeric>
#include "bam_sort.h"
#include "bam_dup.h"
#include "bam_cov.h"
#include "bam_stats.h"

#ifndef O_TMPFILE
#define O_TMPFILE 0
#endif

int bsr_walk(const uint8_t *recs, uint64_t n_bytes, int n_ref, std::vector<uint64_t> &off, const char *fn)
{
	off.clear(); off.push_back(0);
	for (uint64_t p = 0; p < n_bytes;) {
		const uint64_t sz = bsr_record_bytes(recs + p, n_bytes - p);
		if (!sz) { bmh_set_error("%s: the bytes at %llu begin no whole BAM record (the stream is cut, or is no record stream)", fn, (unsigned long long)p); return BMH_EINVAL; }
		const int32_t r = bsr_ref(recs + p);
		if (r < -1 || (n_ref >= 0 && r >= n_ref)) { bmh_set_error("%s: record %zu names reference %d of %d", fn, off.size() - 1, r, n_ref); return BMH_EINVAL; }
		p += sz; off.push_back(p);
		if (off.size() > 0xfffffff0ull) { bmh_set_error("%s: 2^32 records", fn); return BMH_EINVAL; }
	}
	return BMH_OK;
}

void bsr_sort_host(const uint8_t *recs, const std::vector<uint64_t> &off, std::vector<uint64_t> &keys, std::vector<uint32_t> &ord)
{
	const size_t n = off.size() - 1;
	std::vector<uint64_t> k(n);
	for (size_t i = 0; i < n; ++i) k[i] = bsr_key(recs + off[i]);
	ord.resize(n); std::iota(ord.begin(), ord.end(), 0u);
	std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return k[a] < k[b]; });
	keys.resize(n);
	for (size_t j = 0; j < n; ++j) keys[j] = k[ord[j]];
}

int bsr_index_format_check(int format, int min_shift, const char *fn)
{
	if (format != BSR_IX_BAI && format != BSR_IX_CSI) { bmh_set_error("%s: index format %d (BMH_INDEX_BAI or BMH_INDEX_CSI)", fn, format); return BMH_EINVAL; }
	if (format == BSR_IX_CSI && (min_shift < BSR_CSI_SHIFT_MIN || min_shift > BSR_CSI_SHIFT_MAX)) {
		bmh_set_error("%s: a CSI index takes a min_shift of %d .. %d (14 is BAI's), not %d", fn, BSR_CSI_SHIFT_MIN, BSR_CSI_SHIFT_MAX, min_shift); return BMH_EINVAL;
	}
	return BMH_OK;                                        // (BAI: min_shift is not read, it is 14)
}

extern "C" void bmh_sorted_opt_default(bmh_sorted_opt_t *o)
{
	if (!o) return;
	memset(o, 0, sizeof *o);
	o->level = 1; o->index_format = BSR_IX_BAI; o->min_shift = BSR_LIN_SHIFT;
}

uint32_t bsr_out_t::parts() const
{
	return (markdup ? BMH_SORTED_MARKDUP | (P.optical() ? BMH_SORTED_OPTICAL : 0u) | (P.barcode() ? BMH_SORTED_BARCODE : 0u) | (P.grouping() ? BMH_SORTED_GROUPED : 0u) : 0u) |
	       (coverage ? BMH_SORTED_COVERAGE : 0u) | (stats ? BMH_SORTED_STATS : 0u) | (recal || requal ? BMH_SORTED_RECAL : 0u);
}

int bsr_out_make(bsr_out_t &J, const bmh_sorted_opt_t *opt, int n_contigs, const int32_t *contig_len, const char *const *contig_names, bmh_sorted_results_t *res, const char *fn)
{
	bmh_sorted_results_t none; memset(&none, 0, sizeof none);
	if (!res) res = &none;
	bmh_sorted_opt_t o;
	if (opt) o = *opt; else bmh_sorted_opt_default(&o);
	// (the results' last members came with the recalibration table: a caller who does not ask for it may not have set them, so they are read with the option only)
	bmh_markdup_counts_t *const mc = res->markdup; bmh_coverage_t *const cov = res->coverage; bmh_bam_stats_t *const st = res->stats; bmh_recal_t *const rt = o.recal ? res->recal : nullptr;
	memset(res, 0, sizeof *res); res->markdup = mc; res->coverage = cov; res->stats = st; res->recal = rt;
	if (rt) memset(rt, 0, o.recal->apply ? sizeof *rt : BRC_RECAL_OLD_BYTES);      // (the apply step's members exist for the caller who sets `apply`)
	if (cov) memset(cov, 0, sizeof *cov);
	if (st) memset(st, 0, sizeof *st);
	J = bsr_out_t();
	if (o.level != 0 && o.level != 1) { bmh_set_error("%s: level %d (0 or 1)", fn, o.level); return BMH_EINVAL; }
	J.level = o.level; J.window = o.window;
	int rc = J.ix.init(n_contigs, contig_len, fn, o.index_format, o.min_shift);
	if (rc != BMH_OK) return rc;
	if (o.markdup) {
		if (!mc) { bmh_set_error("%s: null argument (marking needs its counts record)", fn); return BMH_EINVAL; }
		if ((rc = bdp_plan_make(J.P, o.markdup, mc, fn)) != BMH_OK || (rc = bsr_markdup_contigs(n_contigs, contig_len, contig_names, fn)) != BMH_OK) return rc;
		J.markdup = true; J.dup_counts = mc->counts;
	}
	if (o.coverage) {
		if (!cov) { bmh_set_error("%s: null argument (coverage needs its record)", fn); return BMH_EINVAL; }
		if ((rc = bcv_plan_make(J.CP, o.coverage->min_mapq, o.coverage->deletions, o.coverage->bin, o.coverage->tile, n_contigs, contig_len, fn)) != BMH_OK) return rc;
		J.coverage = true;
	}
	if (o.stats) {
		if (!st) { bmh_set_error("%s: null argument (the statistics need their record)", fn); return BMH_EINVAL; }
		if ((rc = bst_plan_make(J.SP, o.stats->insert_cap, n_contigs, fn)) != BMH_OK) return rc;
		J.stats = true;
	}
	if (o.recal) {
		if (!rt) { bmh_set_error("%s: null argument (the recalibration table needs its record)", fn); return BMH_EINVAL; }
		const bmh_recal_apply_opt_t *const ap = o.recal->apply;
		if (!(ap && o.recal->no_count)) {
			if ((rc = brc_run_from_opt(J.RU, o.recal, n_contigs, contig_len, false, fn)) != BMH_OK) return rc;
			J.recal = true;
		}
		if (ap) {
			if ((rc = brq_run_from_opt(J.QU, ap, fn)) != BMH_OK) return rc;
			J.requal = true;
		}
	}
	return BMH_OK;
}

void bsr_results_release(bmh_sorted_results_t *res)
{
	if (res && res->stats) bmh_bam_stats_free(res->stats);
	if (res && res->recal) brc_release(res->recal);
	if (bmh_coverage_t *c = res ? res->coverage : nullptr) {
		bmh_free(c->n_reads); bmh_free(c->cov_bases); bmh_free(c->sum_depth); bmh_free(c->max_depth); bmh_free(c->sum_mapq); bmh_free(c->hist); bmh_free(c->bin_sum);
		memset(c, 0, sizeof *c);
	}
}

int bsr_out_export(const bsr_out_t &J, bmh_sorted_results_t *res, const char *fn)
{
	if (!res) return BMH_OK;
	res->parts = J.parts(); res->n_libraries = J.markdup ? (int32_t)J.P.n_lib() : 0;
	res->markdup_ms[0] = J.dup_ms[0]; res->markdup_ms[1] = J.dup_ms[1]; res->markdup_d2h_bytes = (uint64_t)J.dup_ms[2]; res->optical_ms = J.opt_ms;
	res->coverage_ms = J.cov_ms[0]; res->coverage_windows = (uint64_t)J.cov_ms[1]; res->stats_ms = J.stats_ms[0]; res->stats_windows = (uint64_t)J.stats_ms[1];
	res->recal_ms = J.recal_ms[0]; res->recal_windows = (uint64_t)J.recal_ms[1];
	int rc = BMH_OK;
	if (J.coverage && res->coverage) rc = bcv_export(J.CP, J.CR, res->coverage, fn);
	if (rc == BMH_OK && J.stats && res->stats) rc = bst_export(J.SP, J.SR, res->stats, fn);
	if (rc == BMH_OK && (J.recal || J.requal) && res->recal) rc = brc_export(J.recal ? &J.RU : nullptr, J.recal ? &J.RR : nullptr, res->recal, fn, J.requal ? &J.QR : nullptr, J.requal_ms);
	if (rc != BMH_OK) bsr_results_release(res);
	return rc;
}

int bsr_markdup_contigs(int n_contigs, const int32_t *contig_len, const char *const *contig_names, const char *fn)
{
	for (int c = 0; c < n_contigs; ++c)
		if (contig_len[c] > BDP_MAX_CONTIG) {
			bmh_set_error("%s: contig %d (%s) has %lld bases: duplicates are marked on contigs of at most 2^30 - 2^24 bases (the duplicate key holds an unclipped end in 31 bits); sort without marking",
			              fn, c, contig_names && contig_names[c] ? contig_names[c] : "?", (long long)contig_len[c]);
			return BMH_EINVAL;
		}
	return BMH_OK;
}

int bsr_index_t::init(int n_contigs, const int32_t *contig_len, const char *fn, int fmt, int shift)
{
	n_ref = n_contigs; n_win.clear(); lin_off.assign(1, 0); heads.clear(); file_pos = 0;
	const int rc = bsr_index_format_check(fmt, shift, fn);
	if (rc != BMH_OK) return rc;
	format = fmt; min_shift = fmt == BSR_IX_CSI ? shift : (int)BSR_LIN_SHIFT; depth = BSR_BAI_DEPTH;
	int64_t longest = 0;
	for (int c = 0; c < n_contigs; ++c) {
		if (fmt == BSR_IX_BAI && (contig_len[c] < 0 || contig_len[c] >= BSR_MAX_CONTIG)) {
			bmh_set_error("%s: contig %d has %lld bases: a BAI index holds contigs below 2^29 bases (CSI is not written)", fn, c, (long long)(uint32_t)contig_len[c]); return BMH_EINVAL;
		}
		if (contig_len[c] < 0) { bmh_set_error("%s: contig %d has %lld bases: BAM and its CSI index hold contigs of at most 2^31 - 1", fn, c, (long long)(uint32_t)contig_len[c]); return BMH_EINVAL; }
		if (contig_len[c] > longest) longest = contig_len[c];
		n_win.push_back(bsr_n_windows_at(contig_len[c], min_shift)); lin_off.push_back(lin_off.back() + n_win.back());
	}
	if (fmt == BSR_IX_CSI) depth = bsr_csi_depth(longest, min_shift);
	// (8 bytes a window, on the host and on the device: counted before either allocates)
	if (lin_off.back() >= 1ull << 28) {
		bmh_set_error("%s: the index would hold %llu windows of 2^%d bases (%llu bytes; at most 2^28 windows): choose a larger min_shift", fn, (unsigned long long)lin_off.back(), min_shift,
		              8ull * (unsigned long long)lin_off.back());
		return BMH_EINVAL;
	}
	try { lin.assign(lin_off.back() + 1, ~0ull); counts.assign(2 * (size_t)n_ref + 1, 0); }
	catch (const std::bad_alloc &) { bmh_set_error("%s: out of memory for %llu index windows", fn, (unsigned long long)lin_off.back()); return BMH_ENOMEM; }
	return BMH_OK;
}

void bsr_index_t::window_host(const uint8_t *recs, const uint64_t *soff, uint32_t n, const uint64_t *moff)
{
	const uint64_t total = soff[n];
	const bool csi = format == BSR_IX_CSI;
	for (uint32_t j = 0; j < n; ++j) {
		const uint8_t *rec = recs + soff[j], *prev = j ? recs + soff[j - 1] : nullptr;
		const uint64_t v = bsr_voff(file_pos, moff, total, soff[j]);
		const int32_t r = bsr_ref(rec);
		const uint32_t nw = r >= 0 && r < n_ref ? n_win[r] : 1u;
		if (csi) { if (bsr_csi_chunk_head(rec, prev, nw, min_shift, depth)) heads.push_back({r < 0 ? -1 : r, bsr_csi_rec_bin(rec, nw, min_shift, depth), v}); }
		else if (bsr_chunk_head(rec, prev)) heads.push_back({r < 0 ? -1 : r, bsr_bin(rec), v});
		if (r < 0 || r >= n_ref) { ++counts[2 * (size_t)n_ref]; continue; }
		++counts[2 * (size_t)r + ((bsr_flag(rec) & 4u) ? 1 : 0)];
		uint32_t lo, hi;
		bsr_windows_at(rec, n_win[r], min_shift, &lo, &hi);
		for (uint32_t w = lo; w <= hi; ++w) { uint64_t &s = lin[lin_off[r] + w]; if (v < s) s = v; }
	}
	file_pos += moff[(total + BSR_PIECE - 1) / BSR_PIECE];
}

namespace {
// a reference's chunks by bin, and the span of its records
struct ix_ref_t { std::map<uint32_t, std::vector<std::pair<uint64_t, uint64_t>>> bins; uint64_t beg = 0, end = 0; bool any = false; };
// chunks: heads that continue the chunk before them (a window's first record) are dropped; a chunk ends where the next begins
std::vector<ix_ref_t> ix_chunks(const bsr_index_t &ix, uint64_t sh)
{
	std::vector<ix_ref_t> refs((size_t)ix.n_ref);
	std::vector<bsr_head_t> hs;
	for (const bsr_head_t &h : ix.heads)
		if (hs.empty() || hs.back().ref != h.ref || (h.ref >= 0 && hs.back().bin != h.bin)) hs.push_back(h);
	for (size_t i = 0; i < hs.size(); ++i) {
		if (hs[i].ref < 0 || hs[i].ref >= ix.n_ref) continue;
		const uint64_t b = hs[i].beg + sh, e = (i + 1 < hs.size() ? hs[i + 1].beg : ix.file_pos << 16) + sh;
		ix_ref_t &R = refs[(size_t)hs[i].ref];
		R.bins[hs[i].bin].push_back({b, e});
		if (!R.any) { R.any = true; R.beg = b; }
		R.end = e;
	}
	return refs;
}
}   // namespace

void bsr_index_t::bai(uint64_t base_offset, std::string &out) const
{
	const uint64_t sh = base_offset << 16;
	auto u32 = [&](uint32_t v) { for (int k = 0; k < 4; ++k) out.push_back((char)(v >> (8 * k))); };
	auto u64 = [&](uint64_t v) { for (int k = 0; k < 8; ++k) out.push_back((char)(v >> (8 * k))); };
	typedef ix_ref_t ref_t;
	const std::vector<ref_t> refs = ix_chunks(*this, sh);
	out.clear();
	out += "BAI\1"; u32((uint32_t)n_ref);
	for (int r = 0; r < n_ref; ++r) {
		const ref_t &R = refs[(size_t)r];
		if (!R.any) { u32(0); u32(0); continue; }
		u32((uint32_t)R.bins.size() + 1);
		for (const auto &kv : R.bins) {
			u32(kv.first); u32((uint32_t)kv.second.size());
			for (const auto &c : kv.second) { u64(c.first); u64(c.second); }
		}
		u32(BSR_META_BIN); u32(2); u64(R.beg); u64(R.end); u64(counts[2 * (size_t)r]); u64(counts[2 * (size_t)r + 1]);
		uint32_t n_intv = 0;
		for (uint32_t w = 0; w < n_win[r]; ++w) if (lin[lin_off[r] + w] != ~0ull) n_intv = w + 1;
		u32(n_intv);
		uint64_t last = 0;
		for (uint32_t w = 0; w < n_intv; ++w) { const uint64_t v = lin[lin_off[r] + w]; if (v != ~0ull) last = v + sh; u64(last); }
	}
	u64(counts[2 * (size_t)n_ref]);
}

// "CSI\1" min_shift depth l_aux = 0 n_ref | per reference: n_bin, per bin (ascending, the pseudo-bin last): bin loffset n_chunk chunks | n_no_coor -- all of it
// as BGZF members and the end-of-file member.  A bin's loffset is the linear value at its first window, a window without records taking that of the next window
// that has some (htslib's back-fill; bai() above fills its holes forward): a lower bound on the first record that overlaps anything from the bin's start on
int bsr_index_t::csi(uint64_t base_offset, std::string &out) const
{
	const uint64_t sh = base_offset << 16;
	std::string raw;
	auto u32 = [&](uint32_t v) { for (int k = 0; k < 4; ++k) raw.push_back((char)(v >> (8 * k))); };
	auto u64 = [&](uint64_t v) { for (int k = 0; k < 8; ++k) raw.push_back((char)(v >> (8 * k))); };
	const std::vector<ix_ref_t> refs = ix_chunks(*this, sh);
	raw += "CSI\1"; u32((uint32_t)min_shift); u32((uint32_t)depth); u32(0); u32((uint32_t)n_ref);
	std::vector<uint64_t> fill;
	for (int r = 0; r < n_ref; ++r) {
		const ix_ref_t &R = refs[(size_t)r];
		if (!R.any) { u32(0); continue; }
		fill.assign((size_t)n_win[r] + 1, ~0ull);
		for (uint32_t w = n_win[r]; w-- > 0;) { const uint64_t v = lin[lin_off[r] + w]; fill[w] = v != ~0ull ? v + sh : fill[w + 1]; }
		u32((uint32_t)R.bins.size() + 1);
		for (const auto &kv : R.bins) {
			int l = 0;
			while (l < depth && kv.first < bsr_csi_level_first(depth, l)) ++l;
			const uint64_t w0 = (uint64_t)(kv.first - bsr_csi_level_first(depth, l)) << (3 * l);
			const uint64_t lo = w0 < n_win[r] ? fill[(size_t)w0] : ~0ull;
			u32(kv.first); u64(lo != ~0ull ? lo : 0); u32((uint32_t)kv.second.size());
			for (const auto &c : kv.second) { u64(c.first); u64(c.second); }
		}
		u32(bsr_csi_meta_bin(depth)); u64(0); u32(2); u64(R.beg); u64(R.end); u64(counts[2 * (size_t)r]); u64(counts[2 * (size_t)r + 1]);
	}
	u64(counts[2 * (size_t)n_ref]);
	uint8_t *m = nullptr; uint64_t mb = 0;
	const int rc = bmh_bgzf_deflate_host((const uint8_t *)raw.data(), raw.size(), 1, 0, &m, &mb);
	if (rc != BMH_OK) return rc;
	out.assign((const char *)m, mb); bmh_free(m);
	out.append((const char *)bmh_bgzf_eof, 28);
	return BMH_OK;
}

// ---------------------------------------------------------------------------------------------------------------- the run store

void bsr_store_t::clear()
{
	for (bsr_run_t &r : runs) free(r.mem);
	runs.clear(); used = 0; spilled = 0; file_bytes = 0;
	entries.clear(); locs.clear(); bcs.clear(); dup_info[0] = dup_info[1] = 0; lib_info.clear(); tpl_parts.clear();
	if (fd >= 0) close(fd);
	fd = -1;
}

int bsr_store_t::append(const uint8_t *recs, uint64_t bytes, const uint64_t *keys, const uint64_t *off, uint64_t n, const bsr_dup_t *dup)
{
	bsr_run_t r;
	r.n = n; r.bytes = bytes; r.keys.assign(keys, keys + n); r.off.assign(off, off + n + 1);
	if (dup) { r.tpl.assign(dup->tpl, dup->tpl + n); r.tbase = entries.size(); }
	if (bytes <= mem_bytes - std::min(used, mem_bytes)) {
		r.mem = (uint8_t *)malloc(bytes + 1);
		if (!r.mem) { bmh_set_error("sorted BAM: out of memory for a run of %llu bytes", (unsigned long long)bytes); return BMH_ENOMEM; }
		memcpy(r.mem, recs, bytes); used += bytes;
	} else {
		if (fd < 0) {                                     // an unnamed file: nothing to remove, whatever ends the run
			const char *env = getenv("TMPDIR");
			const std::string dir = !tmp_dir.empty() ? tmp_dir : (env && env[0] ? env : "/tmp");
			if (O_TMPFILE) fd = open(dir.c_str(), O_TMPFILE | O_RDWR | O_CLOEXEC, 0600);
			if (fd < 0) {
				std::string t = dir + "/bmh_sort_XXXXXX";
				fd = mkstemp(&t[0]);
				if (fd >= 0) (void)unlink(t.c_str());
			}
			if (fd < 0) { bmh_set_error("sorted BAM: cannot create a temporary file in %s: %s", dir.c_str(), strerror(errno)); return BMH_EINVAL; }
		}
		for (uint64_t p = 0; p < bytes;) {
			const ssize_t w = pwrite(fd, recs + p, (size_t)std::min<uint64_t>(bytes - p, 1u << 30), (off_t)(file_bytes + p));
			if (w <= 0) {
				if (w < 0 && errno == EINTR) continue;
				bmh_set_error("sorted BAM: writing a run of %llu bytes to the temporary file: %s", (unsigned long long)bytes, w < 0 ? strerror(errno) : "nothing was written (no space left?)");
				return BMH_EINVAL;
			}
			p += (uint64_t)w;
		}
		r.file_at = (int64_t)file_bytes; file_bytes += bytes; ++spilled;
	}
	if (dup && dup->locs) locs.insert(locs.end(), dup->locs, dup->locs + dup->n_tpl);
	if (dup && dup->bcs) bcs.insert(bcs.end(), dup->bcs, dup->bcs + dup->n_tpl);
	if (dup) { entries.insert(entries.end(), dup->entries, dup->entries + dup->n_tpl); dup_info[0] += dup->secsup; dup_info[1] += dup->unmapped; }
	if (dup && dup->lib >= 0) {
		if (lib_info.size() < 3 * ((size_t)dup->lib + 1)) lib_info.resize(3 * ((size_t)dup->lib + 1), 0);
		uint64_t *c = &lib_info[3 * (size_t)dup->lib];
		c[0] += dup->secsup; c[1] += dup->unmapped; c[2] += dup->n_tpl;
	}
	if (dup && dup->lib < 0 && dup->lib3) {                // a batch of several libraries: its own per-library counts
		if (lib_info.size() < 3 * (size_t)dup->n_lib3) lib_info.resize(3 * (size_t)dup->n_lib3, 0);
		for (size_t k = 0; k < 3 * (size_t)dup->n_lib3; ++k) lib_info[k] += dup->lib3[k];
	}
	runs.push_back(std::move(r));
	return BMH_OK;
}

void bsr_store_t::retemplate(const std::vector<uint32_t> &rec_tpl)
{
	for (bsr_run_t &r : runs) {
		for (uint32_t &t : r.tpl) t = rec_tpl[(size_t)(r.tbase + t)];
		r.tbase = 0;
	}
}

int bsr_store_t::read(const bsr_run_t &r, uint64_t a, uint64_t b, uint8_t *dst) const
{
	if (r.mem) { memcpy(dst, r.mem + a, b - a); return BMH_OK; }
	for (uint64_t p = a; p < b;) {
		const ssize_t g = pread(fd, dst + (p - a), (size_t)std::min<uint64_t>(b - p, 1u << 30), (off_t)((uint64_t)r.file_at + p));
		if (g <= 0) { if (g < 0 && errno == EINTR) continue; bmh_set_error("sorted BAM: reading a run back from the temporary file: %s", g < 0 ? strerror(errno) : "it is shorter than what was written"); return BMH_EINVAL; }
		p += (uint64_t)g;
	}
	return BMH_OK;
}

// ---------------------------------------------------------------------------------------------------------------- the host entry points

extern "C" int bmh_bam_sort_host(const uint8_t *recs, uint64_t n_bytes, uint8_t **out)
{
	const char *fn = "bmh_bam_sort_host";
	if (!out || (n_bytes && !recs)) { bmh_set_error("%s: null argument", fn); return BMH_EINVAL; }
	*out = nullptr;
	std::vector<uint64_t> off, keys; std::vector<uint32_t> ord;
	const int rc = bsr_walk(recs, n_bytes, -1, off, fn);
	if (rc != BMH_OK) return rc;
	bsr_sort_host(recs, off, keys, ord);
	uint8_t *o = (uint8_t *)malloc(n_bytes + 1);
	if (!o) { bmh_set_error("%s: out of memory", fn); return BMH_ENOMEM; }
	uint64_t p = 0;
	for (uint32_t i : ord) { memcpy(o + p, recs + off[i], off[i + 1] - off[i]); p += off[i + 1] - off[i]; }
	*out = o;
	return BMH_OK;
}

int bsr_write_host(const uint8_t *recs, const uint64_t *off, const uint32_t *ord, uint64_t n, bsr_out_t &J, bsr_sink_t sink, void *user, const char *fn)
{
	bcv_host_t H; bst_host_t SH; brc_host_t RH; brq_host_t QH;
	if (J.coverage) H.begin(J.CP);
	if (J.stats) SH.begin(J.SP);
	if (J.recal) {
		if (!J.RU.pac && J.RU.l_pac) { bmh_set_error("%s: the recalibration table needs the reference (pac, l_pac)", fn); return BMH_EINVAL; }
		RH.begin(J.RU);
	}
	if (J.requal) QH.begin(J.QU);
	const uint64_t W = J.window ? J.window : std::max<uint64_t>(1, (64ull << 20) / std::max<uint64_t>(1, n ? off[n] / n : 1));
	std::vector<uint8_t> buf; std::vector<uint64_t> soff, moff;
	int rc;
	for (uint64_t a = 0; a < n; a += W) {
		const uint64_t b = std::min<uint64_t>(n, a + W);
		soff.assign(1, 0); buf.clear();
		for (uint64_t j = a; j < b; ++j) { const uint64_t o = off[ord[j]], s = off[ord[j] + 1] - o; buf.insert(buf.end(), recs + o, recs + o + s); soff.push_back(buf.size()); }
		if (J.requal && (rc = QH.window(buf.data(), soff.data(), (uint32_t)(b - a), fn)) != BMH_OK) return rc;      // the qualities as they are written: everything below reads them so
		uint8_t *m = nullptr; uint64_t mb = 0;
		if ((rc = bmh_bgzf_deflate_host(buf.data(), buf.size(), J.level, 0, &m, &mb)) != BMH_OK) return rc;
		moff.assign(1, 0);                                // the members' offsets: every member's BSIZE
		for (uint64_t q = 0; q < mb;) { q += ((uint64_t)m[q + 16] | (uint64_t)m[q + 17] << 8) + 1; moff.push_back(q); }
		const int sr = sink(user, (const char *)m, (size_t)mb);
		bmh_free(m);
		if (sr != 0) { bmh_set_error("the sink refused the text"); return BMH_EINVAL; }
		J.ix.window_host(buf.data(), soff.data(), (uint32_t)(b - a), moff.data());
		if (J.coverage && (rc = H.window(buf.data(), soff.data(), (uint32_t)(b - a), fn)) != BMH_OK) return rc;      // the window in its final order, with its final flags
		if (J.stats && (rc = SH.window(buf.data(), soff.data(), (uint32_t)(b - a), fn)) != BMH_OK) return rc;
		if (J.recal && (rc = RH.window(buf.data(), soff.data(), (uint32_t)(b - a), fn)) != BMH_OK) return rc;
	}
	if (J.coverage) { if ((rc = H.finish(fn)) != BMH_OK) return rc; J.CR = std::move(H.R); }
	if (J.stats) { SH.finish(); J.SR = std::move(SH.R); }
	if (J.recal) { RH.finish(); J.RR = std::move(RH.R); }
	if (J.requal) J.QR = std::move(QH.R);
	return BMH_OK;
}

int bsr_file_t::begin(const char *f, const char *header_text, int n_contigs, const char *const *contig_names, const int32_t *contig_len, const uint8_t *recs, uint64_t n_bytes,
                      const bmh_sorted_opt_t *opt, uint8_t **bam_, uint64_t *bam_bytes_, uint8_t **index_, uint64_t *index_bytes_, bmh_sorted_results_t *res)
{
	fn = f; bam = bam_; bam_bytes = bam_bytes_; index = index_; index_bytes = index_bytes_;
	if (bam) *bam = nullptr;
	if (index) *index = nullptr;
	int rc = bsr_out_make(J, opt, n_contigs, contig_len, contig_names, res, fn);
	if (rc != BMH_OK) return rc;
	if (J.P.optical()) { bmh_set_error("%s: a stand-alone sorted file has no optical step: optical_distance stays -1 (bmh_bam_markdup_* counts optical duplicates)", fn); return BMH_EINVAL; }
	if (!header_text || !bam || !bam_bytes || !index || !index_bytes || (n_bytes && !recs)) { bmh_set_error("%s: null argument", fn); return BMH_EINVAL; }
	*bam_bytes = *index_bytes = 0;
	if (J.P.groups() && n_contigs > (int)BDP_MAX_REF) { bmh_set_error("%s: %d references: with read groups a run holds at most 2^24 (the library takes the duplicate key's top byte)", fn, n_contigs); return BMH_EINVAL; }
	if ((rc = bsr_walk(recs, n_bytes, n_contigs, off, fn)) != BMH_OK) return rc;
	uint8_t *hdr = nullptr, *hm = nullptr; uint64_t hb = 0, hmb = 0;
	if ((rc = bmh_bam_header(header_text, n_contigs, contig_names, contig_len, &hdr, &hb)) != BMH_OK) return rc;
	rc = bmh_bgzf_deflate_host(hdr, hb, J.level, 0, &hm, &hmb);
	bmh_free(hdr);
	if (rc != BMH_OK) return rc;
	file.assign((const char *)hm, hmb); bmh_free(hm);
	base = file.size();
	return BMH_OK;
}

int bsr_file_t::end(int rc, bmh_sorted_results_t *res)
{
	std::string ib;
	if (rc == BMH_OK) { file.append((const char *)bmh_bgzf_eof, 28); rc = J.ix.bytes(base, ib); }
	if (rc == BMH_OK) rc = bsr_out_export(J, res, fn);
	if (rc == BMH_OK) {
		uint8_t *f = (uint8_t *)malloc(file.size() + 1), *i = (uint8_t *)malloc(ib.size() + 1);
		if (!f || !i) { free(f); free(i); bmh_set_error("%s: out of memory", fn); rc = BMH_ENOMEM; }
		else { memcpy(f, file.data(), file.size()); memcpy(i, ib.data(), ib.size()); *bam = f; *bam_bytes = file.size(); *index = i; *index_bytes = ib.size(); }
	}
	if (rc != BMH_OK) bsr_results_release(res);
	return rc;
}

extern "C" int bmh_bam_sorted_file_host(const char *header_text, int n_contigs, const char *const *contig_names, const int32_t *contig_len, const uint8_t *recs, uint64_t n_bytes,
                                        const bmh_sorted_opt_t *opt, uint8_t **bam, uint64_t *bam_bytes, uint8_t **index, uint64_t *index_bytes, bmh_sorted_results_t *res)
{
	const char *fn = "bmh_bam_sorted_file_host";
	bsr_file_t F;
	int rc;
	try {
		rc = F.begin(fn, header_text, n_contigs, contig_names, contig_len, recs, n_bytes, opt, bam, bam_bytes, index, index_bytes, res);
		std::vector<uint8_t> marked;                               // duplicate marking: the flags are set before the sort (0x400 enters no key, bin or index)
		if (rc == BMH_OK && F.J.markdup) {
			marked.assign(recs, recs + n_bytes);
			rc = bdp_markdup_host(marked.data(), F.off, F.J.dup_counts, fn, F.J.P);
			recs = marked.data();
		}
		if (rc == BMH_OK) {
			std::vector<uint64_t> keys; std::vector<uint32_t> ord;
			bsr_sort_host(recs, F.off, keys, ord);
			rc = bsr_write_host(recs, F.off.data(), ord.data(), ord.size(), F.J, bsr_sink_string, &F.file, fn);
		}
	} catch (const std::bad_alloc &) { bmh_set_error("%s: out of memory", fn); rc = BMH_ENOMEM; }
	return F.end(rc, res);
}
