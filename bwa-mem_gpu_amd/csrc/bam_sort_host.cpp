// Sorted BAM output on the host: the walk over a record stream, the host form of the sort (std::stable_sort), the index pass over a window and the .bai or .csi
// bytes (csrc/bam_sort_core.h's rules), the run store of csrc/align_pipeline.hip, and bmh_bam_sort_host / bmh_bam_sorted_file_host / _ex_host.
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

int bsr_file_opt_check(const bmh_sorted_file_opt_t *opt, bmh_markdup_counts_t *res, const char *fn, bmh_sorted_file_opt_t &o, bdp_plan_t &P)
{
	o = opt ? *opt : bmh_sorted_file_opt_t{1, 0, BSR_IX_BAI, BSR_LIN_SHIFT, nullptr};
	int rc = bsr_index_format_check(o.index_format, o.min_shift, fn);
	if (rc != BMH_OK || !o.markdup) return rc;
	if (o.markdup->optical_distance != -1) { bmh_set_error("%s: a stand-alone sorted file has no optical step: optical_distance stays -1 (bmh_bam_markdup_* counts optical duplicates)", fn); return BMH_EINVAL; }
	return bdp_plan_make(P, o.markdup, res, fn);
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
	n_ref = n_contigs; n_win.clear(); lin_off.assign(1, 0); heads.clear(); file_pos = 0; valid = false;
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
	valid = true;
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

// header members, the sorted records in windows of `window` records (0: as many as hold about 64 MiB), the end-of-file member; and the index
static int sorted_file_host(const char *fn, const char *header_text, int n_contigs, const char *const *contig_names, const int32_t *contig_len, const uint8_t *recs, uint64_t n_bytes,
                            const bmh_sorted_file_opt_t &o, uint8_t **bam, uint64_t *bam_bytes, uint8_t **bai, uint64_t *bai_bytes, uint64_t *dup_counts, const bdp_plan_t &P,
                            bcv_host_t *cov = nullptr, bst_host_t *stats = nullptr)
{
	const int level = o.level; const uint32_t window = o.window;
	if (!header_text || !bam || !bam_bytes || !bai || !bai_bytes || (n_bytes && !recs)) { bmh_set_error("%s: null argument", fn); return BMH_EINVAL; }
	*bam = *bai = nullptr; *bam_bytes = *bai_bytes = 0;
	if (P.groups() && n_contigs > (int)BDP_MAX_REF) { bmh_set_error("%s: %d references: with read groups a run holds at most 2^24 (the library takes the duplicate key's top byte)", fn, n_contigs); return BMH_EINVAL; }
	bsr_index_t ix;
	int rc = ix.init(n_contigs, contig_len, fn, o.index_format, o.min_shift);
	if (rc != BMH_OK) return rc;
	if (dup_counts && (rc = bsr_markdup_contigs(n_contigs, contig_len, contig_names, fn)) != BMH_OK) return rc;
	std::vector<uint64_t> off, keys; std::vector<uint32_t> ord;
	if ((rc = bsr_walk(recs, n_bytes, n_contigs, off, fn)) != BMH_OK) return rc;
	std::vector<uint8_t> marked;                                   // duplicate marking: the flags are set before the sort (0x400 enters no key, bin or index)
	if (dup_counts) {
		marked.assign(recs, recs + n_bytes);
		if ((rc = bdp_markdup_host(marked.data(), off, dup_counts, fn, P)) != BMH_OK) return rc;
		recs = marked.data();
	}
	bsr_sort_host(recs, off, keys, ord);
	const size_t n = ord.size();
	std::string file;
	auto members = [&](const uint8_t *p, uint64_t nb, std::vector<uint64_t> *moff) {
		uint8_t *m = nullptr; uint64_t mb = 0;
		const int r = bmh_bgzf_deflate_host(p, nb, level, 0, &m, &mb);
		if (r != BMH_OK) return r;
		if (moff) {                                   // the members' offsets: every member's BSIZE
			moff->assign(1, 0);
			for (uint64_t q = 0; q < mb;) { q += ((uint64_t)m[q + 16] | (uint64_t)m[q + 17] << 8) + 1; moff->push_back(q); }
		}
		file.append((const char *)m, mb); bmh_free(m);
		return (int)BMH_OK;
	};
	uint8_t *hdr = nullptr; uint64_t hb = 0;
	if ((rc = bmh_bam_header(header_text, n_contigs, contig_names, contig_len, &hdr, &hb)) != BMH_OK) return rc;
	rc = members(hdr, hb, nullptr); bmh_free(hdr);
	if (rc != BMH_OK) return rc;
	const uint64_t base = file.size();
	const uint64_t W = window ? window : std::max<uint64_t>(1, (64ull << 20) / std::max<uint64_t>(1, n ? n_bytes / n : 1));
	std::vector<uint8_t> buf; std::vector<uint64_t> soff, moff;
	for (size_t a = 0; a < n; a += W) {
		const size_t b = std::min<uint64_t>(n, a + W);
		soff.assign(1, 0); buf.clear();
		for (size_t j = a; j < b; ++j) { const uint64_t o = off[ord[j]], s = off[ord[j] + 1] - o; buf.insert(buf.end(), recs + o, recs + o + s); soff.push_back(buf.size()); }
		if ((rc = members(buf.data(), buf.size(), &moff)) != BMH_OK) return rc;
		ix.window_host(buf.data(), soff.data(), (uint32_t)(b - a), moff.data());
		if (cov && (rc = cov->window(buf.data(), soff.data(), (uint32_t)(b - a), fn)) != BMH_OK) return rc;      // the window in its final order, with its final flags
		if (stats && (rc = stats->window(buf.data(), soff.data(), (uint32_t)(b - a), fn)) != BMH_OK) return rc;
	}
	if (cov && (rc = cov->finish(fn)) != BMH_OK) return rc;
	file.append((const char *)bmh_bgzf_eof, 28);
	std::string ib;
	if ((rc = ix.bytes(base, ib)) != BMH_OK) return rc;
	uint8_t *f = (uint8_t *)malloc(file.size() + 1), *i = (uint8_t *)malloc(ib.size() + 1);
	if (!f || !i) { free(f); free(i); bmh_set_error("%s: out of memory", fn); return BMH_ENOMEM; }
	memcpy(f, file.data(), file.size()); memcpy(i, ib.data(), ib.size());
	*bam = f; *bam_bytes = file.size(); *bai = i; *bai_bytes = ib.size();
	return BMH_OK;
}

extern "C" int bmh_bam_sorted_file_host(const char *header_text, int n_contigs, const char *const *contig_names, const int32_t *contig_len, const uint8_t *recs, uint64_t n_bytes,
                                        const bmh_sorted_file_opt_t *opt, uint8_t **bam, uint64_t *bam_bytes, uint8_t **index, uint64_t *index_bytes, bmh_markdup_counts_t *res)
{
	const char *fn = "bmh_bam_sorted_file_host";
	bmh_sorted_file_opt_t o; bdp_plan_t P;
	const int rc = bsr_file_opt_check(opt, res, fn, o, P);
	if (rc != BMH_OK) return rc;
	return sorted_file_host(fn, header_text, n_contigs, contig_names, contig_len, recs, n_bytes, o, bam, bam_bytes, index, index_bytes, o.markdup ? res->counts : nullptr, P);
}

// the sorted file and, from the same windows of the merge, its coverage (the host form of csrc/bam_cov_kernels.hip)
extern "C" int bmh_bam_sorted_file_coverage_host(const char *header_text, int n_contigs, const char *const *contig_names, const int32_t *contig_len, const uint8_t *recs, uint64_t n_bytes,
                                                 const bmh_sorted_file_opt_t *opt, const bmh_coverage_opt_t *cov_opt, uint8_t **bam, uint64_t *bam_bytes, uint8_t **index, uint64_t *index_bytes,
                                                 bmh_markdup_counts_t *res, bmh_coverage_t *cov)
{
	const char *fn = "bmh_bam_sorted_file_coverage_host";
	if (bam) *bam = nullptr;                                         // (before anything can be refused: a caller who frees what a failed call left frees nothing)
	if (index) *index = nullptr;
	if (!cov) { bmh_set_error("%s: null argument", fn); return BMH_EINVAL; }
	memset(cov, 0, sizeof *cov);
	bmh_sorted_file_opt_t o; bdp_plan_t P;
	int rc = bsr_file_opt_check(opt, res, fn, o, P);
	if (rc != BMH_OK) return rc;
	bmh_coverage_opt_t co; bmh_coverage_opt_default(&co);
	if (cov_opt) co = *cov_opt;
	bcv_plan_t CP;
	if ((rc = bcv_plan_make(CP, co.min_mapq, co.deletions, co.bin, co.tile, n_contigs, contig_len, fn)) != BMH_OK) return rc;
	try {
		bcv_host_t H; H.begin(CP);
		rc = sorted_file_host(fn, header_text, n_contigs, contig_names, contig_len, recs, n_bytes, o, bam, bam_bytes, index, index_bytes, o.markdup ? res->counts : nullptr, P, &H);
		if (rc == BMH_OK && (rc = bcv_export(CP, H.R, cov, fn)) != BMH_OK) {      // the one failure behind the file's bytes: they are the call's to release
			bmh_free(*bam); bmh_free(*index); *bam = *index = nullptr; *bam_bytes = *index_bytes = 0;
		}
	} catch (const std::bad_alloc &) { bmh_set_error("%s: out of memory", fn); rc = BMH_ENOMEM; }
	return rc;
}

// the sorted file and, from the same windows of the merge, its statistics and, with cov, its coverage (the host form of csrc/bam_stats_kernels.hip)
extern "C" int bmh_bam_sorted_file_stats_host(const char *header_text, int n_contigs, const char *const *contig_names, const int32_t *contig_len, const uint8_t *recs, uint64_t n_bytes,
                                              const bmh_sorted_file_opt_t *opt, const bmh_coverage_opt_t *cov_opt, const bmh_bam_stats_opt_t *stats_opt, uint8_t **bam, uint64_t *bam_bytes,
                                              uint8_t **index, uint64_t *index_bytes, bmh_markdup_counts_t *res, bmh_coverage_t *cov, bmh_bam_stats_t *stats)
{
	const char *fn = "bmh_bam_sorted_file_stats_host";
	if (bam) *bam = nullptr;                                         // (before anything can be refused: a caller who frees what a failed call left frees nothing)
	if (index) *index = nullptr;
	if (cov) memset(cov, 0, sizeof *cov);
	if (!stats) { bmh_set_error("%s: null argument", fn); return BMH_EINVAL; }
	memset(stats, 0, sizeof *stats);
	bmh_sorted_file_opt_t o; bdp_plan_t P;
	int rc = bsr_file_opt_check(opt, res, fn, o, P);
	if (rc != BMH_OK) return rc;
	bmh_bam_stats_opt_t so; bmh_bam_stats_opt_default(&so);
	if (stats_opt) so = *stats_opt;
	bst_plan_t SP;
	if ((rc = bst_plan_make(SP, so.insert_cap, n_contigs, fn)) != BMH_OK) return rc;
	bmh_coverage_opt_t co; bmh_coverage_opt_default(&co);
	if (cov_opt) co = *cov_opt;
	bcv_plan_t CP;
	if (cov && (rc = bcv_plan_make(CP, co.min_mapq, co.deletions, co.bin, co.tile, n_contigs, contig_len, fn)) != BMH_OK) return rc;
	try {
		bcv_host_t H; bst_host_t SH;
		if (cov) H.begin(CP);
		SH.begin(SP);
		rc = sorted_file_host(fn, header_text, n_contigs, contig_names, contig_len, recs, n_bytes, o, bam, bam_bytes, index, index_bytes, o.markdup ? res->counts : nullptr, P, cov ? &H : nullptr, &SH);
		if (rc == BMH_OK) {
			SH.finish();
			if (cov) rc = bcv_export(CP, H.R, cov, fn);
			if (rc == BMH_OK && (rc = bst_export(SP, SH.R, stats, fn)) != BMH_OK && cov) {
				bmh_free(cov->n_reads); bmh_free(cov->cov_bases); bmh_free(cov->sum_depth); bmh_free(cov->max_depth); bmh_free(cov->sum_mapq); bmh_free(cov->hist); bmh_free(cov->bin_sum);
				memset(cov, 0, sizeof *cov);
			}
			if (rc != BMH_OK) { bmh_free(*bam); bmh_free(*index); *bam = *index = nullptr; *bam_bytes = *index_bytes = 0; }      // the failures behind the file's bytes: they are the call's to release
		}
	} catch (const std::bad_alloc &) { bmh_set_error("%s: out of memory", fn); rc = BMH_ENOMEM; }
	return rc;
}
