// SAM records from the outputs of bmh_finalize_regs / bmh_finalize_pairs and bmh_cigar_batch: the host form.  What a record says
// (mem_aln2sam, mem_gen_alt, the unmapped record of mem_reg2sam, QUAL and -C) is csrc/sam_core.h, shared with the device kernels; here are the source over the
// caller's host arrays, the sink over a thread's string, the threads and the entry points.  Host code, like the reference's.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>
#include "bmh_internal.h"
#include "sam_core.h"

namespace {

// sam_core's sink over a formatting thread's string: one growth per field
struct string_out {
	std::string &s;
	void ch(char c) { s += c; }
	void str(const char *p, int len) { s.append(p, (size_t)len); }
	template <int N> void lit(const char (&l)[N]) { s.append(l, N - 1); }
	char *grow(int n) { const size_t at = s.size(); s.resize(at + (size_t)n); return &s[at]; }
	void num(long long v) { sam_core::put_num(grow(sam_core::num_len(v)), v); }
	template <class F> void fill(int len, F f) { char *d = grow(len); for (int j = 0; j < len; ++j) d[j] = f(j); }
};

// sam_core's Src over the arguments of bmh_format_sam_parts: nt4 codes (a code above 4 prints N), C strings for the names, alignments through bmh_cigar_src_t
struct host_src_t {
	const bmh_post_opt_t *po; const char *names; const uint64_t *name_off; const uint8_t *reads; const uint64_t *read_offs; const uint32_t *read_lens;
	int nc; const char *const *contig_names; const int64_t *contig_offset; const int32_t *fin; const uint32_t *fin_per_read; const bmh_cigar_src_t &cs;
	const int32_t *h_recs, *unflags; const uint8_t *quals; const char *comments; const uint64_t *comment_off;      // (comments: NULL unless -C copies them)
	const uint64_t *bases;                 // [n_reads] first record of every read
	const char *rg_id; int rg_n;           // read group: RG:Z:<id> on every record
	const bmh_read_groups_t *groups;       // ... or a read group per read (NULL: rg_id)
	struct read_t {
		const bmh_cigar_src_t &cs; uint64_t base; int n; const int32_t *fin;
		sam_core::aln_t aln(int i) const
		{
			sam_core::aln_t x; x.aln = nullptr; x.cigar = nullptr; x.md = "";
			const int64_t s = cs.slot32 ? (int64_t)cs.slot32[base + i] : cs.slot64[base + i];
			if (s >= 0) {
				x.aln = cs.aln + 8 * s;
				if (cs.packed) { x.cigar = cs.packed + cs.off[s]; if (cs.packed_md) x.md = (const char *)(x.cigar + x.aln[3]); }
				else { x.cigar = cs.cigar + (size_t)cs.max_cigar * s; if (cs.md) x.md = cs.md + (size_t)cs.md_cap * s; }
			}
			return x;
		}
	};
	read_t read(uint32_t r) const { return read_t{cs, bases[r], (int)fin_per_read[r], fin + 16 * bases[r]}; }
	bool flag_all() const { return po->flag_all; }
	bool softclip() const { return po->softclip; }
	int sa() const { return po->contig_is_alt ? 11 : 12; }       // (with ALT contigs a record keeps secondary_all, the XA tag's key, in [11]: see bmh_post_opt_t)
	double drop() const { return (double)po->XA_drop_ratio; }
	int max_XA_hits() const { return po->max_XA_hits; }
	int max_XA_hits_alt() const { return po->max_XA_hits_alt; }
	const char *rg() const { return rg_id; }
	int rg_len() const { return rg_n; }
	const char *rg_read(uint32_t r, int &len) const
	{
		if (!groups) { len = rg_n; return rg_id; }
		const uint32_t g = groups->read_group[r], o = groups->id_off[g];
		len = (int)(groups->id_off[g + 1] - o);
		return groups->ids + o;
	}
	bool paired() const { return h_recs != nullptr; }
	int h_rec(uint32_t r) const { return h_recs[r]; }
	int unflag(uint32_t r) const { return unflags ? unflags[r] : 0; }
	int md_len(const sam_core::aln_t &x) const { return (int)strlen(x.md); }
	const char *name(uint32_t r) const { return names + name_off[r]; }
	int name_len(uint32_t r) const { return (int)strlen(names + name_off[r]); }
	int l_seq(uint32_t r) const { return (int)read_lens[r]; }
	const uint8_t *seq(uint32_t r) const { return reads + read_offs[r]; }
	const uint8_t *qual(uint32_t r) const { return quals ? quals + read_offs[r] : nullptr; }
	const char *comment(uint32_t r, int &len) const { if (!comments) return nullptr; len = (int)strlen(comments + comment_off[r]); return comments + comment_off[r]; }
	char letter(uint8_t c, bool rev) const { return (rev ? "TGCAN" : "ACGTN")[c > 4 ? 4 : c]; }
	int n_contigs() const { return nc; }
	long long ctg_off(int i) const { return contig_offset[i]; }
	long long ctg0(int rid) const { return nc > 1 ? contig_offset[rid] : 0; }
	const char *ctg(int rid) const { return contig_names[rid]; }
	int ctg_len(int rid) const { return (int)strlen(contig_names[rid]); }
};

} // namespace

extern "C" void bmh_free(void *p) { free(p); }

// need[i] = 1 for every record of bmh_finalize_regs that must go through bmh_cigar_batch before formatting: the reported
// ones and the XA candidates (mem_gen_alt's two passes: sam_core::xa_primary, xa_listed).  Returns their number.
extern "C" int64_t bmh_sam_need_cigar(const bmh_post_opt_t *po, const int32_t *fin, const uint32_t *fin_per_read, uint32_t n_reads, uint8_t *need)
{
	if (!po || !fin_per_read || !need || (n_reads && !fin)) { bmh_set_error("bmh_sam_need_cigar: null argument"); return BMH_EINVAL; }
	int64_t total = 0; uint64_t base = 0;
	std::vector<int> cnt, has_alt;
	const int sa = po->contig_is_alt ? 11 : 12;
	const double drop = (double)po->XA_drop_ratio;
	for (uint32_t r = 0; r < n_reads; ++r) {
		const int n = (int)fin_per_read[r];
		const int32_t *a = fin + 16 * base;
		for (int i = 0; i < n; ++i) need[base + i] = (a[16 * i + 15] & 1) ? 1 : 0;
		if (!po->flag_all) {
			cnt.assign(n, 0); has_alt.assign(n, 0);
			for (int i = 0; i < n; ++i) { const int k = sam_core::xa_primary(a, i, sa, drop); if (k >= 0) { ++cnt[k]; if (a[16 * i + 15] & 2) has_alt[k] = 1; } }
			for (int i = 0; i < n; ++i) {
				const int k = sam_core::xa_primary(a, i, sa, drop);
				if (k >= 0 && sam_core::xa_listed(cnt[k], has_alt[k] != 0, po->max_XA_hits, po->max_XA_hits_alt)) need[base + i] = 1;
			}
		}
		for (int i = 0; i < n; ++i) total += need[base + i];
		base += n;
	}
	return total;
}

// slot[i] = index of record i in the bmh_cigar_batch outputs (aln [..][8], cigar [..][max_cigar], md [..][md_cap]) or -1.
// names: the read names, NUL-terminated, back to back; name_off[r] = start of read r's name.  contig_names: array of C
// strings.  reads: nt4 codes.  h_rec / unflag: NULL for single-end reads; for interleaved
// pairs the outputs of bmh_finalize_pairs (own-alignment record per read, flags of the unmapped record).
// the text as the parts its formatting threads made, in order (`parts` is the caller's: a caller that formats batch after batch keeps
// the strings, whose capacity survives clear(), so that no quarter-gigabyte buffer is allocated, faulted in and unmapped per batch)
bool bmh_format_sam_parts(const bmh_post_opt_t *po, uint32_t n_reads, const char *names, const uint64_t *name_off, const uint8_t *reads,
                          const uint64_t *read_offs, const uint32_t *read_lens, int n_contigs, const char *const *contig_names,
                          const int64_t *contig_offset, const int32_t *fin, const uint32_t *fin_per_read, const bmh_cigar_src_t &cs,
                          const int32_t *h_rec, const int32_t *unflag, std::vector<std::string> &parts,
                          const uint8_t *quals, const char *comments, const uint64_t *comment_off, const bmh_read_groups_t *groups)
{
	std::vector<uint64_t> bases((size_t)n_reads + 1, 0);
	for (uint32_t r = 0; r < n_reads; ++r) bases[r + 1] = bases[r] + fin_per_read[r];
	const bool cm = po->copy_comment && comments && comment_off;           // -C: the header comment behind every record (an empty one is not written)
	const char *rg = po->rg_id && po->rg_id[0] ? po->rg_id : nullptr;
	const host_src_t S{po, names, name_off, reads, read_offs, read_lens, n_contigs, contig_names, contig_offset, fin, fin_per_read, cs, h_rec, unflag, quals,
	                   cm ? comments : nullptr, comment_off, bases.data(), rg, rg ? (int)strlen(rg) : 0, groups};
	// reads are independent: format ranges of them on host threads (the reference formats inside its worker threads)
	// (threads: the hardware's, not bmh_effective_cpus(): a CPU quota limits the RATE of CPU time, and a batch's text is a burst -- on a box that
	// shows 256 threads and grants 16 CPUs' worth of time, 64 threads format a million reads in 14 ms, 16 threads in 45 ms)
	unsigned n_thr = n_reads >= 8192 ? std::thread::hardware_concurrency() : 1;
	if (n_thr < 1) n_thr = 1;
	if (n_thr > 64) n_thr = 64;
	if (parts.size() < n_thr) parts.resize(n_thr);
	for (std::string &p : parts) p.clear();
	std::vector<int> failed(n_thr, 0);
	auto work = [&](unsigned t) {
	string_out out{parts[t]};
	const uint32_t r_lo = (uint32_t)((uint64_t)n_reads * t / n_thr), r_hi = (uint32_t)((uint64_t)n_reads * (t + 1) / n_thr);
	out.s.reserve((size_t)(r_hi - r_lo) * 400);
	for (uint32_t r = r_lo; r < r_hi; ++r) {
		const int bad = sam_core::read_records(S, r, out);       // what a record says: csrc/sam_core.h
		if (bad < 0) continue;
		const uint32_t mr = r ^ 1u;
		if (h_rec && h_rec[mr] >= 0 && !S.read(mr).aln(h_rec[mr]).aln) bmh_set_error("bmh_format_sam_pe: the alignment record of read %u has no CIGAR", mr);
		else bmh_set_error("bmh_format_sam: record %d of read %u has no CIGAR (see bmh_sam_need_cigar)", bad, r);
		failed[t] = 1; return;
	}
	};
	if (n_thr == 1) work(0);
	else { std::vector<std::thread> th; for (unsigned t = 0; t < n_thr; ++t) th.emplace_back(work, t); for (auto &x : th) x.join(); }
	for (unsigned t = 0; t < n_thr; ++t)
		if (failed[t]) { if (n_thr > 1) bmh_set_error("bmh_format_sam: a record the text needs has no CIGAR (see bmh_sam_need_cigar)"); return false; }
	return true;
}

static char *format_sam(const bmh_post_opt_t *po, uint32_t n_reads, const char *names, const uint64_t *name_off, const uint8_t *reads,
                        const uint64_t *read_offs, const uint32_t *read_lens, int n_contigs, const char *const *contig_names,
                        const int64_t *contig_offset, const int32_t *fin, const uint32_t *fin_per_read, const int64_t *slot,
                        const int32_t *aln, const uint32_t *cigar, int max_cigar, const char *md, int md_cap,
                        const int32_t *h_rec, const int32_t *unflag, const uint8_t *quals, const char *comments, const uint64_t *comment_off, size_t *len_out,
                        const bmh_read_groups_t *groups = nullptr)
{
	std::vector<std::string> parts;
	bmh_cigar_src_t cs;
	cs.slot64 = slot; cs.aln = aln; cs.cigar = cigar; cs.max_cigar = max_cigar; cs.md = md; cs.md_cap = md_cap;
	if (!bmh_format_sam_parts(po, n_reads, names, name_off, reads, read_offs, read_lens, n_contigs, contig_names, contig_offset, fin, fin_per_read, cs, h_rec, unflag, parts,
	                          quals, comments, comment_off, groups)) return nullptr;
	const unsigned n_thr = (unsigned)parts.size();
	size_t total = 0;
	for (const std::string &p : parts) total += p.size();
	char *res = (char *)malloc(total + 1);
	if (!res) { bmh_set_error("bmh_format_sam: out of memory"); return nullptr; }
	{   // the parts into their places, on as many threads (the text of a million reads is a quarter of a gigabyte)
		std::vector<size_t> at(n_thr ? n_thr : 1, 0);
		for (unsigned t = 1; t < n_thr; ++t) at[t] = at[t - 1] + parts[t - 1].size();
		auto put = [&](unsigned t) { memcpy(res + at[t], parts[t].data(), parts[t].size()); std::string().swap(parts[t]); };
		if (n_thr <= 1) { if (n_thr) put(0); }
		else { std::vector<std::thread> th; for (unsigned t = 0; t < n_thr; ++t) th.emplace_back(put, t); for (auto &x : th) x.join(); }
	}
	res[total] = 0;
	*len_out = total;
	return res;
}

extern "C" char *bmh_format_sam_ex(const bmh_post_opt_t *po, uint32_t n_reads, const char *names, const uint64_t *name_off, const uint8_t *reads,
                                   const uint64_t *read_offs, const uint32_t *read_lens, const uint8_t *quals, const char *comments, const uint64_t *comment_off,
                                   int n_contigs, const char *const *contig_names, const int64_t *contig_offset, const int32_t *fin, const uint32_t *fin_per_read,
                                   const int64_t *slot, const int32_t *aln, const uint32_t *cigar, int max_cigar, const char *md, int md_cap, size_t *len_out)
{
	if (!po || !names || !name_off || !reads || !read_offs || !read_lens || !contig_names || !fin_per_read || !len_out || (n_contigs > 1 && !contig_offset) ||
	    (!comments) != (!comment_off)) {
		bmh_set_error("bmh_format_sam: null argument"); return nullptr;
	}
	return format_sam(po, n_reads, names, name_off, reads, read_offs, read_lens, n_contigs, contig_names, contig_offset, fin, fin_per_read, slot, aln, cigar, max_cigar,
	                  md, md_cap, nullptr, nullptr, quals, comments, comment_off, len_out);
}

extern "C" char *bmh_format_sam(const bmh_post_opt_t *po, uint32_t n_reads, const char *names, const uint64_t *name_off, const uint8_t *reads,
                                const uint64_t *read_offs, const uint32_t *read_lens, int n_contigs, const char *const *contig_names,
                                const int64_t *contig_offset, const int32_t *fin, const uint32_t *fin_per_read, const int64_t *slot,
                                const int32_t *aln, const uint32_t *cigar, int max_cigar, const char *md, int md_cap, size_t *len_out)
{
	return bmh_format_sam_ex(po, n_reads, names, name_off, reads, read_offs, read_lens, nullptr, nullptr, nullptr, n_contigs, contig_names, contig_offset, fin,
	                         fin_per_read, slot, aln, cigar, max_cigar, md, md_cap, len_out);
}

// a read group per read (include/bwamem_hip.h: bmh_read_groups_t); h_rec / unflag NULL: single-end reads
extern "C" char *bmh_format_sam_groups(const bmh_post_opt_t *po, uint32_t n_reads, const char *names, const uint64_t *name_off, const uint8_t *reads,
                                       const uint64_t *read_offs, const uint32_t *read_lens, const uint8_t *quals, const char *comments, const uint64_t *comment_off,
                                       int n_contigs, const char *const *contig_names, const int64_t *contig_offset, const int32_t *fin, const uint32_t *fin_per_read,
                                       const int32_t *h_rec, const int32_t *unflag, const int64_t *slot, const int32_t *aln, const uint32_t *cigar, int max_cigar,
                                       const char *md, int md_cap, const bmh_read_groups_t *groups, size_t *len_out)
{
	const char *fn = "bmh_format_sam_groups";
	if (!po || !names || !name_off || !reads || !read_offs || !read_lens || !contig_names || !fin_per_read || !len_out || (n_contigs > 1 && !contig_offset) ||
	    (!comments) != (!comment_off) || (!h_rec) != (!unflag) || (h_rec && (n_reads & 1)) || !groups || !groups->ids || !groups->id_off || (n_reads && !groups->read_group)) {
		bmh_set_error("%s: bad argument", fn); return nullptr;
	}
	if (po->rg_id && po->rg_id[0]) { bmh_set_error("%s: a read group per read beside the options' one read group (rg_id '%s')", fn, po->rg_id); return nullptr; }
	for (uint32_t r = 0; r < n_reads; ++r)
		if (groups->read_group[r] >= groups->n_groups) { bmh_set_error("%s: read %u is of group %u: the table holds %u", fn, r, groups->read_group[r], groups->n_groups); return nullptr; }
	return format_sam(po, n_reads, names, name_off, reads, read_offs, read_lens, n_contigs, contig_names, contig_offset, fin, fin_per_read, slot, aln, cigar, max_cigar,
	                  md, md_cap, h_rec, unflag, quals, comments, comment_off, len_out, groups);
}

// interleaved pairs: fin / fin_per_read / h_rec / unflag from bmh_finalize_pairs (mem_aln2sam with the mate: flags 0x8 0x20,
// RNEXT, PNEXT, TLEN; an unmapped read takes its mate's coordinate and strand)
extern "C" char *bmh_format_sam_pe_ex(const bmh_post_opt_t *po, uint32_t n_reads, const char *names, const uint64_t *name_off, const uint8_t *reads,
                                      const uint64_t *read_offs, const uint32_t *read_lens, const uint8_t *quals, const char *comments, const uint64_t *comment_off,
                                      int n_contigs, const char *const *contig_names, const int64_t *contig_offset, const int32_t *fin, const uint32_t *fin_per_read,
                                      const int32_t *h_rec, const int32_t *unflag, const int64_t *slot, const int32_t *aln, const uint32_t *cigar, int max_cigar,
                                      const char *md, int md_cap, size_t *len_out)
{
	if (!po || !names || !name_off || !reads || !read_offs || !read_lens || !contig_names || !fin_per_read || !h_rec || !unflag || !len_out || (n_reads & 1) ||
	    (n_contigs > 1 && !contig_offset) || (!comments) != (!comment_off)) { bmh_set_error("bmh_format_sam_pe: bad argument"); return nullptr; }
	return format_sam(po, n_reads, names, name_off, reads, read_offs, read_lens, n_contigs, contig_names, contig_offset, fin, fin_per_read, slot, aln, cigar, max_cigar,
	                  md, md_cap, h_rec, unflag, quals, comments, comment_off, len_out);
}

extern "C" char *bmh_format_sam_pe(const bmh_post_opt_t *po, uint32_t n_reads, const char *names, const uint64_t *name_off, const uint8_t *reads,
                                   const uint64_t *read_offs, const uint32_t *read_lens, int n_contigs, const char *const *contig_names,
                                   const int64_t *contig_offset, const int32_t *fin, const uint32_t *fin_per_read, const int32_t *h_rec,
                                   const int32_t *unflag, const int64_t *slot, const int32_t *aln, const uint32_t *cigar, int max_cigar,
                                   const char *md, int md_cap, size_t *len_out)
{
	return bmh_format_sam_pe_ex(po, n_reads, names, name_off, reads, read_offs, read_lens, nullptr, nullptr, nullptr, n_contigs, contig_names, contig_offset, fin,
	                            fin_per_read, h_rec, unflag, slot, aln, cigar, max_cigar, md, md_cap, len_out);
}

// bmh_sam_need_cigar for pairs: additionally the own-alignment record of every read (the mate fields come from it)
extern "C" int64_t bmh_sam_need_cigar_pe(const bmh_post_opt_t *po, const int32_t *fin, const uint32_t *fin_per_read, const int32_t *h_rec,
                                         uint32_t n_reads, uint8_t *need)
{
	if (!h_rec) { bmh_set_error("bmh_sam_need_cigar_pe: null argument"); return BMH_EINVAL; }
	int64_t total = bmh_sam_need_cigar(po, fin, fin_per_read, n_reads, need);
	if (total < 0) return total;
	uint64_t base = 0;
	for (uint32_t r = 0; r < n_reads; ++r) {
		if (h_rec[r] >= 0 && !need[base + h_rec[r]]) { need[base + h_rec[r]] = 1; ++total; }
		base += fin_per_read[r];
	}
	return total;
}
