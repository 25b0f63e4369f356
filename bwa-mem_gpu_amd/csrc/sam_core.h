// The SAM records of one read -- mem_aln2sam (the reference's src/bwamem.c:1506-1683: field order, hard clips on every record of a read
// after its first, SEQ/QUAL of secondary records, NM MD AS XS RG SA pa:f XA and the -C comment), mem_gen_alt (src/bwamem_extra.c:97-150: the
// XA tag) and the unmapped record of mem_reg2sam (src/bwamem.c:1721-1770) -- as ONE piece of code for the device kernels of
// csrc/sam_kernels.hip, for the host formatter csrc/sam_format.cpp and for a plain C++ build (tests/sam_core_host.cpp).  No HIP header.
//
// read_records<Src, Out> is what a record says.  Where the inputs live is the Src's business, where the bytes go the Out's:
//   Src   flag_all() softclip() sa() drop() max_XA_hits() max_XA_hits_alt() rg() rg_len()          the options (sa: the record field of the XA key)
//         rg_read(r, len)                                                                          optional: read r's own read group (a run that keeps its input's); a Src without it: rg() / rg_len() for every read
//         paired() h_rec(r) unflag(r)                                                              pairs: own-alignment record, flags of the unmapped record
//         read(r) -> { n, fin, aln(i) }                                                            the read's 16-int records; aln(i).aln == nullptr: none
//         md_len(x)  name(r) name_len(r)  l_seq(r) seq(r) letter(c, rev) qual(r)  comment(r, len)  MD length; name; bases, SEQ letter of a base, QUAL or nullptr
//         n_contigs() ctg_off(i) ctg0(rid) ctg(rid) ctg_len(rid)                                   contig offsets (ctg0: 0 with one contig), names
//   Out   ch(c)  str(p, len)  lit("..")  num(v)  fill(n, f): the n bytes f(0) .. f(n - 1) in one step (SEQ, QUAL)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SAM_FN __host__ __device__ inline
#else
#define SAM_FN inline
#endif
#define SAM_INL SAM_FN __attribute__((always_inline))

namespace sam_core {

// ---- the XA tag's selection (mem_gen_alt's two passes): the text, bmh_sam_need_cigar[_pe] and bmh_sam_select_device go by these two
// the primary record i is listed under, or -1: its key a[16 i + sa], if it scores at least `drop` of it (get_pri_idx takes XA_drop_ratio as a
// double: the float 0.8 widened, so a hit at exactly 80 % of its primary is out)
SAM_INL int xa_primary(const int32_t *a, int i, int sa, double drop)
{
	const int k = a[16 * i + sa];
	return (k >= 0 && (double)a[16 * i + 1] >= (double)a[16 * k + 1] * drop) ? k : -1;
}
// a primary with cnt hits under it, one of them on an ALT contig or not, lists them (src/bwamem_extra.c:125)
SAM_INL bool xa_listed(int cnt, bool has_alt, int max_XA_hits, int max_XA_hits_alt) { return !(cnt > max_XA_hits_alt || (!has_alt && cnt > max_XA_hits)); }

// ---- sinks: decimal digits by hand (a record holds nine or more numbers), counted or written through any pointer type (global, LDS, host)
SAM_INL int num_len(long long v)
{
	unsigned long long u = v < 0 ? 0ull - (unsigned long long)v : (unsigned long long)v;
	int nd = v < 0 ? 2 : 1;
	for (; u >= 10; u /= 10) ++nd;
	return nd;
}
template <class P> SAM_INL P put_num(P p, long long v)
{
	unsigned long long u = v < 0 ? 0ull - (unsigned long long)v : (unsigned long long)v;
	if (v < 0) *p++ = '-';
	int nd = 1;
	for (unsigned long long t = u; t >= 10; t /= 10) ++nd;
	P q = p + nd;
	do { *--q = (char)('0' + u % 10); u /= 10; } while (u);
	return p + nd;
}
struct count_out {
	uint32_t n = 0;
	SAM_INL void ch(char) { ++n; }
	SAM_INL void str(const char *, int len) { n += (uint32_t)len; }
	template <int N> SAM_INL void lit(const char (&)[N]) { n += N - 1; }
	SAM_INL void num(long long v) { n += (uint32_t)num_len(v); }
	template <class F> SAM_INL void fill(int len, F) { n += (uint32_t)len; }
};
template <class P> struct ptr_out {
	P p;
	SAM_INL void ch(char c) { *p++ = c; }
	SAM_INL void str(const char *s, int len) { for (int i = 0; i < len; ++i) *p++ = s[i]; }
	template <int N> SAM_INL void lit(const char (&s)[N]) { for (int i = 0; i < N - 1; ++i) *p++ = s[i]; }
	SAM_INL void num(long long v) { p = put_num(p, v); }
	template <class F> SAM_INL void fill(int len, F f) { for (int j = 0; j < len; ++j) *p++ = f(j); }
};

// ---- the small rules
struct aln_t { const int32_t *aln; const uint32_t *cigar; const char *md; };     // aln[8] of bmh_cigar_batch, its operations, its MD string
struct mate_t { int rid; long long pos; int is_rev, n_cigar; const uint32_t *cigar; };

SAM_INL long long aln_pos(const int32_t *a) { return (long long)(uint32_t)a[0] | (long long)a[1] << 32; }
template <class Src> SAM_INL int contig_of(const Src &S, long long pos)
{
	if (S.n_contigs() <= 1) return 0;
	int lo = 0, hi = S.n_contigs();                 // last sequence starting at or before pos
	while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (S.ctg_off(mid) <= pos) lo = mid; else hi = mid; }
	return lo;
}
SAM_INL int ref_len(int n, const uint32_t *cg)      // get_rlen, src/bwamem.c:1496-1504
{
	int l = 0;
	for (int k = 0; k < n; ++k) { const int op = (int)(cg[k] & 0xf); if (op == 0 || op == 2) l += (int)(cg[k] >> 4); }
	return l;
}
template <class Out> SAM_FN void put_cigar(Out &o, const aln_t &x, bool hard)
{
	const int n = x.aln[3];
	for (int i = 0; i < n; ++i) {
		int c = (int)(x.cigar[i] & 0xf);
		if (hard && (c == 3 || c == 4)) c = 4;
		o.num(x.cigar[i] >> 4);
		o.ch("MIDSH"[c]);
	}
}
// a hard-clipped record prints only the aligned part [qb, qe) of the read
SAM_INL void clip_range(const aln_t &x, int &qb, int &qe)
{
	const int nc = x.aln[3];
	if (!nc) return;
	const int c0 = (int)(x.cigar[0] & 0xf), c1 = (int)(x.cigar[nc - 1] & 0xf);
	if (!x.aln[2]) { if (c0 == 3 || c0 == 4) qb += x.cigar[0] >> 4; if (c1 == 3 || c1 == 4) qe -= x.cigar[nc - 1] >> 4; }
	else { if (c0 == 3 || c0 == 4) qe -= x.cigar[0] >> 4; if (c1 == 3 || c1 == 4) qb += x.cigar[nc - 1] >> 4; }
}
template <class Src, class Out> SAM_INL void put_ctg(const Src &S, Out &o, int rid) { o.str(S.ctg(rid), S.ctg_len(rid)); }
// SEQ: bases [qb, qe) as letters, reverse-complemented on the reverse strand; QUAL: the qualities as they are, reversed (not complemented)
template <class Src, class Out> SAM_FN void put_seq(const Src &S, Out &o, const uint8_t *seq, int qb, int qe, bool rev)
{
	if (qe <= qb) return;
	if (!rev) o.fill(qe - qb, [&](int j) { return S.letter(seq[qb + j], false); });
	else o.fill(qe - qb, [&](int j) { return S.letter(seq[qe - 1 - j], true); });
}
template <class Out> SAM_FN void put_qual(Out &o, const uint8_t *q, int qb, int qe, bool rev)
{
	if (qe <= qb) return;
	if (!rev) o.fill(qe - qb, [&](int j) { return (char)q[qb + j]; });
	else o.fill(qe - qb, [&](int j) { return (char)q[qe - 1 - j]; });
}
// RNEXT PNEXT TLEN of a record at (p_*) whose mate is at (m_*)
template <class Src, class Out> SAM_FN void mate_fields(const Src &S, Out &o, bool pe, int p_rid, long long p_pos, int p_rev, int p_ncig, const uint32_t *p_cig,
                                                       bool mate_mapped, int m_rid, long long m_pos, int m_rev, int m_ncig, const uint32_t *m_cig)
{
	if (pe && mate_mapped) {
		if (p_rid == m_rid) o.ch('='); else put_ctg(S, o, m_rid);
		o.ch('\t'); o.num(m_pos - S.ctg0(m_rid) + 1); o.ch('\t');
		if (p_rid == m_rid) {
			const long long p0 = p_pos + (p_rev ? ref_len(p_ncig, p_cig) - 1 : 0), p1 = m_pos + (m_rev ? ref_len(m_ncig, m_cig) - 1 : 0);
			if (m_ncig == 0 || p_ncig == 0) o.ch('0');
			else o.num(-(p0 - p1 + (p0 > p1 ? 1 : p0 < p1 ? -1 : 0)));
		} else o.ch('0');
	} else o.lit("*\t0\t0");
	o.ch('\t');
}
// a / b as printf("%.3f") writes it (the pa:f tag, src/bwamem.c:1663): the double nearest to a / b, rounded to three decimals from its EXACT value, ties to even
// -- m x 2^e x 1000 in integers
template <class Out> SAM_FN void fmt3(Out &o, int a, int b)
{
	const double x = (double)a / (double)b;
	unsigned long long q = 0;
	if (x > 0.) {
		unsigned long long bits;
		__builtin_memcpy(&bits, &x, 8);
		const int ex = (int)(bits >> 52 & 0x7FF);
		const unsigned long long m = ex ? (bits & 0xFFFFFFFFFFFFFull) | 1ull << 52 : (bits & 0xFFFFFFFFFFFFFull);
		const int e = (ex ? ex : 1) - 1075;                         // x = m * 2^e
		const unsigned long long N = m * 1000ull;                   // < 2^63
		if (e >= 0) q = N << e;                                     // (not reached for a ratio of two scores)
		else if (-e >= 64) q = 0;
		else {
			const int sft = -e;
			q = N >> sft;
			const unsigned long long rem = N & ((1ull << sft) - 1), half = 1ull << (sft - 1);
			if (rem > half || (rem == half && (q & 1))) ++q;
		}
	}
	o.num((long long)(q / 1000));
	o.ch('.');
	const int f = (int)(q % 1000);
	o.ch((char)('0' + f / 100)); o.ch((char)('0' + f / 10 % 10)); o.ch((char)('0' + f % 10));
}

// ---- the read group of read r's records: the Src's rg_read(r, len) when it has one, else its one rg() / rg_len() (overload resolution prefers the int form)
template <class Src> SAM_INL auto read_rg(const Src &S, uint32_t r, int &len, int) -> decltype(S.rg_read(r, len)) { return S.rg_read(r, len); }
template <class Src> SAM_INL const char *read_rg(const Src &S, uint32_t, int &len, long) { len = S.rg_len(); return S.rg(); }

// ---- the records of read r: the unmapped record when nothing is reported, else every reported record in order.  Returns a negative value, or -- a record the
// text needs has no alignment -- the index of that record in its read (the mate's own-alignment record is looked at first, before anything is written)
template <class Src, class Out> SAM_FN int read_records(const Src &S, uint32_t r, Out &out)
{
	const auto R = S.read(r);
	const int n = R.n;
	const int32_t *a = R.fin;
	const bool pe = S.paired();
	mate_t m; m.rid = -1; m.pos = 0; m.is_rev = 0; m.n_cigar = 0; m.cigar = nullptr;      // the mate's own alignment (mem_sam_pe's h[!i])
	if (pe) {
		const uint32_t mr = r ^ 1u;
		const int h = S.h_rec(mr);
		if (h >= 0) {
			const aln_t y = S.read(mr).aln(h);
			if (!y.aln) return h;
			m.pos = aln_pos(y.aln); m.rid = contig_of(S, m.pos); m.is_rev = y.aln[2]; m.n_cigar = y.aln[3]; m.cigar = y.cigar;
		}
	}
	const char *name = S.name(r);
	const int name_len = S.name_len(r);
	const uint8_t *seq = S.seq(r);
	const uint8_t *qual = S.qual(r);
	int cmt_len = 0;
	const char *cmt = S.comment(r, cmt_len);
	const int l_seq = S.l_seq(r);
	int rg_len = 0;
	const char *rg = read_rg(S, r, rg_len, 0);
	int n_rep = 0;
	for (int i = 0; i < n; ++i) n_rep += a[16 * i + 15] & 1;
	if (n_rep == 0) {                                           // unmapped record (mem_reg2sam's aa.n == 0 branch)
		int flag = 4 | S.unflag(r);
		const bool mm = pe && m.rid >= 0;
		if (pe && m.rid < 0) flag |= 8;
		const int p_rev = mm ? m.is_rev : 0;                     // an unmapped read takes its mate's coordinate and strand
		if (p_rev) flag |= 0x10;
		if (mm && m.is_rev) flag |= 0x20;
		out.str(name, name_len); out.ch('\t'); out.num(flag); out.ch('\t');
		if (mm) { put_ctg(S, out, m.rid); out.ch('\t'); out.num(m.pos - S.ctg0(m.rid) + 1); out.lit("\t0\t*\t"); }
		else out.lit("*\t0\t0\t*\t");
		mate_fields(S, out, pe, mm ? m.rid : -1, m.pos, p_rev, 0, nullptr, mm, m.rid, m.pos, m.is_rev, m.n_cigar, m.cigar);
		put_seq(S, out, seq, 0, l_seq, p_rev != 0);
		out.ch('\t');
		if (qual) put_qual(out, qual, 0, l_seq, p_rev != 0); else out.ch('*');
		out.lit("\tAS:i:0\tXS:i:0");
		if (rg_len) { out.lit("\tRG:Z:"); out.str(rg, rg_len); }
		if (cmt_len > 0) { out.ch('\t'); out.str(cmt, cmt_len); }
		out.ch('\n');
		return -1;
	}
	const int sa = S.sa();
	const double drop = S.drop();
	int which = 0;
	for (int i = 0; i < n; ++i) {
		if (!(a[16 * i + 15] & 1)) continue;
		const int32_t *fin = a + 16 * i;
		const aln_t x = R.aln(i);
		if (!x.aln) return i;
		const long long pos = aln_pos(x.aln);
		const int rid = contig_of(S, pos);
		// a mapped read whose mate is unmapped lends it its coordinate and strand (mem_aln2sam :1518-1521)
		const bool mate_mapped = pe && m.rid >= 0;
		const int m_rid = mate_mapped ? m.rid : rid; const long long m_pos = mate_mapped ? m.pos : pos; const int m_rev = mate_mapped ? m.is_rev : (x.aln[2] ? 1 : 0);
		int flag = (x.aln[2] ? 0x10 : 0) | fin[14];
		if (pe) { if (m.rid < 0) flag |= 8; if (m_rev) flag |= 0x20; }
		const bool hard = which > 0 && !S.softclip() && !(fin[15] & 2);       // src/bwamem.c:1540,1578 (never on an ALT hit)
		out.str(name, name_len); out.ch('\t'); out.num((flag & 0xffff) | (flag & 0x10000 ? 0x100 : 0)); out.ch('\t');
		put_ctg(S, out, rid); out.ch('\t'); out.num(pos - S.ctg0(rid) + 1); out.ch('\t');
		out.num(fin[13]); out.ch('\t');
		if (x.aln[3]) put_cigar(out, x, hard); else out.ch('*');
		out.ch('\t');
		mate_fields(S, out, pe, rid, pos, x.aln[2] ? 1 : 0, x.aln[3], x.cigar, pe, m_rid, m_pos, m_rev, mate_mapped ? m.n_cigar : 0, mate_mapped ? m.cigar : nullptr);
		if (flag & 0x100) out.lit("*\t*");
		else {
			int qb = 0, qe = l_seq;
			if (hard) clip_range(x, qb, qe);
			put_seq(S, out, seq, qb, qe, x.aln[2] != 0);
			out.ch('\t');
			if (qual) put_qual(out, qual, qb, qe, x.aln[2] != 0); else out.ch('*');
		}
		if (x.aln[3]) { out.lit("\tNM:i:"); out.num(x.aln[4]); out.lit("\tMD:Z:"); out.str(x.md, S.md_len(x)); }
		if (fin[1] >= 0) { out.lit("\tAS:i:"); out.num(fin[1]); }
		if (!(flag & 0x100) && fin[10] >= 0) { out.lit("\tXS:i:"); out.num(fin[10]); }      // sub is not printed for secondary records (q->sub = -1)
		if (rg_len) { out.lit("\tRG:Z:"); out.str(rg, rg_len); }      // src/bwamem.c:1631-1634
		if (!(flag & 0x100)) {                                     // SA: the other reported records that are not secondary
			bool other = false;
			for (int j = 0; j < n; ++j) if (j != i && (a[16 * j + 15] & 1) && !(a[16 * j + 14] & 0x100)) other = true;
			if (other) {
				out.lit("\tSA:Z:");
				for (int j = 0; j < n; ++j) {
					if (j == i || !(a[16 * j + 15] & 1) || (a[16 * j + 14] & 0x100)) continue;
					const aln_t y = R.aln(j);
					if (!y.aln) return j;
					const long long p2 = aln_pos(y.aln);
					const int rid2 = contig_of(S, p2);
					put_ctg(S, out, rid2); out.ch(','); out.num(p2 - S.ctg0(rid2) + 1); out.ch(',');
					out.ch("+-"[y.aln[2] ? 1 : 0]); out.ch(',');
					put_cigar(out, y, false);
					out.ch(','); out.num(a[16 * j + 13]); out.ch(','); out.num(y.aln[4]); out.ch(';');
				}
			}
		}
		if (!(flag & 0x100) && (fin[15] >> 2) > 0) { out.lit("\tpa:f:"); fmt3(out, fin[1], fin[15] >> 2); }      // score / score of the ALT hit that shadows it (src/bwamem.c:1663)
		if (!S.flag_all()) {                                       // the XA tag of this record: the hits listed under it (mem_gen_alt)
			int cnt = 0; bool has_alt = false;
			for (int j = 0; j < n; ++j) if (xa_primary(a, j, sa, drop) == i) { ++cnt; has_alt = has_alt || (a[16 * j + 15] & 2); }
			if (cnt > 0 && xa_listed(cnt, has_alt, S.max_XA_hits(), S.max_XA_hits_alt())) {
				out.lit("\tXA:Z:");
				for (int j = 0; j < n; ++j) {
					if (xa_primary(a, j, sa, drop) != i) continue;
					const aln_t y = R.aln(j);
					if (!y.aln) return j;
					const long long p2 = aln_pos(y.aln);
					const int rid2 = contig_of(S, p2);
					put_ctg(S, out, rid2); out.ch(','); out.ch("+-"[y.aln[2] ? 1 : 0]); out.num(p2 - S.ctg0(rid2) + 1); out.ch(',');
					put_cigar(out, y, false);
					out.ch(','); out.num(y.aln[4]); out.ch(';');
				}
			}
		}
		if (cmt_len > 0) { out.ch('\t'); out.str(cmt, cmt_len); }              // src/bwamem.c:1670-1673
		out.ch('\n');
		++which;
	}
	return -1;
}

} // namespace sam_core
