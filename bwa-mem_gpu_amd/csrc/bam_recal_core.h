// Covariate counting for base quality score recalibration: the per-record and per-base rules of csrc/bam_recal_kernels.hip (a group of lanes per
// record) and, compiled as plain C++, of csrc/bam_recal_host.cpp and tests/bam_recal_core_host.cpp (under the sanitizers).  Every result is a uint64 sum over
// bases or records, so no result depends on the order of the records, on windows or on the form.
//
//   counted   refID in 0 .. n_contigs - 1; none of 0x4 0x100 0x200 0x400 (0x800 counts); mapq neither 0 nor 255; qualities (not all 0xff; l_seq > 0); at least
//             one operation.  The first reason that holds, in this order, is the one a record is left out for
//   refused   of counted records only, by the record's index, in this order: M I S = X lengths that do not sum to l_seq; the long-CIGAR placeholder (l_seq S,
//             then N, with a CG:B,I tag: the rule of bcv_check -- seen only when the tags can be walked); pos below 0 or pos + the reference length (M D N = X)
//             beyond the contig; tags that cannot be walked to the record's end; with a group table no RG tag, an RG tag of another type than Z, an ID the
//             table does not hold.  A record whose bytes do not hold what it announces is refused as not whole
//   kept      the stored bases s0 .. s0 + n - 1 between the leading and the trailing run of S (H, P and empty operations beside them are passed over)
//   order     sequencing order: base k is stored base s0 + k of a forward record and the complement of stored base s0 + n - 1 - k of a 0x10 record
//   cycle     k + 1, negated with 0x1 and 0x80; magnitudes above max_cycle share max_cycle.  Slot max_cycle + c - 1 for cycle c > 0, max_cycle + c for c < 0
//   context   mismatch: bases k - 1, k as 4 a + b (A C G T = 0 1 2 3), none (16) when k < 1 or a base is no ACGT; indel: k - 2 .. k as 16 a + 4 b + c, none (64)
//   events    snp: under M = X the stored base differs from the reference's.  ins / del: the kept base before a run of I / a D (forward record: the last
//             base in front of it; 0x10 record: the first base behind it); a base inside an I run never carries ins
//   skipped   for all three events, the first that holds: a stored code outside A C G T (1 2 4 8); a quality below min_qual; under M = X a masked reference
//             position; inside I a masked position before the operation (pos + reference offset - 1, when that is 0 or more)
//   observed  every other base: event M at its quality (above 93: 93) with error snp, events I and D at quality 45 with errors ins, del -- each into the
//             cycle table and into the context table (or its slot `none`).  I and D see the same bases: their observations are one word
#pragma once
#include <stdint.h>
#include "bam_sort_core.h"

#define BRC_FN BSR_FN

enum { BRC_NQ = 94, BRC_INDEL_Q = 45, BRC_MCTX = 17, BRC_ICTX = 65, BRC_MAX_GROUPS = 255, BRC_MIN_QUAL = 6, BRC_MAX_CYCLE = 500, BRC_CYCLE_LIMIT = 65535 };
enum { BRC_SEEN = 0, BRC_COUNTED, BRC_F_REF, BRC_F_FLAGS, BRC_F_MAPQ, BRC_F_NOQUAL, BRC_F_NOOPS, BRC_KEPT, BRC_SK_BASE, BRC_SK_QUAL, BRC_SK_MASK, BRC_SK_ANCHOR, BRC_CAPPED, BRC_MASKED,
       BRC_N_SUM = 16 };
enum { BRC_OK = 0, BRC_E_SUM = 1, BRC_E_PLACEHOLDER, BRC_E_SPAN, BRC_E_TAGS, BRC_E_RG_NONE, BRC_E_RG_TYPE, BRC_E_RG_ID, BRC_E_CUT, BRC_FILTERED = 16 };
enum { BRC_SKIP_FLAGS = 0x4 | 0x100 | 0x200 | 0x400 };
#define BRC_MAX_WORDS (1ull << 28)

// what a run is made under, and the accumulator's layout: the summary words, then
//   cy_m [group][quality][slot][2]   event M by cycle: observations, errors          cy_id [group][slot][3]     events I and D by cycle: observations, ins, del errors
//   cx_m [group][quality][17][2]     event M by context (16: none)                   cx_id [group][65][3]       events I and D by context (64: none)
struct brc_plan_t {
	int32_t n_contigs, n_groups, has_groups, min_qual, max_cycle;
	BRC_FN uint64_t ncy() const { return 2ull * (uint64_t)max_cycle; }
	BRC_FN uint64_t w_cy_m() const { return BRC_N_SUM; }
	BRC_FN uint64_t w_cy_id() const { return w_cy_m() + (uint64_t)n_groups * BRC_NQ * ncy() * 2; }
	BRC_FN uint64_t w_cx_m() const { return w_cy_id() + (uint64_t)n_groups * ncy() * 3; }
	BRC_FN uint64_t w_cx_id() const { return w_cx_m() + (uint64_t)n_groups * BRC_NQ * BRC_MCTX * 2; }
	BRC_FN uint64_t words() const { return w_cx_id() + (uint64_t)n_groups * BRC_ICTX * 3; }
	BRC_FN uint64_t at_cy_m(uint32_t g, uint32_t q, uint32_t ci) const { return w_cy_m() + (((uint64_t)g * BRC_NQ + q) * ncy() + ci) * 2; }
	BRC_FN uint64_t at_cy_id(uint32_t g, uint32_t ci) const { return w_cy_id() + ((uint64_t)g * ncy() + ci) * 3; }
	BRC_FN uint64_t at_cx_m(uint32_t g, uint32_t q, uint32_t c) const { return w_cx_m() + (((uint64_t)g * BRC_NQ + q) * BRC_MCTX + c) * 2; }
	BRC_FN uint64_t at_cx_id(uint32_t g, uint32_t c) const { return w_cx_id() + ((uint64_t)g * BRC_ICTX + c) * 3; }
};

// the reference as both forms read it: the .pac body (4 bases a byte, the first in the top bits), the mask (bit i & 63 of word i >> 6; NULL: nothing masked), every
// contig's first base in both and its length, the group IDs back to back with their NULs (rg_off [n_groups + 1])
struct brc_ref_t { const uint8_t *pac; const uint64_t *mask; const uint64_t *coff; const int32_t *clen; const char *rg; const uint32_t *rg_off; };

BRC_FN uint32_t brc_pac_base(const uint8_t *pac, uint64_t i) { return pac[i >> 2] >> ((~i & 3u) << 1) & 3u; }
BRC_FN bool brc_masked(const uint64_t *mask, uint64_t i) { return mask && (mask[i >> 6] >> (i & 63u) & 1u); }

// a counted record, ready for its bases
struct brc_rec_t {
	uint64_t ops_at, seq_at, qual_at, gpos;                            // gpos: the position of its first reference base in pac and mask
	uint32_t n_ops, s0, n, group; int32_t pos; bool rev, neg;
};

// the operation the stored base i lies in, of the operations from k on: q0 / r0 the stored bases / reference bases in front of it
struct brc_cur_t { uint32_t k; uint64_t q0, r0; uint32_t op; uint64_t len; };

BRC_FN bool brc_op_query(uint32_t op) { return op == 0 || op == 1 || op == 4 || op == 7 || op == 8; }
BRC_FN bool brc_op_ref(uint32_t op) { return op == 0 || op == 2 || op == 3 || op == 7 || op == 8; }

// the tags from byte p on: true when they can be walked to the record's end.  *cg: a CG:B,I tag; *rg_type (0: none), *rg_at: the first RG tag's type and value
BRC_FN bool brc_tags(const uint8_t *rec, uint64_t size, uint64_t p, bool *cg, uint8_t *rg_type, uint64_t *rg_at)
{
	*cg = false; *rg_type = 0; *rg_at = 0;
	while (p < size) {
		if (size - p < 3) return false;
		const uint8_t a = rec[p], b = rec[p + 1], t = rec[p + 2];
		p += 3;
		uint64_t len;
		if (t == 'A' || t == 'c' || t == 'C') len = 1;
		else if (t == 's' || t == 'S') len = 2;
		else if (t == 'i' || t == 'I' || t == 'f') len = 4;
		else if (t == 'Z' || t == 'H') {
			len = 0;
			while (p + len < size && rec[p + len]) ++len;
			if (p + len >= size) return false;
			++len;
		} else if (t == 'B') {
			if (size - p < 5) return false;
			const uint8_t s = rec[p];
			const uint64_t w = s == 'c' || s == 'C' ? 1 : s == 's' || s == 'S' ? 2 : s == 'i' || s == 'I' || s == 'f' ? 4 : 0;
			if (!w) return false;
			if (a == 'C' && b == 'G' && s == 'I') *cg = true;
			len = 5 + w * (uint64_t)bsr_u32(rec + p + 1);
		} else return false;
		if (len > size - p) return false;
		if (a == 'R' && b == 'G' && !*rg_type) { *rg_type = t; *rg_at = p; }
		p += len;
	}
	return true;
}

// the group of the NUL-terminated ID at id, or -1
BRC_FN int brc_group_of(const uint8_t *id, const brc_plan_t &P, const brc_ref_t &F)
{
	for (int g = 0; g < P.n_groups; ++g) {
		const char *s = F.rg + F.rg_off[g];
		uint32_t k = 0;
		while (s[k] && (uint8_t)s[k] == id[k]) ++k;
		if (!s[k] && !id[k]) return g;
	}
	return -1;
}

// the record of `size` bytes -> BRC_OK and R (counted), BRC_FILTERED + the reason (0 .. 4: left out), or why it is refused
BRC_FN int brc_prep(const uint8_t *rec, uint64_t size, const brc_plan_t &P, const brc_ref_t &F, brc_rec_t &R)
{
	if (size < BSR_FIXED) return BRC_E_CUT;
	const uint32_t flag = bsr_flag(rec), mapq = rec[13];
	const int32_t ref = bsr_ref(rec);
	if (ref < 0 || ref >= P.n_contigs) return BRC_FILTERED + 0;
	if (flag & (uint32_t)BRC_SKIP_FLAGS) return BRC_FILTERED + 1;
	if (mapq == 0 || mapq == 255) return BRC_FILTERED + 2;
	const uint32_t n_ops = bsr_u16(rec + 16);
	const uint64_t l_seq = bsr_u32(rec + 20);
	R.n_ops = n_ops; R.ops_at = (uint64_t)BSR_FIXED + rec[12]; R.seq_at = R.ops_at + 4ull * n_ops; R.qual_at = R.seq_at + (l_seq + 1) / 2;
	const uint64_t tags_at = R.qual_at + l_seq;
	if (tags_at > size) return BRC_E_CUT;
	bool qual = false;                                                 // (a record with qualities has one in front: the whole row is read only for one that begins 0xff)
	for (uint64_t i = 0; i < l_seq && !qual; ++i) qual = rec[R.qual_at + i] != 0xff;
	if (!qual) return BRC_FILTERED + 3;
	if (!n_ops) return BRC_FILTERED + 4;
	const uint8_t *c = rec + R.ops_at;
	uint64_t qsum = 0, rsum = 0, lead = 0, trail = 0;
	bool in_lead = true;
	for (uint32_t i = 0; i < n_ops; ++i) {
		const uint32_t v = bsr_u32(c + 4 * i), op = v & 15u; const uint64_t len = v >> 4;
		if (brc_op_query(op)) qsum += len;
		if (brc_op_ref(op)) rsum += len;
		if (!len || op == 5 || op == 6) continue;                      // (beside a clip, H and P stand for nothing)
		if (op == 4) { if (in_lead) lead += len; else trail += len; }
		else { in_lead = false; trail = 0; }
	}
	if (qsum != l_seq) return BRC_E_SUM;
	bool cg; uint8_t rg_type; uint64_t rg_at;
	const bool walked = brc_tags(rec, size, tags_at, &cg, &rg_type, &rg_at);
	if (walked && cg && n_ops == 2) {
		const uint32_t a = bsr_u32(c), b = bsr_u32(c + 4);
		if ((a & 15u) == 4u && (a >> 4) == l_seq && (b & 15u) == 3u) return BRC_E_PLACEHOLDER;
	}
	const int64_t pos = bsr_pos(rec);
	if (pos < 0 || (uint64_t)pos + rsum > (uint64_t)F.clen[ref]) return BRC_E_SPAN;
	if (!walked) return BRC_E_TAGS;
	R.group = 0;
	if (P.has_groups) {
		if (!rg_type) return BRC_E_RG_NONE;
		if (rg_type != 'Z') return BRC_E_RG_TYPE;
		const int g = brc_group_of(rec + rg_at, P, F);
		if (g < 0) return BRC_E_RG_ID;
		R.group = (uint32_t)g;
	}
	R.s0 = (uint32_t)lead; R.n = (uint32_t)(l_seq - lead - trail);      // (in_lead to the end: every base is clipped, trail is 0 and n is 0)
	R.pos = (int32_t)pos; R.gpos = F.coff[ref] + (uint64_t)pos;
	R.rev = (flag & 0x10u) != 0; R.neg = (flag & 0x81u) == 0x81u;
	return BRC_OK;
}

BRC_FN void brc_cur_begin(brc_cur_t &C) { C.k = 0; C.q0 = C.r0 = 0; C.op = 15; C.len = 0; }

// C -> the operation that holds the stored base i (i at or behind the base of the call before; brc_prep has seen the lengths sum to l_seq)
BRC_FN void brc_cur_seek(const uint8_t *rec, const brc_rec_t &R, uint64_t i, brc_cur_t &C)
{
	const uint8_t *c = rec + R.ops_at;
	if (C.len && i < C.q0 + C.len) return;
	if (C.len) { C.q0 += C.len; if (brc_op_ref(C.op)) C.r0 += C.len; ++C.k; C.len = 0; }
	for (; C.k < R.n_ops; ++C.k) {
		const uint32_t v = bsr_u32(c + 4 * C.k), op = v & 15u; const uint64_t len = v >> 4;
		if (brc_op_query(op)) {
			if (len && i < C.q0 + len) { C.op = op; C.len = len; return; }
			C.q0 += len;
		}
		if (brc_op_ref(op)) C.r0 += len;
	}
}

// what stands between the operation k and the next (dir 1) or the one before (dir -1) that holds stored bases: *del: a D; the return: that operation's code, 15: none
BRC_FN uint32_t brc_neighbour(const uint8_t *rec, const brc_rec_t &R, uint32_t k, int dir, bool *del)
{
	const uint8_t *c = rec + R.ops_at;
	*del = false;
	for (int64_t j = (int64_t)k + dir; j >= 0 && j < (int64_t)R.n_ops; j += dir) {
		const uint32_t v = bsr_u32(c + 4 * j), op = v & 15u;
		if (!(v >> 4)) continue;
		if (op == 2) *del = true;
		if (brc_op_query(op)) return op;
	}
	return 15u;
}

// the stored base i as A C G T = 0 .. 3, or -1
BRC_FN int brc_code(const uint8_t *rec, const brc_rec_t &R, uint64_t i)
{
	const uint32_t b = rec[R.seq_at + (i >> 1)] >> ((~i & 1u) << 2) & 15u;
	return b == 1 ? 0 : b == 2 ? 1 : b == 4 ? 2 : b == 8 ? 3 : -1;
}

// base k of the kept bases in sequencing order, or -1
BRC_FN int brc_seq_code(const uint8_t *rec, const brc_rec_t &R, uint32_t k)
{
	const int c = brc_code(rec, R, R.rev ? (uint64_t)R.s0 + R.n - 1 - k : (uint64_t)R.s0 + k);
	return c < 0 ? c : R.rev ? 3 - c : c;
}

// what an observed base adds
struct brc_obs_t { uint32_t q, ci, mctx, ictx; bool capped, snp, ins, del; };

// the stored base i (s0 <= i < s0 + n; C sought to i) -> 0 and o, or 1 .. 4: skipped for the reason BRC_SK_BASE - 1 + that
BRC_FN int brc_base(const uint8_t *rec, const brc_rec_t &R, const brc_plan_t &P, const brc_ref_t &F, uint64_t i, const brc_cur_t &C, brc_obs_t &o)
{
	const int code = brc_code(rec, R, i);
	if (code < 0) return 1;
	const uint32_t q = rec[R.qual_at + i];
	if ((int32_t)q < P.min_qual) return 2;
	const bool aligned = C.op == 0 || C.op == 7 || C.op == 8, inserted = C.op == 1;
	o.snp = false;
	if (aligned) {
		const uint64_t rp = R.gpos + C.r0 + (i - C.q0);
		if (brc_masked(F.mask, rp)) return 3;
		o.snp = brc_pac_base(F.pac, rp) != (uint32_t)code;
	} else if (inserted && (uint64_t)R.pos + C.r0 > 0 && brc_masked(F.mask, R.gpos + C.r0 - 1)) return 4;
	o.ins = o.del = false;
	if (!R.rev ? i == C.q0 + C.len - 1 : i == C.q0) {
		bool d;
		const uint32_t nb = brc_neighbour(rec, R, C.k, R.rev ? -1 : 1, &d);
		o.ins = !inserted && nb == 1u; o.del = d;
	}
	const uint32_t k = R.rev ? (uint32_t)((uint64_t)R.s0 + R.n - 1 - i) : (uint32_t)(i - R.s0);
	uint32_t cyc = k + 1;
	o.capped = cyc > (uint32_t)P.max_cycle;
	if (o.capped) cyc = (uint32_t)P.max_cycle;
	o.ci = R.neg ? (uint32_t)P.max_cycle - cyc : (uint32_t)P.max_cycle + cyc - 1;
	o.q = q < (uint32_t)BRC_NQ ? q : (uint32_t)BRC_NQ - 1;
	const int b1 = k >= 1 ? brc_seq_code(rec, R, k - 1) : -1, b2 = k >= 2 ? brc_seq_code(rec, R, k - 2) : -1;
	const int b0 = R.rev ? 3 - code : code;
	o.mctx = b1 < 0 ? 16u : (uint32_t)(4 * b1 + b0);
	o.ictx = b1 < 0 || b2 < 0 ? 64u : (uint32_t)(16 * b2 + 4 * b1 + b0);
	return 0;
}

BRC_FN uint64_t brc_refusal(uint64_t index, int code) { return index << 4 | (uint64_t)code; }
