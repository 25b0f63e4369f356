// Applying a recalibration table to the base qualities: the per-record and per-base rules of csrc/bam_requal_kernels.hip (a group of lanes per
// record) and, compiled as plain C++, of the host form in csrc/bam_requal.h and of tests/bam_requal_core_host.cpp (under the sanitizers).  Both forms read the same
// int16 tables, made once on the host, so they give the same bytes whatever the device's or the host's logarithm does.
//
//   tables    t [group][quality 0 .. 93][row]: a row is b, then the 2 max_cycle cycle deltas c (slot max_cycle + cy - 1 for cycle cy > 0, max_cycle + cy for
//             cy < 0), then the 16 context deltas x -- all in 1/256 of a quality
//   rewritten every record with qualities (l_seq > 0 and not all 0xff: brc_prep's rule), whatever its flags; a record without them is passed over before its tags
//             are read
//   refused   by the record's index, in this order: a record whose bytes do not hold what it announces; with a group table tags that cannot be walked to the
//             record's end, no RG tag, an RG tag of another type than Z, an ID the table does not hold
//   cycle     of stored base i of l_seq: k + 1 with k = i (forward) or l_seq - 1 - i (0x10), negated with 0x1 and 0x80; magnitudes above max_cycle share
//             max_cycle.  No clip is removed: the position in the whole read is the machine's cycle
//   context   sequencing-order bases k - 1, k as 4 a + b (A C G T = 0 1 2 3, complemented for 0x10); none when k = 0 or one of them is no ACGT
//   quality   below min_qual: unchanged.  Else, looked up as min(q, 93): clamp((b + c + x + 128) >> 8, 1, 93), x = 0 without a context
#pragma once
#include <stdint.h>
#include "bam_recal_core.h"

#define BRQ_FN BRC_FN

enum { BRQ_SEEN = 0, BRQ_REWRITTEN, BRQ_NOQUAL, BRQ_BASES, BRQ_LOW, BRQ_CHANGED, BRQ_UNCHANGED, BRQ_CAPPED, BRQ_NOCTX, BRQ_N_SUM = 16, BRQ_HIST = 2 * BRC_NQ, BRQ_WORDS = BRQ_N_SUM + BRQ_HIST };
enum { BRQ_SKIP = 16, BRQ_CTX = 16, BRQ_MAX_Q = BRC_NQ - 1 };

struct brq_plan_t {
	int32_t n_groups, has_groups, min_qual, max_cycle;
	BRQ_FN uint32_t row() const { return 1u + 2u * (uint32_t)max_cycle + (uint32_t)BRQ_CTX; }
	BRQ_FN uint64_t entries() const { return (uint64_t)n_groups * BRC_NQ * row(); }
	BRQ_FN uint64_t at(uint32_t g, uint32_t q) const { return ((uint64_t)g * BRC_NQ + q) * row(); }
};

// the tables and the group IDs as both forms read them (rg: the IDs back to back with their NULs, rg_off [n_groups + 1])
struct brq_tab_t { const int16_t *t; const char *rg; const uint32_t *rg_off; };

// a record with qualities, ready for its bases
struct brq_rec_t { uint64_t seq_at, qual_at; uint32_t l_seq, group; bool rev, neg; };

// the record of `size` bytes -> BRC_OK and R (rewritten), BRQ_SKIP (no qualities), or why it is refused (brc_prep's codes)
BRQ_FN int brq_prep(const uint8_t *rec, uint64_t size, const brq_plan_t &P, const brq_tab_t &T, brq_rec_t &R)
{
	if (size < BSR_FIXED) return BRC_E_CUT;
	const uint32_t flag = bsr_flag(rec);
	const uint64_t l_seq = bsr_u32(rec + 20);
	R.seq_at = (uint64_t)BSR_FIXED + rec[12] + 4ull * bsr_u16(rec + 16); R.qual_at = R.seq_at + (l_seq + 1) / 2;
	const uint64_t tags_at = R.qual_at + l_seq;
	if (tags_at > size) return BRC_E_CUT;
	bool qual = false;
	for (uint64_t i = 0; i < l_seq && !qual; ++i) qual = rec[R.qual_at + i] != 0xff;
	if (!qual) return BRQ_SKIP;
	R.group = 0;
	if (P.has_groups) {
		bool cg; uint8_t rg_type; uint64_t rg_at;
		if (!brc_tags(rec, size, tags_at, &cg, &rg_type, &rg_at)) return BRC_E_TAGS;
		if (!rg_type) return BRC_E_RG_NONE;
		if (rg_type != 'Z') return BRC_E_RG_TYPE;
		brc_plan_t bp; bp.n_contigs = 0; bp.n_groups = P.n_groups; bp.has_groups = 1; bp.min_qual = P.min_qual; bp.max_cycle = P.max_cycle;
		const brc_ref_t F = {nullptr, nullptr, nullptr, nullptr, T.rg, T.rg_off};
		const int g = brc_group_of(rec + rg_at, bp, F);
		if (g < 0) return BRC_E_RG_ID;
		R.group = (uint32_t)g;
	}
	R.l_seq = (uint32_t)l_seq;
	R.rev = (flag & 0x10u) != 0; R.neg = (flag & 0x81u) == 0x81u;
	return BRC_OK;
}

// the stored base i as A C G T = 0 .. 3, or -1
BRQ_FN int brq_code(const uint8_t *rec, const brq_rec_t &R, uint64_t i)
{
	const uint32_t b = rec[R.seq_at + (i >> 1)] >> ((~i & 1u) << 2) & 15u;
	return b == 1 ? 0 : b == 2 ? 1 : b == 4 ? 2 : b == 8 ? 3 : -1;
}

// what a base adds to the counts beside its two histogram bins
struct brq_obs_t { bool low, capped, noctx; };

// the stored base i (i < l_seq) whose quality is q0 -> its new quality
BRQ_FN uint32_t brq_base(const uint8_t *rec, const brq_rec_t &R, const brq_plan_t &P, const int16_t *t, uint64_t i, uint32_t q0, brq_obs_t &o)
{
	o.low = (int32_t)q0 < P.min_qual; o.capped = o.noctx = false;
	if (o.low) return q0;
	const uint32_t q = q0 < (uint32_t)BRQ_MAX_Q ? q0 : (uint32_t)BRQ_MAX_Q, C = (uint32_t)P.max_cycle;
	const uint64_t k = R.rev ? (uint64_t)R.l_seq - 1 - i : i;
	o.capped = k + 1 > C;
	const uint32_t cyc = o.capped ? C : (uint32_t)k + 1u;
	const uint32_t ci = R.neg ? C - cyc : C + cyc - 1;
	int ctx = -1;
	if (k > 0) {
		const int b = brq_code(rec, R, i), a = brq_code(rec, R, R.rev ? i + 1 : i - 1);
		if (a >= 0 && b >= 0) ctx = R.rev ? 4 * (3 - a) + (3 - b) : 4 * a + b;
	}
	o.noctx = ctx < 0;
	const int16_t *row = t + P.at(R.group, q);
	const int32_t v = (int32_t)row[0] + (int32_t)row[1u + ci] + (ctx < 0 ? 0 : (int32_t)row[1u + 2u * C + (uint32_t)ctx]);
	const int32_t n = (v + 128) >> 8;                                  // (arithmetic: the sum may be negative)
	return (uint32_t)(n < 1 ? 1 : n > (int32_t)BRQ_MAX_Q ? (int32_t)BRQ_MAX_Q : n);
}
