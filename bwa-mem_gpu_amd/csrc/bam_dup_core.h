// Duplicate marking of BAM records (flag 0x400): the per-record and per-template rules of csrc/bam_dup_kernels.hip (one lane per record or template) and,
// compiled as plain C++, of csrc/bam_dup_host.cpp and tests/bam_dup_core_host.cpp (under the sanitizers).  They are Picard MarkDuplicates' rules with the open
// points fixed:
//
//   template  in the writer's order a record begins a template when it has neither 0x100 nor 0x800 and either 0x1 is clear or 0x40 is set (the writer puts a
//             read's primary line first and read 1's records before read 2's); a template's primary lines are its records without 0x100 / 0x800: one for an
//             unpaired read, two (0x40, 0x80) for a pair
//   end word  of a mapped primary line: u = the unclipped 5' coordinate -- forward: pos minus the leading S and H lengths; reverse: bsr_end - 1 plus the trailing
//             S and H lengths --, word = (uint64)refID << 32 | (uint32)(u + 2^30) << 1 | reverse: u + 2^30 must lie in [0, 2^31).  A record lies
//             inside its contig and this aligner clips at most 16 384 bases, so contigs of up to BDP_MAX_CONTIG = 2^30 - 2^24 bases (16 M of slack on either
//             side) keep it there; a run with a longer contig is refused before anything is marked (bsr_markdup_contigs).  Under a BAI index contigs stay
//             below 2^29 anyway
//   kind      pair: both primary lines mapped; fragment: an unpaired mapped read, or a pair with exactly one mapped primary line; none: everything else
//   score     the sum of the base qualities >= 15 over the template's primary lines; a record without qualities (first byte 0xff) scores 0
//   pairs     key (smaller end word, larger end word); among the pairs of one key the highest score stays, ties go to the smallest template ordinal (input
//             order over the whole run); all others are duplicates
//   fragments key: the end word; a duplicate if some pair has an end with that word, otherwise the best fragment at that word (score, then ordinal) stays
//   flagging  every record of a duplicate template gets 0x400 (byte 19 |= 0x04): primary, secondary and supplementary lines, the unmapped mate of a fragment
//
//   library   only when the run gives a table of (read group ID, library index): a template's library is that of the RG:Z tag on its first record.  The index
//             replaces the top 8 bits of both end words (above a refID below 2^24), so pairs are duplicates of each other, a fragment is a duplicate through a
//             pair's end, and the best fragment stays, within one library only -- keys of different libraries differ, the decision's passes do not change.
//             Without a table no tag is read and every byte is as it was
//
// No optical duplicates, no library-size estimate, nothing is removed.
#pragma once
#include "bam_sort_core.h"

enum { BDP_NONE = 0, BDP_FRAG = 1, BDP_PAIR = 2, BDP_QMIN = 15 };
enum { BDP_LIB_SHIFT = 56, BDP_MAX_LIBS = 255, BDP_MAX_REF = 1 << 24, BDP_MAX_CONTIG = (1 << 30) - (1 << 24) };
// what bdp_entry_lib says of a template
enum { BDP_E_OK = 0, BDP_E_TEMPLATE = 1, BDP_E_NO_RG = 2, BDP_E_RG_UNKNOWN = 3 };

// a run's read groups: the IDs back to back (no terminators) with offsets id_off [n + 1], and every group's library index (below BDP_MAX_LIBS)
struct bdp_groups_t { const char *ids; const uint32_t *id_off; const uint8_t *lib; uint32_t n; };

// one template: lo <= hi the end words of a pair, hi all ones for a fragment (both for kind none); kind_n: kind | records of the template << 2
struct bdp_entry_t { uint64_t lo, hi; uint32_t score, kind_n; };
static_assert(sizeof(bdp_entry_t) == 24, "an entry is 24 bytes");

BSR_FN uint32_t bdp_kind(const bdp_entry_t &e) { return e.kind_n & 3u; }
BSR_FN uint32_t bdp_n_rec(const bdp_entry_t &e) { return e.kind_n >> 2; }

BSR_FN bool bdp_primary(uint32_t flag) { return !(flag & 0x900u); }
BSR_FN bool bdp_head(uint32_t flag) { return bdp_primary(flag) && (!(flag & 1u) || (flag & 0x40u)); }

// do the bases and qualities the record announces lie inside its sz bytes (bsr_record_bytes has vouched for the name and the operations)
BSR_FN bool bdp_record_whole(const uint8_t *rec, uint64_t sz)
{
	const uint64_t l_seq = bsr_u32(rec + 20);
	return (uint64_t)BSR_FIXED + rec[12] + 4ull * bsr_u16(rec + 16) + (l_seq + 1) / 2 + l_seq <= sz;
}

// the end word of a mapped primary line
BSR_FN uint64_t bdp_end_word(const uint8_t *rec)
{
	const uint8_t *c = rec + BSR_FIXED + rec[12];
	const uint32_t n = bsr_u16(rec + 16), rev = (bsr_flag(rec) >> 4) & 1u;
	int64_t u;
	if (!rev) {
		u = bsr_pos(rec);
		for (uint32_t i = 0; i < n; ++i) { const uint32_t v = bsr_u32(c + 4 * i), op = v & 15u; if (op != 4 && op != 5) break; u -= v >> 4; }
	} else {
		u = bsr_end(rec) - 1;
		for (uint32_t i = n; i > 0; --i) { const uint32_t v = bsr_u32(c + 4 * (i - 1)), op = v & 15u; if (op != 4 && op != 5) break; u += v >> 4; }
	}
	return (uint64_t)bsr_u32(rec + 4) << 32 | (uint64_t)(uint32_t)(((uint32_t)u + (1u << 30)) << 1) | rev;
}

// the sum of the record's base qualities >= 15 (sz: the record's bytes; a record whose qualities do not lie inside them scores 0)
BSR_FN uint32_t bdp_score(const uint8_t *rec, uint64_t sz)
{
	if (!bdp_record_whole(rec, sz)) return 0;
	const uint32_t l_seq = bsr_u32(rec + 20);
	const uint8_t *q = rec + BSR_FIXED + rec[12] + 4u * bsr_u16(rec + 16) + (l_seq + 1) / 2;
	if (l_seq == 0 || q[0] == 0xff) return 0;
	uint64_t s = 0;
	for (uint32_t i = 0; i < l_seq; ++i) if (q[i] >= BDP_QMIN) s += q[i];
	return s > 0xffffffffull ? 0xffffffffu : (uint32_t)s;
}

// the entry of the template whose records are a .. b - 1 of a stream with offsets off [n + 1]; false: a paired template without both of its primary lines
BSR_FN bool bdp_entry(const uint8_t *recs, const uint64_t *off, uint32_t a, uint32_t b, bdp_entry_t *e)
{
	uint64_t w[2] = {0, 0}; uint32_t n_map = 0, n_pri = 0, seen = 0; uint64_t score = 0; bool paired = false;
	for (uint32_t i = a; i < b; ++i) {
		const uint8_t *rec = recs + off[i];
		const uint32_t fl = bsr_flag(rec);
		if (!bdp_primary(fl)) continue;
		++n_pri;
		if (fl & 1u) { paired = true; seen |= (fl & 0x40u ? 1u : 0u) | (fl & 0x80u ? 2u : 0u); }
		score += bdp_score(rec, off[i + 1] - off[i]);
		if (!(fl & 4u) && n_map < 2) w[n_map++] = bdp_end_word(rec);
	}
	e->score = score > 0xffffffffull ? 0xffffffffu : (uint32_t)score;
	e->lo = e->hi = ~0ull;
	uint32_t kind = BDP_NONE;
	const bool ok = paired ? (n_pri == 2 && seen == 3u) : n_pri == 1;
	if (ok) {
		if (n_map == 2) { kind = BDP_PAIR; e->lo = w[0] < w[1] ? w[0] : w[1]; e->hi = w[0] < w[1] ? w[1] : w[0]; }
		else if (n_map == 1) { kind = BDP_FRAG; e->lo = w[0]; }
	}
	e->kind_n = kind | (b - a) << 2;
	return ok;
}

// the sort words of the decision.  Pairs: third word -- better pairs first, then the earlier template
BSR_FN uint64_t bdp_rank_word(const bdp_entry_t &e, uint32_t ordinal) { return (uint64_t)(0xffffffffu - e.score) << 32 | ordinal; }
// the fragment pass's second word: pair ends (0) before fragments, those best-first (ordinals stay below 2^31)
BSR_FN uint64_t bdp_frag_word(const bdp_entry_t &e, uint32_t ordinal) { return bdp_kind(e) == BDP_PAIR ? 0ull : 1ull << 63 | (uint64_t)(0xffffffffu - e.score) << 31 | ordinal; }

// ---- libraries

BSR_FN uint32_t bdp_aux_width(uint8_t type) { return type == 'A' || type == 'c' || type == 'C' ? 1u : type == 's' || type == 'S' ? 2u : type == 'i' || type == 'I' || type == 'f' ? 4u : 0u; }

// the value of the record's RG:Z tag (its length in *len), found by a walk over the tags behind the qualities; nullptr: none, or tags that cannot be walked
BSR_FN const uint8_t *bdp_rg_tag(const uint8_t *rec, uint64_t sz, uint32_t *len)
{
	if (sz < BSR_FIXED || !bdp_record_whole(rec, sz)) return nullptr;
	const uint64_t l_seq = bsr_u32(rec + 20);
	uint64_t p = (uint64_t)BSR_FIXED + rec[12] + 4ull * bsr_u16(rec + 16) + (l_seq + 1) / 2 + l_seq;
	while (p + 3 <= sz) {
		const uint8_t t0 = rec[p], t1 = rec[p + 1], ty = rec[p + 2];
		p += 3;
		if (ty == 'Z' || ty == 'H') {
			uint64_t e = p;
			while (e < sz && rec[e]) ++e;
			if (e >= sz) return nullptr;
			if (t0 == 'R' && t1 == 'G' && ty == 'Z') { *len = (uint32_t)(e - p); return rec + p; }
			p = e + 1;
		} else if (ty == 'B') {
			if (p + 5 > sz) return nullptr;
			const uint32_t w = bdp_aux_width(rec[p]);
			if (!w) return nullptr;
			p += 5 + (uint64_t)w * bsr_u32(rec + p + 1);
		} else {
			const uint32_t w = bdp_aux_width(ty);
			if (!w) return nullptr;
			p += w;
		}
	}
	return nullptr;
}

// the library of the record's read group by the table (compared row by row: a run has a handful of groups); -1: no RG:Z tag, -2: an ID the table does not hold
BSR_FN int bdp_library(const uint8_t *rec, uint64_t sz, const bdp_groups_t &G)
{
	uint32_t len = 0;
	const uint8_t *id = bdp_rg_tag(rec, sz, &len);
	if (!id) return -1;
	for (uint32_t g = 0; g < G.n; ++g) {
		const uint32_t a = G.id_off[g];
		if (G.id_off[g + 1] - a != len) continue;
		uint32_t k = 0;
		while (k < len && (uint8_t)G.ids[a + k] == id[k]) ++k;
		if (k == len) return G.lib[g];
	}
	return -2;
}

BSR_FN uint64_t bdp_lib_word(uint64_t word, uint32_t lib) { return (word & ((1ull << BDP_LIB_SHIFT) - 1)) | (uint64_t)lib << BDP_LIB_SHIFT; }
// the library of an entry that bdp_entry_lib made
BSR_FN uint32_t bdp_lib_of(const bdp_entry_t &e) { return (uint32_t)(e.lo >> BDP_LIB_SHIFT); }

// bdp_entry with the library of the template's first record in the end words; BDP_E_*
BSR_FN int bdp_entry_lib(const uint8_t *recs, const uint64_t *off, uint32_t a, uint32_t b, const bdp_groups_t &G, bdp_entry_t *e)
{
	const bool ok = bdp_entry(recs, off, a, b, e);
	const int lib = bdp_library(recs + off[a], off[a + 1] - off[a], G);
	if (lib < 0) return lib == -1 ? BDP_E_NO_RG : BDP_E_RG_UNKNOWN;
	if (!ok) return BDP_E_TEMPLATE;
	e->lo = bdp_lib_word(e->lo, (uint32_t)lib);                            // (of every kind: a template that is neither pair nor fragment keeps its library here too, for the counts)
	if (bdp_kind(*e) == BDP_PAIR) e->hi = bdp_lib_word(e->hi, (uint32_t)lib);
	return BDP_E_OK;
}

// where a pair's or a fragment's entry counts among its library's five counters: examined (0 pairs, 1 fragments), and as a duplicate 2 / 3 and its records at 4
BSR_FN uint32_t bdp_examined_slot(const bdp_entry_t &e) { return bdp_kind(e) == BDP_PAIR ? 0u : 1u; }
