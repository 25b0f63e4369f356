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
//   optical   only when the run asks for it (an optical distance D): counts, never flags -- the records' bytes stay those of the run without it
//     location  of a template, from the read name of its first record (without the NUL): split at ':'; with exactly 5 or 7 fields tile, x and y are the last
//               three, any other field count gives none.  A field's value is its leading run of ASCII digits -- at least one, the value below 2^31; what
//               follows the digits is ignored (..:15343#ACGT parses, as with Picard's rapidParseInt).  No digit, a sign, or 2^31 and more: no location.  A
//               template without one is never an optical duplicate and joins no cluster
//     role      1 when the pair's smaller end word belongs to the 0x80 record and the two end words differ, else 0 (Picard's orientationForOpticalDuplicates:
//               copies of one cluster have the same mate on the same side)
//     group     the row of the RG:Z ID in the run's table (the row whose library the end words carry); 0 without a table
//     set       the pairs of one key (lo, hi), the one that stays included.  Sets of one pair, and sets of more than max_set pairs (300 000, Picard's
//               MAX_OPTICAL_DUPLICATE_SET_SIZE), are not examined; the latter are counted
//     edge      between two located pairs of a set: same group, same role, same tile, |x1 - x2| <= D and |y1 - y2| <= D (differences in 64 bits)
//     count     clusters are the connected components; a cluster of k pairs has k - 1 optical duplicates, so a set counts its located members minus their
//               components, whichever member stays.  In total and per library; fragments never count
//     size      bdp_library_size: Picard's estimateLibrarySize
//
//   barcode   only when the run asks for it (a tag XX, or the read name): templates with different molecular barcodes (UMIs) are no duplicates of each other
//     value     of a template, from its first record (the one the library and the location come from).  Tag: the value of tag XX of type Z, verbatim -- no case
//               folding, no splitting at '-': a dual UMI ACGT-TTGA is one value.  Name: the bytes behind the last ':' of the read name (without the NUL).  An
//               absent tag, an empty value, a name without ':' and a name that ends in ':' all mean no barcode; templates without one are comparable with each
//               other and with no barcoded template.  A tag XX of another type, and tags that cannot be walked, are refused by the record's index
//     word      64-bit FNV-1a over the value's bytes; 0 is kept for no barcode, so a value that hashes to 0 takes 1.  Words are compared, never strings
//     pairs     key (lo, hi, word); fragments: key (end word, word) -- a fragment is a duplicate through a pair's end only if that pair has its word
//     optical   a set is the pairs of one (lo, hi, word); in name mode the location is parsed from the name without its last field and that field's ':'
//
//   grouping  only when the run also asks for it (barcode edits N, 0 .. 21): barcodes within N mismatches are one molecule, as in Picard's
//             UmiAwareMarkDuplicatesWithMateCigar (MAX_EDIT_DISTANCE_TO_JOIN), with the open points fixed
//     word      the value itself, not its hash: 3 bits a byte -- A 1, C 2, G 3, T 4, N 5, '-' 6, '+' 7 --, symbol i in bits 3 i .. 3 i + 2, at most 21 symbols.  0
//               stays no barcode; the packing is injective, so equal words are equal values.  A first record whose value holds another byte (lower case too) or
//               more than 21 bytes is refused by the record's index.  The value's source, the no-barcode cases and the refused tags are those above
//     distance  the positions at which the symbols differ, separators like the rest; values of different lengths, and a template without a barcode and one with,
//               are never joined
//     pairs     within one (library, lo, hi) the distinct words are vertices, with an edge where the distance is <= N; the clusters are the connected components
//               (joining is transitive) and every pair takes the numerically smallest word of its component.  The pair rule then runs on (lo, hi, that word)
//     fragments the same within one (library, end word), over the distinct words of the pass's items -- the fragments and both ends of every pair, each under
//               its original word; the fragment rule then runs on (end word, the component's smallest word).  The two clusterings are independent
//     optical   a set is the pairs of one (lo, hi, the pair clustering's word)
//     cap       a key with more than max_set (65 536) distinct words is not clustered -- the walk is quadratic in them: its words stay exact, the key is counted
//     counts    in total and per library: the distinct (library, lo, hi, word) over barcoded pairs, the components of those, and the keys of either pass over the cap
//     clustering the union-find of the optical step over the distinct words in sorted order (key, then word): a root is its component's smallest word, and the
//               components do not depend on the order of the unions
//
// Nothing is removed, no DT:Z or MI:Z tag is written, edits are mismatches (no indels, no count-based direction), the names' pattern is fixed.
#pragma once
#include "bam_sort_core.h"

enum { BDP_NONE = 0, BDP_FRAG = 1, BDP_PAIR = 2, BDP_QMIN = 15 };
enum { BDP_LIB_SHIFT = 56, BDP_MAX_LIBS = 255, BDP_MAX_REF = 1 << 24, BDP_MAX_CONTIG = (1 << 30) - (1 << 24) };
// what bdp_entry_lib says of a template
enum { BDP_E_OK = 0, BDP_E_TEMPLATE = 1, BDP_E_NO_RG = 2, BDP_E_RG_UNKNOWN = 3, BDP_E_BC_TYPE = 4, BDP_E_BC_WALK = 5, BDP_E_BC_PACK = 6 };
// where a template begins: BDP_TPL_WRITER -- in the writer's order, by the flags (bdp_head); BDP_TPL_NAME -- where the read name changes (csrc/bam_post_core.h), for
// files of other programs, whose records of one name are adjacent in any order
enum { BDP_TPL_WRITER = 0, BDP_TPL_NAME = 1 };

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
// role (or NULL): the pair's role for optical duplicates
BSR_FN bool bdp_entry(const uint8_t *recs, const uint64_t *off, uint32_t a, uint32_t b, bdp_entry_t *e, uint32_t *role = nullptr)
{
	uint64_t w[2] = {0, 0}; uint32_t n_map = 0, n_pri = 0, seen = 0, second[2] = {0, 0}; uint64_t score = 0; bool paired = false;
	for (uint32_t i = a; i < b; ++i) {
		const uint8_t *rec = recs + off[i];
		const uint32_t fl = bsr_flag(rec);
		if (!bdp_primary(fl)) continue;
		++n_pri;
		if (fl & 1u) { paired = true; seen |= (fl & 0x40u ? 1u : 0u) | (fl & 0x80u ? 2u : 0u); }
		score += bdp_score(rec, off[i + 1] - off[i]);
		if (!(fl & 4u) && n_map < 2) { second[n_map] = (fl >> 7) & 1u; w[n_map++] = bdp_end_word(rec); }
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
	if (role) *role = kind == BDP_PAIR && w[0] != w[1] ? second[w[0] < w[1] ? 0 : 1] : 0u;
	return ok;
}

// the sort words of the decision.  Pairs: third word -- better pairs first, then the earlier template
BSR_FN uint64_t bdp_rank_word(const bdp_entry_t &e, uint32_t ordinal) { return (uint64_t)(0xffffffffu - e.score) << 32 | ordinal; }
// the fragment pass's second word: pair ends (0) before fragments, those best-first (ordinals stay below 2^31)
BSR_FN uint64_t bdp_frag_word(const bdp_entry_t &e, uint32_t ordinal) { return bdp_kind(e) == BDP_PAIR ? 0ull : 1ull << 63 | (uint64_t)(0xffffffffu - e.score) << 31 | ordinal; }

// ---- libraries

BSR_FN uint32_t bdp_aux_width(uint8_t type) { return type == 'A' || type == 'c' || type == 'C' ? 1u : type == 's' || type == 'S' ? 2u : type == 'i' || type == 'I' || type == 'f' ? 4u : 0u; }

// what bdp_aux_z says of a record's tags
enum { BDP_AUX_FOUND = 0, BDP_AUX_ABSENT = 1, BDP_AUX_TYPE = 2, BDP_AUX_WALK = 3, BDP_AUX_PACK = 4 };      // (PACK: bdp_barcode alone -- a value that does not pack)

// the value of the record's first tag t0 t1 of type Z (its length in *len), found by a walk over the tags behind the qualities.  *st: found; absent; a tag of
// that name and another type came first (the walk goes on: the value, if one follows, is still returned); or tags that cannot be walked (a cut tag, an unknown
// type, bytes left over) -- nullptr then, and when absent
BSR_FN const uint8_t *bdp_aux_z(const uint8_t *rec, uint64_t sz, uint8_t t0, uint8_t t1, uint32_t *len, int *st)
{
	*st = BDP_AUX_WALK;
	if (sz < BSR_FIXED || !bdp_record_whole(rec, sz)) return nullptr;
	const uint64_t l_seq = bsr_u32(rec + 20);
	uint64_t p = (uint64_t)BSR_FIXED + rec[12] + 4ull * bsr_u16(rec + 16) + (l_seq + 1) / 2 + l_seq;
	bool other = false;
	while (p + 3 <= sz) {
		const bool hit = rec[p] == t0 && rec[p + 1] == t1;
		const uint8_t ty = rec[p + 2];
		p += 3;
		if (ty == 'Z' || ty == 'H') {
			uint64_t e = p;
			while (e < sz && rec[e]) ++e;
			if (e >= sz) return nullptr;
			if (hit && ty == 'Z') { *len = (uint32_t)(e - p); *st = other ? BDP_AUX_TYPE : BDP_AUX_FOUND; return rec + p; }
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
		other = other || hit;
	}
	if (p == sz) *st = other ? BDP_AUX_TYPE : BDP_AUX_ABSENT;
	return nullptr;
}

// the value of the record's RG:Z tag (its length in *len); nullptr: none, or tags that cannot be walked
BSR_FN const uint8_t *bdp_rg_tag(const uint8_t *rec, uint64_t sz, uint32_t *len)
{
	int st;
	return bdp_aux_z(rec, sz, 'R', 'G', len, &st);
}

// the row of the record's read group in the table (compared row by row: a run has a handful of groups); -1: no RG:Z tag, -2: an ID the table does not hold
BSR_FN int bdp_group_row(const uint8_t *rec, uint64_t sz, const bdp_groups_t &G)
{
	uint32_t len = 0;
	const uint8_t *id = bdp_rg_tag(rec, sz, &len);
	if (!id) return -1;
	for (uint32_t g = 0; g < G.n; ++g) {
		const uint32_t a = G.id_off[g];
		if (G.id_off[g + 1] - a != len) continue;
		uint32_t k = 0;
		while (k < len && (uint8_t)G.ids[a + k] == id[k]) ++k;
		if (k == len) return (int)g;
	}
	return -2;
}
// the library of the record's read group; -1, -2 as bdp_group_row
BSR_FN int bdp_library(const uint8_t *rec, uint64_t sz, const bdp_groups_t &G) { const int g = bdp_group_row(rec, sz, G); return g < 0 ? g : (int)G.lib[g]; }

BSR_FN uint64_t bdp_lib_word(uint64_t word, uint32_t lib) { return (word & ((1ull << BDP_LIB_SHIFT) - 1)) | (uint64_t)lib << BDP_LIB_SHIFT; }
// the library of an entry that bdp_entry_lib made
BSR_FN uint32_t bdp_lib_of(const bdp_entry_t &e) { return (uint32_t)(e.lo >> BDP_LIB_SHIFT); }

// bdp_entry with the library of the template's first record in the end words; BDP_E_*
// role, row (or NULL): the pair's role and the table row of its read group, for optical duplicates
BSR_FN int bdp_entry_lib(const uint8_t *recs, const uint64_t *off, uint32_t a, uint32_t b, const bdp_groups_t &G, bdp_entry_t *e, uint32_t *role = nullptr, uint32_t *row = nullptr)
{
	const bool ok = bdp_entry(recs, off, a, b, e, role);
	const int g = bdp_group_row(recs + off[a], off[a + 1] - off[a], G);
	if (g < 0) return g == -1 ? BDP_E_NO_RG : BDP_E_RG_UNKNOWN;
	const int lib = G.lib[g];
	if (row) *row = (uint32_t)g;
	if (!ok) return BDP_E_TEMPLATE;
	e->lo = bdp_lib_word(e->lo, (uint32_t)lib);                            // (of every kind: a template that is neither pair nor fragment keeps its library here too, for the counts)
	if (bdp_kind(*e) == BDP_PAIR) e->hi = bdp_lib_word(e->hi, (uint32_t)lib);
	return BDP_E_OK;
}

// where a pair's or a fragment's entry counts among its library's five counters: examined (0 pairs, 1 fragments), and as a duplicate 2 / 3 and its records at 4
BSR_FN uint32_t bdp_examined_slot(const bdp_entry_t &e) { return bdp_kind(e) == BDP_PAIR ? 0u : 1u; }

// ---- optical duplicates

enum { BDP_LOC_LOCATED = 1, BDP_LOC_ROLE = 2, BDP_OPT_MAX_SET = 300000, BDP_OPT_MAX_GROUPS = 65536 };
// the three counts of the optical step: optical duplicate pairs, examined pairs with a location, sets skipped for their size
enum { BDP_OPT_DUPS = 0, BDP_OPT_LOCATED = 1, BDP_OPT_SKIPPED = 2, BDP_OPT_N = 3 };

// one template's place on the flow cell; flags: BDP_LOC_LOCATED | BDP_LOC_ROLE
struct bdp_loc_t { int32_t x, y; uint32_t tile; uint16_t rg, flags; };
static_assert(sizeof(bdp_loc_t) == 16, "a location is 16 bytes");

// the leading run of ASCII digits of p [n] -> *v; false: no digit first, or 2^31 and more
BSR_FN bool bdp_field_value(const uint8_t *p, uint32_t n, uint32_t *v)
{
	uint64_t x = 0; uint32_t k = 0;
	while (k < n && p[k] >= '0' && p[k] <= '9') {                      // (x stays below 2^31 before every step: no overflow)
		x = 10 * x + (uint32_t)(p[k] - '0');
		if (x >> 31) return false;
		++k;
	}
	*v = (uint32_t)x;
	return k > 0;
}

// tile, x, y of a read name (len bytes, no NUL) -> out [3]; false: no location
BSR_FN bool bdp_name_location(const uint8_t *name, uint32_t len, uint32_t out[3])
{
	uint32_t n_colon = 0, a0 = 0, a1 = 0, a2 = 0;                         // where the last three fields begin (scalars: nothing here is indexed, so nothing goes to scratch)
	for (uint32_t i = 0; i < len; ++i) if (name[i] == ':') { ++n_colon; a0 = a1; a1 = a2; a2 = i + 1; }
	if (n_colon != 4 && n_colon != 6) return false;
	uint32_t tile = 0, x = 0, y = 0;
	if (!bdp_field_value(name + a0, a1 - 1 - a0, &tile) || !bdp_field_value(name + a1, a2 - 1 - a1, &x) || !bdp_field_value(name + a2, len - a2, &y)) return false;
	out[0] = tile; out[1] = x; out[2] = y;
	return true;
}

// ---- barcodes

// where a run's barcodes come from: mode (BDP_BC_*) and, for a tag, its two letters; pack: the words are the packed values (grouping by edits), not hashes.
// Passed by value to the kernel
enum { BDP_BC_OFF = 0, BDP_BC_TAG = 1, BDP_BC_NAME = 2 };
struct bdp_bc_t { uint32_t mode; uint8_t t0, t1, pack; };
static_assert(sizeof(bdp_bc_t) == 8, "the barcode source is 8 bytes");

// the barcode word of a value of n bytes: 64-bit FNV-1a, one walk over the bytes; 0 is no barcode, so an empty value gives 0 and a value that hashes to 0 gives 1
BSR_FN uint64_t bdp_fnv1a64(const uint8_t *v, uint64_t n)       // (the hash alone: csrc/bam_collate_core.h keys read names with it)
{
	uint64_t h = 0xcbf29ce484222325ull;
	for (uint64_t i = 0; i < n; ++i) h = (h ^ v[i]) * 0x100000001b3ull;
	return h;
}
BSR_FN uint64_t bdp_barcode_word(const uint8_t *v, uint64_t n)
{
	if (!n) return 0;
	const uint64_t h = bdp_fnv1a64(v, n);
	return h ? h : 1ull;
}

// where the last field of a read name (len bytes, no NUL) begins: behind its last ':'; len + 1 for a name without one (no barcode, nothing to cut)
BSR_FN uint32_t bdp_name_last_field(const uint8_t *name, uint32_t len)
{
	uint32_t a = len + 1;
	for (uint32_t i = 0; i < len; ++i) if (name[i] == ':') a = i + 1;
	return a;
}

// the length of the name the location parser is given: in name mode the name without its last field and that field's ':'
BSR_FN uint32_t bdp_located_name_len(const uint8_t *name, uint32_t len, bool cut) { const uint32_t a = cut ? bdp_name_last_field(name, len) : len + 1; return a <= len ? a - 1 : len; }

// grouping by edits: the limits, and the three counts (distinct words of barcoded pairs, their components, keys over the cap)
enum { BDP_BC_SYMBOLS = 21, BDP_BC_MAX_EDITS = 21, BDP_BC_MAX_SET = 65536 };
enum { BDP_GRP_OBSERVED = 0, BDP_GRP_INFERRED = 1, BDP_GRP_SKIPPED = 2, BDP_GRP_N = 3 };

// a barcode byte's symbol; 0: a byte that does not pack
BSR_FN uint32_t bdp_bc_symbol(uint8_t c) { return c == 'A' ? 1u : c == 'C' ? 2u : c == 'G' ? 3u : c == 'T' ? 4u : c == 'N' ? 5u : c == '-' ? 6u : c == '+' ? 7u : 0u; }

// the packed word of a value of n bytes: symbol i in bits 3 i .. 3 i + 2; an empty value gives 0, no barcode.  false: more than 21 bytes, or a byte without a symbol
BSR_FN bool bdp_barcode_pack(const uint8_t *v, uint64_t n, uint64_t *word)
{
	*word = 0;
	if (n > BDP_BC_SYMBOLS) return false;
	uint64_t w = 0;
	for (uint32_t i = 0; i < (uint32_t)n; ++i) { const uint32_t s = bdp_bc_symbol(v[i]); if (!s) return false; w |= (uint64_t)s << 3 * i; }
	*word = w;
	return true;
}

// every 3-bit field of x folded to its lowest bit: set where the field is not 0
BSR_FN uint64_t bdp_bc_fold(uint64_t x) { return (x | x >> 1 | x >> 2) & 0x1249249249249249ull; }
// two packed words within N mismatches: the same places occupied (symbols are never 0, so that is the same length), and at most N fields of a ^ b not 0
BSR_FN bool bdp_bc_near(uint64_t a, uint64_t b, uint32_t N) { return bdp_bc_fold(a) == bdp_bc_fold(b) && (uint32_t)__builtin_popcountll(bdp_bc_fold(a ^ b)) <= N; }

// the barcode word of the template whose first record is rec (sz bytes; its name vouched for by bsr_record_bytes) -> *word; BDP_AUX_FOUND, or BDP_AUX_TYPE /
// BDP_AUX_WALK: the record is refused.  pack: the packed word, not the hash -- BDP_AUX_PACK: a value that does not pack
BSR_FN int bdp_barcode(const uint8_t *rec, uint64_t sz, const bdp_bc_t &bc, uint64_t *word, bool pack = false)
{
	*word = 0;
	if (bc.mode == BDP_BC_NAME) {
		if (sz < BSR_FIXED || sz - BSR_FIXED < rec[12]) return BDP_AUX_WALK;
		const uint32_t ln = rec[12] ? rec[12] - 1u : 0u, a = bdp_name_last_field(rec + BSR_FIXED, ln);
		if (a <= ln) { if (!pack) *word = bdp_barcode_word(rec + BSR_FIXED + a, ln - a); else if (!bdp_barcode_pack(rec + BSR_FIXED + a, ln - a, word)) return BDP_AUX_PACK; }
		return BDP_AUX_FOUND;
	}
	uint32_t len = 0; int st;                                           // (a record holds fewer than 2^32 bytes)
	const uint8_t *v = bdp_aux_z(rec, sz, bc.t0, bc.t1, &len, &st);
	if (st == BDP_AUX_TYPE || st == BDP_AUX_WALK) return st;
	if (v) { if (!pack) *word = bdp_barcode_word(v, len); else if (!bdp_barcode_pack(v, len, word)) return BDP_AUX_PACK; }
	return BDP_AUX_FOUND;
}

// the location of the template whose first record is rec (its name vouched for by bsr_record_bytes); cut: the barcode is the name's last field, which the parser
// does not see
BSR_FN bdp_loc_t bdp_location(const uint8_t *rec, uint32_t role, uint32_t row, bool cut = false)
{
	bdp_loc_t l; l.x = l.y = 0; l.tile = 0; l.rg = (uint16_t)row; l.flags = (uint16_t)(role ? BDP_LOC_ROLE : 0);
	uint32_t v[3];
	const uint32_t ln = rec[12];
	if (ln && bdp_name_location(rec + BSR_FIXED, bdp_located_name_len(rec + BSR_FIXED, ln - 1, cut), v)) { l.tile = v[0]; l.x = (int32_t)v[1]; l.y = (int32_t)v[2]; l.flags |= BDP_LOC_LOCATED; }
	return l;
}

// the sort words of the clustering: members of one set, group and role next to each other, there by tile, then x
BSR_FN uint64_t bdp_opt_word1(const bdp_loc_t &l) { return (uint64_t)l.tile << 32 | (uint32_t)l.x; }
BSR_FN uint64_t bdp_opt_word2(uint32_t set_head, const bdp_loc_t &l) { return (uint64_t)set_head << 17 | (uint64_t)l.rg << 1 | ((l.flags & BDP_LOC_ROLE) ? 1u : 0u); }

// Union-find over the members in sorted order.  The invariant: parent [v] <= v at all times, and a stored value only ever gets smaller -- so every find
// descends strictly and ends at a root (parent [v] == v) after at most v steps.  On the device the lanes share `parent` in global memory: a root is hooked with
// a compare-and-swap (only a root is hooked, and under a smaller index), paths are halved with an atomic minimum.
#if defined(__HIP_DEVICE_COMPILE__)
#define BDP_UF_LOAD(p) __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define BDP_UF_MIN(p, v) atomicMin(p, v)
#define BDP_UF_CAS(p, o, v) (atomicCAS(p, o, v) == (o))
#else
#define BDP_UF_LOAD(p) (*(p))
#define BDP_UF_MIN(p, v) do { if ((v) < *(p)) *(p) = (v); } while (0)
#define BDP_UF_CAS(p, o, v) (*(p) == (o) ? (*(p) = (v), true) : false)
#endif

BSR_FN uint32_t bdp_uf_find(uint32_t *parent, uint32_t v)
{
	for (;;) {                                                          // (every round ends or goes on at p < v)
		const uint32_t p = BDP_UF_LOAD(parent + v);
		if (p >= v) return v;                                         // (p == v: a root; p > v never is)
		const uint32_t g = BDP_UF_LOAD(parent + p);
		if (g < p) BDP_UF_MIN(parent + v, g);
		v = p;
	}
}

BSR_FN void bdp_uf_unite(uint32_t *parent, uint32_t a, uint32_t b)
{
	// every round either ends, or another lane's hook has taken a root away: roots only disappear, and there are finitely many
	for (;;) {
		a = bdp_uf_find(parent, a); b = bdp_uf_find(parent, b);
		if (a == b) return;
		if (a < b) { const uint32_t t = a; a = b; b = t; }               // the larger root goes under the smaller
		if (BDP_UF_CAS(parent + a, a, b)) return;
	}
}

// member i of n in sorted order (word2, then tile, then x): it walks j = i + 1 .. while set, group, role and tile are its own and x_j - x_i <= D, and unites with
// those whose y lies within D.  The walk ends at n at the latest: j only grows
BSR_FN void bdp_opt_walk(uint32_t i, uint32_t n, const uint64_t *word2, const uint32_t *tile, const int32_t *x, const int32_t *y, int64_t D, uint32_t *parent)
{
	const uint64_t w = word2[i]; const uint32_t t = tile[i]; const int64_t xi = x[i], yi = y[i];
	for (uint32_t j = i + 1; j < n; ++j) {
		if (word2[j] != w || tile[j] != t || (int64_t)x[j] - xi > D) break;
		const int64_t dy = (int64_t)y[j] - yi;
		if ((dy < 0 ? -dy : dy) <= D) bdp_uf_unite(parent, i, j);
	}
}

// member i of m distinct (key, word) in sorted order (key, then word): it walks the members j > i of its key and unites with those within N mismatches.  The walk
// ends at m at the latest: j only grows.  Indices ascend with the words inside a key, so a component's root is its smallest word
BSR_FN void bdp_bc_walk(uint32_t i, uint32_t m, const uint32_t *key, const uint64_t *word, uint32_t N, uint32_t *parent)
{
	const uint32_t k = key[i]; const uint64_t w = word[i];
	for (uint32_t j = i + 1; j < m && key[j] == k; ++j) if (bdp_bc_near(w, word[j], N)) bdp_uf_unite(parent, i, j);
}

// Picard's estimateLibrarySize: n pairs that are no optical duplicates, c of them distinct; 0: no estimate (the column stays empty)
inline int64_t bdp_library_size(uint64_t n_pairs, uint64_t n_unique, bool *has)
{
	*has = false;
	if (!(n_pairs > 0 && n_pairs > n_unique) || n_unique == 0) return 0;
	const double n = (double)n_pairs, c = (double)n_unique;
	auto f = [&](double x) { return c / x - 1 + __builtin_exp(-n / x); };
	double m = 1, M = 100;
	if (!(f(m * c) >= 0)) return 0;
	while (f(M * c) > 0) M *= 10;
	for (int i = 0; i < 40; ++i) {
		const double r = (m + M) / 2, u = f(r * c);
		if (u == 0) break;
		if (u > 0) m = r; else M = r;
	}
	*has = true;
	return (int64_t)(c * (m + M) / 2);
}
