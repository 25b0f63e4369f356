// Whole-file templates by name (BDP_TPL_FILE): the records of a file that carry one read name are one template, adjacent or not -- what a
// coordinate-sorted file needs before its duplicates can be marked.  The per-record part and the fold of a set of parts, for csrc/bam_tpl_kernels.hip (one lane per
// record, one lane per set) and, compiled as plain C++, for csrc/bam_tpl_host.cpp and tests/bam_tpl_core_host.cpp (under the sanitizers).
//
//   key       128 bits of a name: h0 = bdp_fnv1a64 over the name without its NUL (the mate collation's key), h1 = btp_hash1 over l_read_name and all its bytes --
//             another mixing step, another seed, the length folded in: no function of h0.  Names are never compared byte by byte (the records may have been spilled
//             by the time the sets are formed).  Two whole templates under one key hold two primary lines of one role, or paired and unpaired primary lines
//             together: the set is improper and refused, so a collision cannot make a wrong template silently.  hash_bits below 128 cuts the key (for the tests)
//   part      32 bytes per record: the key, the end word of a mapped primary line (else all ones), the score of a primary line (else 0), and one word of bits --
//             primary, paired, 0x40, 0x80, secondary or supplementary, unmapped (a mapped primary line: primary and not unmapped), the barcode's status, the
//             library byte and the group row of the record's RG:Z tag, all as they would count were the record its template's first.  A record without a usable
//             read group has the library byte BTP_NO_LIB and the row says why
//   fold      bdp_entry's rule on a set of parts given in file order: primary lines, paired, seen, the score summed over the primary lines, the end words of the
//             first two mapped primary lines, the kind; n_rec the size of the set; the role the 0x80 bit of the part that owns lo.  Library, group row, barcode
//             word and location are the first part's.  The verdict is the smallest BDP_E_* code that holds: all of a set's refusals name its first record
//   refusal   index << 3 | code over the whole file, the smallest wins (bpo_refusal): the index is the set's first record's
#pragma once
#include "bam_post_core.h"

enum { BDP_TPL_FILE = 2 };                                            // beside BDP_TPL_WRITER and BDP_TPL_NAME: templates by name over the whole file
enum { BTP_PRIMARY = 1, BTP_PAIRED = 2, BTP_FIRST = 4, BTP_SECOND = 8, BTP_SECSUP = 16, BTP_UNMAPPED = 32, BTP_BC_SHIFT = 6, BTP_LIB_SHIFT = 8, BTP_ROW_SHIFT = 16, BTP_NO_LIB = 255 };

struct btp_part_t { uint64_t h0, h1, end; uint32_t score, bits; };
static_assert(sizeof(btp_part_t) == 32, "a part is 32 bytes");

// the second hash: over l_read_name and the name's l bytes (the NUL with them)
BSR_FN uint64_t btp_hash1(const uint8_t *name, uint32_t l)
{
	uint64_t h = 0x9e3779b97f4a7c15ull ^ l;
	for (uint32_t i = 0; i < l; ++i) { h = (h ^ name[i]) * 0xff51afd7ed558ccdull; h ^= h >> 32; }
	h *= 0xc4ceb9fe1a85ec53ull;
	return h ^ h >> 29;
}

// the key cut to hash_bits (128: whole; 64 and below: h1 is 0)
BSR_FN void btp_cut(uint64_t *h0, uint64_t *h1, uint32_t hash_bits)
{
	if (hash_bits >= 128) return;
	if (hash_bits > 64) { *h1 &= (1ull << (hash_bits - 64)) - 1; return; }
	*h1 = 0;
	if (hash_bits < 64) *h0 &= (1ull << hash_bits) - 1;
}

BSR_FN bool btp_key_equal(const btp_part_t &a, const btp_part_t &b) { return a.h0 == b.h0 && a.h1 == b.h1; }
BSR_FN uint32_t btp_lib(const btp_part_t &p) { return (p.bits >> BTP_LIB_SHIFT) & 0xffu; }
BSR_FN uint32_t btp_row(const btp_part_t &p) { return p.bits >> BTP_ROW_SHIFT; }
BSR_FN bool btp_mapped(const btp_part_t &p) { return (p.bits & (BTP_PRIMARY | BTP_UNMAPPED)) == BTP_PRIMARY; }

// the part of a record that bpo_check has passed (whole inside its sz bytes).  G (or NULL): the run's read groups; bc (or NULL): its barcode source -- *bcw the
// record's barcode word; loc (or NULL): the record's location, role and row left 0 for the fold
BSR_FN btp_part_t btp_part(const uint8_t *rec, uint64_t sz, const bdp_groups_t *G, const bdp_bc_t *bc, uint64_t *bcw, bdp_loc_t *loc, uint32_t hash_bits)
{
	btp_part_t p;
	const uint32_t fl = bsr_flag(rec), l = rec[12];
	p.h0 = bdp_fnv1a64(rec + BSR_FIXED, l ? l - 1 : 0); p.h1 = btp_hash1(rec + BSR_FIXED, l);
	btp_cut(&p.h0, &p.h1, hash_bits);
	const bool pri = bdp_primary(fl);
	p.end = pri && !(fl & 4u) ? bdp_end_word(rec) : ~0ull;
	p.score = pri ? bdp_score(rec, sz) : 0u;
	uint32_t bits = (pri ? BTP_PRIMARY : 0u) | (fl & 1u ? BTP_PAIRED : 0u) | (fl & 0x40u ? BTP_FIRST : 0u) | (fl & 0x80u ? BTP_SECOND : 0u) | (fl & 0x900u ? BTP_SECSUP : 0u) | (fl & 4u ? BTP_UNMAPPED : 0u);
	if (G) {
		const int g = bdp_group_row(rec, sz, *G);
		if (g < 0) bits |= (uint32_t)BTP_NO_LIB << BTP_LIB_SHIFT | (uint32_t)(g == -1 ? BDP_E_NO_RG : BDP_E_RG_UNKNOWN) << BTP_ROW_SHIFT;
		else bits |= (uint32_t)G->lib[g] << BTP_LIB_SHIFT | (uint32_t)g << BTP_ROW_SHIFT;
	}
	if (bc) {
		const int bs = bdp_barcode(rec, sz, *bc, bcw, bc->pack != 0);
		bits |= (uint32_t)(bs == BDP_AUX_FOUND ? 0 : bs == BDP_AUX_TYPE ? 1 : bs == BDP_AUX_WALK ? 2 : 3) << BTP_BC_SHIFT;
	}
	if (loc) *loc = bdp_location(rec, 0, 0, bc && bc->mode == BDP_BC_NAME);
	p.bits = bits;
	return p;
}

// what a refused set holds, for the message: its primary lines, those with 0x40, those with 0x80, and whether one of them is paired
struct btp_lines_t { uint32_t n_pri, n_first, n_second, paired; };

// The m parts P [mem [k]], mem ascending (file order), as one template -> *e; BDP_E_*.  groups, barcode: the run has read groups / a barcode source (their bits
// are read).  role (or NULL): the pair's role; lines (or NULL): the counts of the primary lines
BSR_FN int btp_fold(const btp_part_t *P, const uint32_t *mem, uint32_t m, bool groups, bool barcode, bdp_entry_t *e, uint32_t *role = nullptr, btp_lines_t *lines = nullptr)
{
	uint64_t w[2] = {0, 0}, score = 0; uint32_t n_map = 0, n_pri = 0, n_first = 0, n_second = 0, second[2] = {0, 0}; bool paired = false;
	for (uint32_t k = 0; k < m; ++k) {
		const btp_part_t &p = P[mem[k]];
		if (!(p.bits & BTP_PRIMARY)) continue;
		++n_pri;
		if (p.bits & BTP_PAIRED) { paired = true; if (p.bits & BTP_FIRST) ++n_first; if (p.bits & BTP_SECOND) ++n_second; }
		score += p.score;
		if (btp_mapped(p) && n_map < 2) { second[n_map] = p.bits & BTP_SECOND ? 1u : 0u; w[n_map++] = p.end; }
	}
	if (lines) { lines->n_pri = n_pri; lines->n_first = n_first; lines->n_second = n_second; lines->paired = paired; }
	e->score = score > 0xffffffffull ? 0xffffffffu : (uint32_t)score;
	e->lo = e->hi = ~0ull;
	uint32_t kind = BDP_NONE;
	const bool ok = paired ? (n_pri == 2 && n_first >= 1 && n_second >= 1) : n_pri == 1;          // (bdp_entry's: two primary lines that show 0x40 and 0x80 between them)
	if (ok) {
		if (n_map == 2) { kind = BDP_PAIR; e->lo = w[0] < w[1] ? w[0] : w[1]; e->hi = w[0] < w[1] ? w[1] : w[0]; }
		else if (n_map == 1) { kind = BDP_FRAG; e->lo = w[0]; }
	}
	e->kind_n = kind | m << 2;
	if (role) *role = kind == BDP_PAIR && w[0] != w[1] ? second[w[0] < w[1] ? 0 : 1] : 0u;
	if (!ok) return BDP_E_TEMPLATE;
	const btp_part_t &f = P[mem[0]];
	if (groups) {
		const uint32_t lib = btp_lib(f);
		if (lib == BTP_NO_LIB) return (int)btp_row(f);                     // (BDP_E_NO_RG or BDP_E_RG_UNKNOWN)
		e->lo = bdp_lib_word(e->lo, lib);
		if (kind == BDP_PAIR) e->hi = bdp_lib_word(e->hi, lib);
	}
	if (barcode) { const uint32_t bs = (f.bits >> BTP_BC_SHIFT) & 3u; if (bs) return bs == 1 ? BDP_E_BC_TYPE : bs == 2 ? BDP_E_BC_WALK : BDP_E_BC_PACK; }
	return BDP_E_OK;
}

// the location of the template whose first record has the location l: the fold's role and the first part's row go in
BSR_FN bdp_loc_t btp_location(bdp_loc_t l, uint32_t role, const btp_part_t &first, bool groups)
{
	l.rg = (uint16_t)(groups ? btp_row(first) : 0u);
	l.flags = (uint16_t)((l.flags & BDP_LOC_LOCATED) | (role ? BDP_LOC_ROLE : 0));
	return l;
}
