// Duplicate marking on the host (csrc/bam_dup_core.h's rules): the templates' entries of a record stream, the decision (std::sort where the device runs radix
// passes), the flags, and bmh_bam_markdup_host.  Byte for byte what csrc/bam_dup_kernels.hip gives.
#include <stdlib.h>
#include <string.h>
#include <assert.h>
#include <algorithm>
#include <numeric>
#include "bam_dup.h"
#include "bam_post_core.h"
#ifndef BDP_STANDALONE
#include "bam_sort.h"
#endif

int bdp_batch_refused(uint32_t n, uint32_t bad, const char *fn)
{
	if (bad > n) bmh_set_error("%s: duplicate marking: the stream's first record begins no template (a secondary or supplementary line, or read 2 of a pair)", fn);
	else bmh_set_error("%s: duplicate marking: the template that begins at record %u is paired and lacks one of its two primary lines (0x40, 0x80)", fn, bad - 1);
	return BMH_EINVAL;
}

int bdp_group_refused(uint32_t rec, int st, const char *fn)
{
	if (st == BDP_E_NO_RG) bmh_set_error("%s: duplicate marking: record %u begins a template and carries no RG:Z tag (read groups were given: every template's library comes from that tag)", fn, rec);
	else bmh_set_error("%s: duplicate marking: record %u begins a template and names a read group that is not among those given", fn, rec);
	return BMH_EINVAL;
}

int bdp_barcode_refused(uint32_t rec, int st, const char *fn)
{
	if (st == BDP_E_BC_TYPE) bmh_set_error("%s: duplicate marking: record %u begins a template and carries the barcode tag with a type other than Z", fn, rec);
	else if (st == BDP_E_BC_PACK) bmh_set_error("%s: duplicate marking: record %u begins a template and its barcode does not pack for grouping by edits: more than %d bytes, or a byte other than A C G T N - +", fn, rec, (int)BDP_BC_SYMBOLS);
	else bmh_set_error("%s: duplicate marking: record %u begins a template and its tags cannot be walked to the barcode tag (a cut tag, an unknown type, or bytes left over)", fn, rec);
	return BMH_EINVAL;
}

int bdp_barcode_check(int mode, const char *tag, const char *fn, bdp_bc_t *bc)
{
	bc->mode = BDP_BC_OFF; bc->t0 = bc->t1 = bc->pack = 0;
	if (mode != BDP_BC_OFF && mode != BDP_BC_TAG && mode != BDP_BC_NAME) { bmh_set_error("%s: barcode mode %d (0: none, 1: a tag, 2: the read name)", fn, mode); return BMH_EINVAL; }
	if (mode == BDP_BC_TAG) {
		if (!tag) { bmh_set_error("%s: a barcode tag has two characters, [A-Za-z][A-Za-z0-9]", fn); return BMH_EINVAL; }
		const char a = tag[0], b = a ? tag[1] : 0;
		const bool ok = ((a >= 'A' && a <= 'Z') || (a >= 'a' && a <= 'z')) && ((b >= 'A' && b <= 'Z') || (b >= 'a' && b <= 'z') || (b >= '0' && b <= '9'));
		if (!ok) { bmh_set_error("%s: a barcode tag has two characters, [A-Za-z][A-Za-z0-9]", fn); return BMH_EINVAL; }
		static const char own[8][3] = {"RG", "NM", "MD", "AS", "XS", "SA", "XA", "pa"};
		for (const char *o : own)
			if (a == o[0] && b == o[1]) { bmh_set_error("%s: tag %c%c cannot be a barcode: RG names the read group, and NM MD AS XS SA XA pa are written by the aligner itself", fn, a, b); return BMH_EINVAL; }
		bc->t0 = (uint8_t)a; bc->t1 = (uint8_t)b;
	}
	bc->mode = (uint32_t)mode;
	return BMH_OK;
}

int bdp_group_check(int edits, uint64_t max_set, const char *fn, bdp_bc_t *bc)
{
	bc->pack = 0;
	if (edits == -1) return BMH_OK;
	if (edits < 0 || edits > (int)BDP_BC_MAX_EDITS) { bmh_set_error("%s: barcode edits of %d (0 .. %d)", fn, edits, (int)BDP_BC_MAX_EDITS); return BMH_EINVAL; }
	if (bc->mode == BDP_BC_OFF) { bmh_set_error("%s: barcode edits group the barcodes that are compared: they need a barcode source (a tag or the read name)", fn); return BMH_EINVAL; }
	if (max_set > 0x7fffffffull) { bmh_set_error("%s: a largest key of %llu distinct barcodes (below 2^31; 0: %d)", fn, (unsigned long long)max_set, (int)BDP_BC_MAX_SET); return BMH_EINVAL; }
	bc->pack = 1;
	return BMH_OK;
}

uint64_t bdp_no_barcode(const uint64_t *B, uint64_t T) { uint64_t c = 0; for (uint64_t t = 0; t < T; ++t) c += B[t] == 0; return c; }

int bdp_batch_verdict(uint32_t n, const uint32_t *info, bool groups, bool barcode, bool pack, uint32_t *bad_out)
{
	*bad_out = 0;
	if (!n) return BDP_E_OK;
	// (the smallest record index wins, as a walk from the front would find it)
	if (info[1] == 0) { *bad_out = n + 1; return BDP_E_TEMPLATE; }
	uint32_t bad = info[1]; int st = BDP_E_TEMPLATE;
	if (groups) for (int k = 0; k < 2; ++k) if (info[4 + k] < bad) { bad = info[4 + k]; st = k ? BDP_E_RG_UNKNOWN : BDP_E_NO_RG; }
	if (barcode) for (int k = 0; k < 2; ++k) if (info[6 + k] < bad) { bad = info[6 + k]; st = k ? BDP_E_BC_WALK : BDP_E_BC_TYPE; }
	if (barcode && pack && info[8] < bad) { bad = info[8]; st = BDP_E_BC_PACK; }
	if (bad == 0xffffffffu) return BDP_E_OK;
	*bad_out = bad;
	return st;
}

int bdp_batch_check(uint32_t n, const uint32_t *info, bool groups, const char *fn, bool barcode, bool pack)
{
	uint32_t bad = 0;
	const int st = bdp_batch_verdict(n, info, groups, barcode, pack, &bad);
	if (st == BDP_E_OK) return BMH_OK;
	return st == BDP_E_TEMPLATE ? bdp_batch_refused(n, bad, fn) : st >= BDP_E_BC_TYPE ? bdp_barcode_refused(bad - 1, st, fn) : bdp_group_refused(bad - 1, st, fn);
}

int bdp_name_refused(uint64_t rec, const char *fn)
{
	bmh_set_error("%s: duplicate marking: the records under the read name of record %llu, which lie next to each other, are paired and are not one 0x40 and one 0x80 primary line: "
	              "marking needs the records of a read name next to each other (a coordinate-sorted file has them apart: sort it by name first, or realign it with --collate); "
	              "`python -m bwamem_hip.bam --markdup --collate` marks such a file as it is", fn, (unsigned long long)rec);
	return BMH_EINVAL;
}

int bdp_table_make(bdp_table_t &T, const char *const *ids, const int32_t *lib, int n, const char *fn)
{
	T.ids.clear(); T.id_off.assign(1, 0); T.lib.clear(); T.n_lib = 0;
	if (n < 1 || !ids || !lib) { bmh_set_error("%s: no read groups were given", fn); return BMH_EINVAL; }
	for (int g = 0; g < n; ++g) {
		if (!ids[g] || !ids[g][0]) { bmh_set_error("%s: read group %d has no ID", fn, g); return BMH_EINVAL; }
		for (int k = 0; k < g; ++k)
			if (!strcmp(ids[k], ids[g])) { bmh_set_error("%s: read groups %d and %d share the ID '%s'", fn, k, g, ids[g]); return BMH_EINVAL; }
		if (lib[g] < 0 || lib[g] >= BDP_MAX_LIBS) {
			bmh_set_error("%s: read group %d ('%s') is of library %d: a run holds at most %d libraries (the library is a byte of the duplicate key)", fn, g, ids[g], lib[g], (int)BDP_MAX_LIBS);
			return BMH_EINVAL;
		}
		T.ids += ids[g]; T.id_off.push_back((uint32_t)T.ids.size()); T.lib.push_back((uint8_t)lib[g]);
		if ((uint32_t)lib[g] + 1 > T.n_lib) T.n_lib = (uint32_t)lib[g] + 1;
	}
	return BMH_OK;
}

int bdp_refs_fit(const uint8_t *recs, const uint64_t *off, uint32_t n, const char *fn)
{
	for (uint32_t i = 0; i < n; ++i)
		if (bsr_ref(recs + off[i]) >= (int32_t)BDP_MAX_REF) {
			bmh_set_error("%s: duplicate marking: record %u names reference %d: with read groups references stay below 2^24 (the library takes the key's top byte)", fn, i, bsr_ref(recs + off[i]));
			return BMH_EINVAL;
		}
	return BMH_OK;
}

int bdp_entries_host(const uint8_t *recs, const uint64_t *off, uint32_t n, std::vector<uint32_t> &tpl, std::vector<bdp_entry_t> &entries, uint64_t info[2], const char *fn, const bdp_plan_t &P,
                     std::vector<bdp_loc_t> *locs, std::vector<uint64_t> *bcs, int tpl_rule, uint64_t rec_base)
{
	const bool by_name = tpl_rule == BDP_TPL_NAME;
	const bdp_bc_t *bc = bcs ? P.barcode() : nullptr;
	const bdp_groups_t G = P.table.view();
	tpl.resize(n); entries.clear();
	if (locs) locs->clear();
	if (bcs) bcs->clear();
	if (n && !by_name && !bdp_head(bsr_flag(recs + off[0]))) return bdp_batch_refused(n, n + 1, fn);
	std::vector<uint32_t> start;
	for (uint32_t i = 0; i < n; ++i) {
		const uint32_t fl = bsr_flag(recs + off[i]);
		if (by_name ? bpo_head(recs, off, i) : bdp_head(fl)) start.push_back(i);
		tpl[i] = (uint32_t)start.size() - 1;
		if (fl & 0x900u) ++info[0];
		if (fl & 4u) ++info[1];
	}
	if (start.size() >= 1ull << 31) { bmh_set_error("%s: duplicate marking: 2^31 templates", fn); return BMH_EINVAL; }
	entries.resize(start.size());
	if (locs) locs->resize(start.size());
	if (bc) bcs->resize(start.size());
	for (size_t t = 0; t < start.size(); ++t) {
		const uint32_t a = start[t], b = t + 1 < start.size() ? start[t + 1] : n;
		uint32_t role = 0, row = 0;
		const int st = P.groups() ? bdp_entry_lib(recs, off, a, b, G, &entries[t], &role, &row) : bdp_entry(recs, off, a, b, &entries[t], &role) ? BDP_E_OK : BDP_E_TEMPLATE;
		if (st == BDP_E_TEMPLATE) return by_name ? bdp_name_refused(rec_base + a, fn) : bdp_batch_refused(n, a + 1, fn);
		if (st != BDP_E_OK) return bdp_group_refused((uint32_t)(rec_base + a), st, fn);
		if (locs) (*locs)[t] = bdp_location(recs + off[a], role, row, bc && bc->mode == BDP_BC_NAME);
		if (bc) {
			const int bs = bdp_barcode(recs + off[a], off[a + 1] - off[a], *bc, &(*bcs)[t], bc->pack != 0);
			if (bs != BDP_AUX_FOUND) return bdp_barcode_refused((uint32_t)(rec_base + a), bs ==BDP_AUX_TYPE ? BDP_E_BC_TYPE : bs == BDP_AUX_PACK ? BDP_E_BC_PACK : BDP_E_BC_WALK, fn);
		}
	}
	return BMH_OK;
}

void bdp_group_host(const bdp_entry_t *E, uint64_t T, const uint64_t *B, const bdp_group_t &G, uint32_t n_lib, bool frag, std::vector<uint64_t> &words)
{
	if (!G.lib_out) n_lib = 0;
	if (!frag) { for (int k = 0; k < BDP_GRP_N; ++k) G.out[k] = 0; for (uint32_t k = 0; k < BDP_GRP_N * n_lib; ++k) G.lib_out[k] = 0; }
	auto add = [&](uint32_t t, int k) { ++G.out[k]; if (bdp_lib_of(E[t]) < n_lib) ++G.lib_out[BDP_GRP_N * (size_t)bdp_lib_of(E[t]) + k]; };
	// the barcoded elements of the pass: a, b the key (b 0 in the fragment pass), w the word, id where the canonical word goes
	struct elem_t { uint64_t a, b, w; uint32_t id, t; };
	std::vector<elem_t> el;
	words.assign((size_t)(frag ? 2 * T : T), 0);
	for (uint64_t t = 0; t < T; ++t) {
		const uint32_t k = bdp_kind(E[t]), u = (uint32_t)t;
		if (frag) { words[2 * t] = words[2 * t + 1] = B[t]; if (k != BDP_NONE && B[t]) { el.push_back({E[t].lo, 0, B[t], u << 1, u}); if (k == BDP_PAIR) el.push_back({E[t].hi, 0, B[t], u << 1 | 1u, u}); } }
		else { words[t] = B[t]; if (k == BDP_PAIR && B[t]) el.push_back({E[t].lo, E[t].hi, B[t], u, u}); }
	}
	std::sort(el.begin(), el.end(), [](const elem_t &x, const elem_t &y) { return x.a != y.a ? x.a < y.a : x.b != y.b ? x.b < y.b : x.w != y.w ? x.w < y.w : x.id < y.id; });
	// the distinct (key, word) in that order: the members; wid: every element's member
	std::vector<uint32_t> key, mt, parent, wid(el.size()), kstart; std::vector<uint64_t> word;
	for (size_t i = 0; i < el.size(); ++i) {
		const bool same_key = i && el[i].a == el[i - 1].a && el[i].b == el[i - 1].b;
		if (!same_key) kstart.push_back((uint32_t)word.size());
		if (!(same_key && el[i].w == el[i - 1].w)) { key.push_back((uint32_t)kstart.size() - 1); word.push_back(el[i].w); mt.push_back(el[i].t); parent.push_back((uint32_t)parent.size()); }
		wid[i] = (uint32_t)word.size() - 1;
	}
	const uint32_t m = (uint32_t)word.size();
	kstart.push_back(m);
	for (uint32_t i = 0; i < m; ++i) {
		const uint32_t size = kstart[key[i] + 1] - kstart[key[i]];
		if (size > G.max_set) { if (kstart[key[i]] == i) add(mt[i], BDP_GRP_SKIPPED); continue; }
		bdp_bc_walk(i, m, key.data(), word.data(), G.edits, parent.data());
		assert(parent[i] <= i);
	}
	for (uint32_t i = 0; i < m && !frag; ++i) { add(mt[i], BDP_GRP_OBSERVED); if (parent[i] == i) add(mt[i], BDP_GRP_INFERRED); }
	for (size_t i = 0; i < el.size(); ++i) words[el[i].id] = word[bdp_uf_find(parent.data(), wid[i])];
}

void bdp_decide_host(const bdp_entry_t *E, uint64_t T, std::vector<uint32_t> &bits, uint64_t counts[5], const bdp_plan_t &P, const uint64_t *B, std::vector<uint64_t> *pair_words)
{
	const uint32_t n_lib = P.n_lib(); uint64_t *lib_counts = n_lib ? P.lib_counts : nullptr;
	const bdp_group_t *G = B ? P.grouping() : nullptr;
	// grouping by edits: the pair pass and the fragment pass each compare their own canonical words
	std::vector<uint64_t> Bp, Bf;
	if (G) { bdp_group_host(E, T, B, *G, n_lib, false, Bp); bdp_group_host(E, T, B, *G, n_lib, true, Bf); if (pair_words) *pair_words = Bp; }
	auto bc = [&](uint32_t t) { return G ? Bp[t] : B ? B[t] : 0ull; };  // (without barcodes every word is equal: the keys are those of old)
	auto bci = [&](uint32_t t, uint32_t end) { return G ? Bf[2 * (size_t)t + end] : B ? B[t] : 0ull; };
	bits.assign((size_t)((T + 31) / 32), 0u);
	for (int k = 0; k < 5; ++k) counts[k] = 0;
	auto mark = [&](uint32_t t) { bits[t >> 5] |= 1u << (t & 31); counts[BDP_FLAGGED] += bdp_n_rec(E[t]); };
	std::vector<uint32_t> pairs;
	struct item_t { uint64_t word, bc, rank; uint32_t t; };
	std::vector<item_t> items;
	for (uint64_t t = 0; t < T; ++t) {
		const uint32_t k = bdp_kind(E[t]);
		if (k == BDP_PAIR) { pairs.push_back((uint32_t)t); items.push_back({E[t].lo, bci((uint32_t)t, 0), 0, (uint32_t)t}); items.push_back({E[t].hi, bci((uint32_t)t, 1), 0, (uint32_t)t}); }
		else if (k == BDP_FRAG) items.push_back({E[t].lo, bci((uint32_t)t, 0), bdp_frag_word(E[t], (uint32_t)t), (uint32_t)t});
	}
	counts[BDP_PAIRS] = pairs.size(); counts[BDP_FRAGS] = items.size() - 2 * pairs.size();
	std::sort(pairs.begin(), pairs.end(), [&](uint32_t a, uint32_t b) {
		if (E[a].lo != E[b].lo) return E[a].lo < E[b].lo;
		if (E[a].hi != E[b].hi) return E[a].hi < E[b].hi;
		if (bc(a) != bc(b)) return bc(a) < bc(b);
		return bdp_rank_word(E[a], a) < bdp_rank_word(E[b], b);
	});
	for (size_t i = 1; i < pairs.size(); ++i)
		if (E[pairs[i]].lo == E[pairs[i - 1]].lo && E[pairs[i]].hi == E[pairs[i - 1]].hi && bc(pairs[i]) == bc(pairs[i - 1])) { mark(pairs[i]); ++counts[BDP_DUP_PAIRS]; }
	std::sort(items.begin(), items.end(), [](const item_t &a, const item_t &b) { return a.word != b.word ? a.word < b.word : a.bc != b.bc ? a.bc < b.bc : a.rank < b.rank; });
	for (size_t i = 0, first = 0; i < items.size(); ++i) {
		if (i && (items[i].word != items[i - 1].word || items[i].bc != items[i - 1].bc)) first = i;
		if (bdp_kind(E[items[i].t]) != BDP_FRAG) continue;
		if (bdp_kind(E[items[first].t]) == BDP_PAIR || i != first) { mark(items[i].t); ++counts[BDP_DUP_FRAGS]; }
	}
	if (!lib_counts) return;
	for (uint32_t k = 0; k < BDP_N_COUNTS * n_lib; ++k) lib_counts[k] = 0;
	for (uint64_t t = 0; t < T; ++t) {
		if (bdp_kind(E[t]) == BDP_NONE || bdp_lib_of(E[t]) >= n_lib) continue;
		uint64_t *c = lib_counts + BDP_N_COUNTS * (size_t)bdp_lib_of(E[t]);
		const uint32_t s = bdp_examined_slot(E[t]);
		++c[s];
		if (bits[t >> 5] >> (t & 31) & 1u) { ++c[2 + s]; c[BDP_FLAGGED] += bdp_n_rec(E[t]); }
	}
}

int bdp_optical_check(int64_t distance, uint64_t max_set, const char *fn)
{
	if (distance < 0 || distance > 0x7fffffffll) { bmh_set_error("%s: an optical distance of %lld (0 .. 2^31 - 1)", fn, (long long)distance); return BMH_EINVAL; }
	if (max_set > 0x7fffffffull) { bmh_set_error("%s: a largest set of %llu pairs (below 2^31; 0: %d)", fn, (unsigned long long)max_set, (int)BDP_OPT_MAX_SET); return BMH_EINVAL; }
	return BMH_OK;
}

void bdp_optical_host(const bdp_entry_t *E, const bdp_loc_t *L, uint64_t T, const bdp_optical_t &O, uint32_t n_lib, const uint64_t *B)
{
	auto bc = [&](uint32_t t) { return B ? B[t] : 0ull; };
	for (int k = 0; k < BDP_OPT_N; ++k) O.out[k] = 0;
	if (!O.lib_out) n_lib = 0;
	for (uint32_t k = 0; k < BDP_OPT_N * n_lib; ++k) O.lib_out[k] = 0;
	auto add = [&](uint32_t t, int k, uint64_t v) { O.out[k] += v; if (bdp_lib_of(E[t]) < n_lib) O.lib_out[BDP_OPT_N * (size_t)bdp_lib_of(E[t]) + k] += v; };
	std::vector<uint32_t> pairs;
	for (uint64_t t = 0; t < T; ++t) if (bdp_kind(E[t]) == BDP_PAIR) { pairs.push_back((uint32_t)t); if (L[t].flags & BDP_LOC_LOCATED) add((uint32_t)t, BDP_OPT_LOCATED, 1); }
	std::sort(pairs.begin(), pairs.end(), [&](uint32_t a, uint32_t b) { return E[a].lo != E[b].lo ? E[a].lo < E[b].lo : E[a].hi != E[b].hi ? E[a].hi < E[b].hi : bc(a) != bc(b) ? bc(a) < bc(b) : a < b; });
	// the located members of the sets of 2 .. max_set pairs, every one with the index of its set's first pair
	struct member_t { uint64_t w2, w1; uint32_t t; };
	std::vector<member_t> mem;
	for (size_t a = 0, b; a < pairs.size(); a = b) {
		for (b = a + 1; b < pairs.size() && E[pairs[b]].lo == E[pairs[a]].lo && E[pairs[b]].hi == E[pairs[a]].hi && bc(pairs[b]) == bc(pairs[a]);) ++b;
		if (b - a < 2) continue;
		if (b - a > O.max_set) { add(pairs[a], BDP_OPT_SKIPPED, 1); continue; }
		for (size_t i = a; i < b; ++i) if (L[pairs[i]].flags & BDP_LOC_LOCATED) mem.push_back({bdp_opt_word2((uint32_t)a, L[pairs[i]]), bdp_opt_word1(L[pairs[i]]), pairs[i]});
	}
	std::sort(mem.begin(), mem.end(), [](const member_t &a, const member_t &b) { return a.w2 != b.w2 ? a.w2 < b.w2 : a.w1 != b.w1 ? a.w1 < b.w1 : a.t < b.t; });
	const uint32_t m = (uint32_t)mem.size();
	std::vector<uint64_t> w2(m); std::vector<uint32_t> tile(m), parent(m); std::vector<int32_t> x(m), y(m);
	for (uint32_t j = 0; j < m; ++j) { const bdp_loc_t &l = L[mem[j].t]; w2[j] = mem[j].w2; tile[j] = l.tile; x[j] = l.x; y[j] = l.y; parent[j] = j; }
	for (uint32_t i = 0; i < m; ++i) {
		bdp_opt_walk(i, m, w2.data(), tile.data(), x.data(), y.data(), O.distance, parent.data());
		assert(parent[i] <= i);
	}
	for (uint32_t j = 0; j < m; ++j) { assert(parent[j] <= j); if (parent[j] != j) add(mem[j].t, BDP_OPT_DUPS, 1); }
}

void bdp_lib_tally_host(const uint8_t *recs, const uint64_t *off, uint32_t n, const uint32_t *tpl, const bdp_entry_t *E, uint64_t T, uint32_t n_lib, uint64_t *lib_counts)
{
	for (uint64_t t = 0; t < T; ++t) if (bdp_lib_of(E[t]) < n_lib) ++lib_counts[BDP_N_COUNTS * (size_t)bdp_lib_of(E[t]) + BDP_TEMPLATES];
	for (uint32_t i = 0; i < n; ++i) {
		if (tpl[i] >= T || bdp_lib_of(E[tpl[i]]) >= n_lib) continue;
		uint64_t *c = lib_counts + BDP_N_COUNTS * (size_t)bdp_lib_of(E[tpl[i]]);
		const uint32_t fl = bsr_flag(recs + off[i]);
		if (fl & 0x900u) ++c[BDP_SECSUP];
		if (fl & 4u) ++c[BDP_UNMAPPED];
	}
}

int bdp_markdup_host(uint8_t *recs, const std::vector<uint64_t> &off, uint64_t counts[BDP_N_COUNTS], const char *fn, const bdp_plan_t &P)
{
	const bdp_table_t *T = P.groups(); const bdp_optical_t *O = P.optical(); const bdp_bc_t *bc = P.barcode(); const bdp_group_t *grp = P.grouping();
	std::vector<uint64_t> Bp;
	if (P.no_barcode) *P.no_barcode = 0;
	std::vector<uint64_t> Bw;
	const uint32_t n = (uint32_t)(off.size() - 1);
	for (int k = 0; k < BDP_N_COUNTS; ++k) counts[k] = 0;
	for (uint32_t i = 0; i < n; ++i)
		if (!bdp_record_whole(recs + off[i], off[i + 1] - off[i])) {
			bmh_set_error("%s: record %u is cut: its bases and qualities do not lie inside its block_size", fn, i); return BMH_EINVAL;
		}
	std::vector<uint32_t> tpl, bits; std::vector<bdp_entry_t> E; std::vector<bdp_loc_t> locs;
	int rc = T ? bdp_refs_fit(recs, off.data(), n, fn) : BMH_OK;
	if (rc != BMH_OK) return rc;
	rc = bdp_entries_host(recs, off.data(), n, tpl, E, counts + BDP_SECSUP, fn, P, O ? &locs : nullptr, bc ? &Bw : nullptr);
	if (rc != BMH_OK) return rc;
	counts[BDP_TEMPLATES] = E.size();
	if (bc && P.no_barcode) *P.no_barcode = bdp_no_barcode(Bw.data(), Bw.size());
	bdp_decide_host(E.data(), E.size(), bits, counts, P, bc ? Bw.data() : nullptr, &Bp);
	if (O) bdp_optical_host(E.data(), locs.data(), E.size(), *O, P.n_lib(), grp ? Bp.data() : bc ? Bw.data() : nullptr);
	if (T && P.lib_counts) bdp_lib_tally_host(recs, off.data(), n, tpl.data(), E.data(), E.size(), T->n_lib, P.lib_counts);
	for (uint32_t i = 0; i < n; ++i) if (bits[tpl[i] >> 5] >> (tpl[i] & 31) & 1u) recs[off[i] + 19] |= 0x04;
	return BMH_OK;
}

#ifndef BDP_STANDALONE
extern "C" void bmh_markdup_opt_default(bmh_markdup_opt_t *o)
{
	if (!o) return;
	memset(o, 0, sizeof *o);
	o->optical_distance = -1; o->barcode_edits = -1;
}

int bdp_plan_make(bdp_plan_t &P, const bmh_markdup_opt_t *opt, bmh_markdup_counts_t *res, const char *fn)
{
	P = bdp_plan_t();
	if (!res) { bmh_set_error("%s: null argument", fn); return BMH_EINVAL; }
	for (uint64_t &c : res->counts) c = 0;
	for (int k = 0; k < 3; ++k) res->optical[k] = res->grouped[k] = 0;
	res->no_barcode = 0;
	bmh_markdup_opt_t def;
	if (!opt) { bmh_markdup_opt_default(&def); opt = &def; }
	int rc = bdp_barcode_check(opt->barcode_mode, opt->barcode_tag, fn, &P.bc);
	if (rc != BMH_OK) return rc;
	if ((rc = bdp_group_check(opt->barcode_edits, opt->barcode_max_set, fn, &P.bc)) != BMH_OK) return rc;
	const bool optical = opt->optical_distance != -1;
	if (optical && (rc = bdp_optical_check(opt->optical_distance, opt->optical_max_set, fn)) != BMH_OK) return rc;
	const bool groups = opt->rg_ids || opt->rg_lib || opt->n_groups;
	if (groups && (rc = bdp_table_make(P.table, opt->rg_ids, opt->rg_lib, opt->n_groups, fn)) != BMH_OK) return rc;
	if (optical && groups && opt->n_groups > (int)BDP_OPT_MAX_GROUPS) { bmh_set_error("%s: %d read groups: a location holds a group's row in 16 bits", fn, opt->n_groups); return BMH_EINVAL; }
	if (optical) P.opt = {opt->optical_distance, opt->optical_max_set ? (uint32_t)opt->optical_max_set : (uint32_t)BDP_OPT_MAX_SET, res->optical, groups ? res->lib_optical : nullptr};
	if (P.bc.pack) P.grp = {(uint32_t)opt->barcode_edits, opt->barcode_max_set ? (uint32_t)opt->barcode_max_set : (uint32_t)BDP_BC_MAX_SET, res->grouped, groups ? res->lib_grouped : nullptr};
	P.lib_counts = groups ? res->lib_counts : nullptr; P.no_barcode = &res->no_barcode;
	return BMH_OK;
}

// probe: stop at the templates' locations or barcode words (bdp_probe_t)
static int markdup_host(const char *fn, const uint8_t *recs, uint64_t n_bytes, const bdp_plan_t &P, bdp_probe_t probe, uint8_t **out, uint64_t counts[BDP_N_COUNTS])
{
	if (!out || (n_bytes && !recs)) { bmh_set_error("%s: null argument", fn); return BMH_EINVAL; }
	*out = nullptr;
	std::vector<uint64_t> off;
	int rc = bsr_walk(recs, n_bytes, -1, off, fn);
	if (rc != BMH_OK) return rc;
	std::vector<uint32_t> tpl; std::vector<bdp_entry_t> E; std::vector<bdp_loc_t> L; std::vector<uint64_t> Bw; uint64_t info[2] = {0, 0};
	const uint8_t *src = recs; uint64_t nb = n_bytes;
	if (probe != BDP_MARK) {
		const uint32_t n = (uint32_t)(off.size() - 1);
		for (uint32_t i = 0; i < n; ++i)
			if (!bdp_record_whole(recs + off[i], off[i + 1] - off[i])) { bmh_set_error("%s: record %u is cut: its bases and qualities do not lie inside its block_size", fn, i); return BMH_EINVAL; }
		if ((rc = bdp_entries_host(recs, off.data(), n, tpl, E, info, fn, P, probe == BDP_PROBE_LOCS ? &L : nullptr, probe == BDP_PROBE_BCS ? &Bw : nullptr)) != BMH_OK) return rc;
		counts[BDP_TEMPLATES] = E.size();
		src = probe == BDP_PROBE_LOCS ? (const uint8_t *)L.data() : (const uint8_t *)Bw.data(); nb = (probe == BDP_PROBE_LOCS ? sizeof(bdp_loc_t) : 8) * E.size();
	}
	uint8_t *o = (uint8_t *)malloc(nb + 8);
	if (!o) { bmh_set_error("%s: out of memory", fn); return BMH_ENOMEM; }
	if (nb) memcpy(o, src, nb);
	if (probe == BDP_MARK && (rc = bdp_markdup_host(o, off, counts, fn, P)) != BMH_OK) { free(o); return rc; }
	*out = o;
	return BMH_OK;
}

extern "C" int bmh_bam_markdup_host(const uint8_t *recs, uint64_t n_bytes, const bmh_markdup_opt_t *opt, uint8_t **out, bmh_markdup_counts_t *res)
{
	const char *fn = "bmh_bam_markdup_host";
	bdp_plan_t P;
	if (out) *out = nullptr;
	const int rc = bdp_plan_make(P, opt, res, fn);
	return rc != BMH_OK ? rc : markdup_host(fn, recs, n_bytes, P, BDP_MARK, out, res->counts);
}

int bdp_probe_plan(bdp_plan_t &P, const char *const *rg_ids, const int32_t *rg_lib, int n_groups, int barcode_mode, const char tag[2], int packed, const char *fn)
{
	bmh_markdup_opt_t o; bmh_markdup_counts_t res = {};
	bmh_markdup_opt_default(&o);
	o.rg_ids = rg_ids; o.rg_lib = rg_lib; o.n_groups = n_groups; o.barcode_mode = barcode_mode;
	if (tag) { o.barcode_tag[0] = tag[0]; o.barcode_tag[1] = tag[0] ? tag[1] : 0; }
	if (barcode_mode == BDP_BC_OFF) o.optical_distance = 0; else if (packed) o.barcode_edits = 0;
	const int rc = bdp_plan_make(P, &o, &res, fn);
	P.opt.out = P.grp.out = P.no_barcode = nullptr;               // (res ends here: a probe counts nothing)
	return rc;
}

extern "C" int bmh_bam_dup_locations_host(const uint8_t *recs, uint64_t n_bytes, const char *const *rg_ids, const int32_t *rg_lib, int n_groups, uint8_t **locs, uint64_t *n_templates)
{
	const char *fn = "bmh_bam_dup_locations_host";
	if (locs) *locs = nullptr;
	if (!n_templates) { bmh_set_error("%s: null argument", fn); return BMH_EINVAL; }
	*n_templates = 0;
	bdp_plan_t P; uint64_t counts[BDP_N_COUNTS];
	int rc = bdp_probe_plan(P, rg_ids, rg_lib, n_groups, BDP_BC_OFF, nullptr, 0, fn);
	if (rc != BMH_OK || (rc = markdup_host(fn, recs, n_bytes, P, BDP_PROBE_LOCS, locs, counts)) != BMH_OK) return rc;
	*n_templates = counts[BDP_TEMPLATES];
	return BMH_OK;
}

extern "C" int bmh_bam_dup_barcodes_host(const uint8_t *recs, uint64_t n_bytes, int barcode_mode, const char tag[2], int packed, uint64_t **words, uint64_t *n_templates)
{
	const char *fn = "bmh_bam_dup_barcodes_host";
	if (words) *words = nullptr;
	if (!n_templates) { bmh_set_error("%s: null argument", fn); return BMH_EINVAL; }
	*n_templates = 0;
	if (barcode_mode == BDP_BC_OFF) { bmh_set_error("%s: no barcode source (1: a tag, 2: the read name)", fn); return BMH_EINVAL; }
	bdp_plan_t P; uint64_t counts[BDP_N_COUNTS];
	int rc = bdp_probe_plan(P, nullptr, nullptr, 0, barcode_mode, tag, packed, fn);
	if (rc != BMH_OK || (rc = markdup_host(fn, recs, n_bytes, P, BDP_PROBE_BCS, (uint8_t **)words, counts)) != BMH_OK) return rc;
	*n_templates = counts[BDP_TEMPLATES];
	return BMH_OK;
}

extern "C" uint64_t bmh_barcode_word(const uint8_t *value, uint64_t n) { return value || !n ? bdp_barcode_word(value, n) : 0; }

extern "C" int bmh_barcode_pack(const uint8_t *value, uint64_t n, uint64_t *word)
{
	if (!word || (n && !value)) { bmh_set_error("bmh_barcode_pack: null argument"); return BMH_EINVAL; }
	return bdp_barcode_pack(value, n, word) ? 1 : 0;
}

extern "C" int bmh_bam_name_location(const char *name, uint32_t len, uint32_t out[3])
{
	if (!out || (len && !name)) { bmh_set_error("bmh_bam_name_location: null argument"); return BMH_EINVAL; }
	out[0] = out[1] = out[2] = 0;
	return bdp_name_location((const uint8_t *)name, len, out) ? 1 : 0;
}

extern "C" int bmh_library_size(uint64_t n_pairs, uint64_t n_unique, int64_t *size)
{
	bool has = false;
	const int64_t v = bdp_library_size(n_pairs, n_unique, &has);
	if (size) *size = v;
	return has ? 1 : 0;
}
#endif
