// Duplicate marking on the host (csrc/bam_dup_core.h's rules): the templates' entries of a record stream, the decision (std::sort where the device runs radix
// passes), the flags, and bmh_bam_markdup_host.  Byte for byte what csrc/bam_dup_kernels.hip gives.
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <numeric>
#include "bam_dup.h"
#ifndef BDP_STANDALONE
#include "bam_sort.h"
#endif

int bdp_batch_refused(uint32_t n, uint32_t bad, const char *fn)
{
	if (bad > n) bmh_set_error("%s: duplicate marking: the stream's first record begins no template (a secondary or supplementary line, or read 2 of a pair)", fn);
	else bmh_set_error("%s: duplicate marking: the template that begins at record %u is paired and lacks one of its two primary lines (0x40, 0x80)", fn, bad - 1);
	return BMH_EINVAL;
}

int bdp_entries_host(const uint8_t *recs, const uint64_t *off, uint32_t n, std::vector<uint32_t> &tpl, std::vector<bdp_entry_t> &entries, uint64_t info[2], const char *fn)
{
	tpl.resize(n); entries.clear();
	if (n && !bdp_head(bsr_flag(recs + off[0]))) return bdp_batch_refused(n, n + 1, fn);
	std::vector<uint32_t> start;
	for (uint32_t i = 0; i < n; ++i) {
		const uint32_t fl = bsr_flag(recs + off[i]);
		if (bdp_head(fl)) start.push_back(i);
		tpl[i] = (uint32_t)start.size() - 1;
		if (fl & 0x900u) ++info[0];
		if (fl & 4u) ++info[1];
	}
	if (start.size() >= 1ull << 31) { bmh_set_error("%s: duplicate marking: 2^31 templates", fn); return BMH_EINVAL; }
	entries.resize(start.size());
	for (size_t t = 0; t < start.size(); ++t)
		if (!bdp_entry(recs, off, start[t], t + 1 < start.size() ? start[t + 1] : n, &entries[t])) return bdp_batch_refused(n, start[t] + 1, fn);
	return BMH_OK;
}

void bdp_decide_host(const bdp_entry_t *E, uint64_t T, std::vector<uint32_t> &bits, uint64_t counts[5])
{
	bits.assign((size_t)((T + 31) / 32), 0u);
	for (int k = 0; k < 5; ++k) counts[k] = 0;
	auto mark = [&](uint32_t t) { bits[t >> 5] |= 1u << (t & 31); counts[BDP_FLAGGED] += bdp_n_rec(E[t]); };
	std::vector<uint32_t> pairs;
	struct item_t { uint64_t word, rank; uint32_t t; };
	std::vector<item_t> items;
	for (uint64_t t = 0; t < T; ++t) {
		const uint32_t k = bdp_kind(E[t]);
		if (k == BDP_PAIR) { pairs.push_back((uint32_t)t); items.push_back({E[t].lo, 0, (uint32_t)t}); items.push_back({E[t].hi, 0, (uint32_t)t}); }
		else if (k == BDP_FRAG) items.push_back({E[t].lo, bdp_frag_word(E[t], (uint32_t)t), (uint32_t)t});
	}
	counts[BDP_PAIRS] = pairs.size(); counts[BDP_FRAGS] = items.size() - 2 * pairs.size();
	std::sort(pairs.begin(), pairs.end(), [&](uint32_t a, uint32_t b) {
		if (E[a].lo != E[b].lo) return E[a].lo < E[b].lo;
		if (E[a].hi != E[b].hi) return E[a].hi < E[b].hi;
		return bdp_rank_word(E[a], a) < bdp_rank_word(E[b], b);
	});
	for (size_t i = 1; i < pairs.size(); ++i)
		if (E[pairs[i]].lo == E[pairs[i - 1]].lo && E[pairs[i]].hi == E[pairs[i - 1]].hi) { mark(pairs[i]); ++counts[BDP_DUP_PAIRS]; }
	std::sort(items.begin(), items.end(), [](const item_t &a, const item_t &b) { return a.word != b.word ? a.word < b.word : a.rank < b.rank; });
	for (size_t i = 0, first = 0; i < items.size(); ++i) {
		if (i && items[i].word != items[i - 1].word) first = i;
		if (bdp_kind(E[items[i].t]) != BDP_FRAG) continue;
		if (bdp_kind(E[items[first].t]) == BDP_PAIR || i != first) { mark(items[i].t); ++counts[BDP_DUP_FRAGS]; }
	}
}

int bdp_markdup_host(uint8_t *recs, const std::vector<uint64_t> &off, uint64_t counts[BDP_N_COUNTS], const char *fn)
{
	const uint32_t n = (uint32_t)(off.size() - 1);
	for (int k = 0; k < BDP_N_COUNTS; ++k) counts[k] = 0;
	for (uint32_t i = 0; i < n; ++i)
		if (!bdp_record_whole(recs + off[i], off[i + 1] - off[i])) {
			bmh_set_error("%s: record %u is cut: its bases and qualities do not lie inside its block_size", fn, i); return BMH_EINVAL;
		}
	std::vector<uint32_t> tpl, bits; std::vector<bdp_entry_t> E;
	const int rc = bdp_entries_host(recs, off.data(), n, tpl, E, counts + BDP_SECSUP, fn);
	if (rc != BMH_OK) return rc;
	counts[BDP_TEMPLATES] = E.size();
	bdp_decide_host(E.data(), E.size(), bits, counts);
	for (uint32_t i = 0; i < n; ++i) if (bits[tpl[i] >> 5] >> (tpl[i] & 31) & 1u) recs[off[i] + 19] |= 0x04;
	return BMH_OK;
}

#ifndef BDP_STANDALONE
extern "C" int bmh_bam_markdup_host(const uint8_t *recs, uint64_t n_bytes, uint8_t **out, uint64_t counts[8])
{
	const char *fn = "bmh_bam_markdup_host";
	if (!out || !counts || (n_bytes && !recs)) { bmh_set_error("%s: null argument", fn); return BMH_EINVAL; }
	*out = nullptr;
	std::vector<uint64_t> off;
	int rc = bsr_walk(recs, n_bytes, -1, off, fn);
	if (rc != BMH_OK) return rc;
	uint8_t *o = (uint8_t *)malloc(n_bytes + 1);
	if (!o) { bmh_set_error("%s: out of memory", fn); return BMH_ENOMEM; }
	if (n_bytes) memcpy(o, recs, n_bytes);
	if ((rc = bdp_markdup_host(o, off, counts, fn)) != BMH_OK) { free(o); return rc; }
	*out = o;
	return BMH_OK;
}
#endif
