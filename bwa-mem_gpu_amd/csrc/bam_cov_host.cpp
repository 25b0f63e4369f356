// Coverage depth on the host (csrc/bam_cov_core.h's rules): the plan, the host form of the sweep -- the same tiles, frontier and carry as
// csrc/bam_cov_kernels.hip, in plain C++ -- and bmh_bam_coverage_host.
#include <stdlib.h>
#include <string.h>
#include <stddef.h>
#include <algorithm>
#include <new>
#include "bam_cov.h"

int bcv_plan_make(bcv_plan_t &P, int32_t min_mapq, int32_t deletions, uint32_t bin, uint32_t tile, int n_contigs, const int32_t *contig_len, const char *fn)
{
	if (min_mapq < 0 || min_mapq > 255) { bmh_set_error("%s: min_mapq %d (0 .. 255)", fn, min_mapq); return BMH_EINVAL; }
	if (tile > (uint32_t)BCV_TILE_MAX) { bmh_set_error("%s: a tile of %u positions (1 .. %d; 0: %d)", fn, tile, (int)BCV_TILE_MAX, (int)BCV_TILE_DEFAULT); return BMH_EINVAL; }
	if (n_contigs < 0 || (n_contigs && !contig_len)) { bmh_set_error("%s: null argument", fn); return BMH_EINVAL; }
	P.min_mapq = min_mapq; P.deletions = deletions != 0; P.bin = bin; P.tile = tile ? tile : (uint32_t)BCV_TILE_DEFAULT; P.n_contigs = n_contigs;
	P.len.clear(); P.coff.assign(1, 0); P.bin_off.assign(1, 0);
	for (int c = 0; c < n_contigs; ++c) {
		if (contig_len[c] < 0) { bmh_set_error("%s: contig %d has %lld bases: BAM holds contigs of at most 2^31 - 1", fn, c, (long long)(uint32_t)contig_len[c]); return BMH_EINVAL; }
		P.len.push_back(contig_len[c]); P.coff.push_back(P.coff.back() + (uint64_t)contig_len[c]);
		P.bin_off.push_back(P.bin_off.back() + (bin ? ((uint64_t)contig_len[c] + bin - 1) / bin : 0));
	}
	if (P.n_bins() >= BCV_MAX_BINS) { bmh_set_error("%s: %llu bins of %u bases (fewer than 2^28): choose a larger bin", fn, (unsigned long long)P.n_bins(), bin); return BMH_EINVAL; }
	return BMH_OK;
}

void bcv_result_t::init(const bcv_plan_t &P)
{
	const size_t n = (size_t)P.n_contigs;
	n_reads.assign(n, 0); cov_bases.assign(n, 0); sum_depth.assign(n, 0); max_depth.assign(n, 0); sum_mapq.assign(n, 0);
	hist.assign(BCV_HIST, 0); bin_sum.assign((size_t)P.n_bins(), 0);
}

void bcv_result_t::close(const bcv_plan_t &P)
{
	uint64_t covered = 0;
	for (int d = 1; d < BCV_HIST; ++d) covered += hist[(size_t)d];
	hist[0] = P.genome() - covered;
}

int bcv_refused(uint64_t rec, int st, const char *fn)
{
	if (st < 0) bmh_set_error("%s: record %llu lies before record %llu: coverage takes records in coordinate order", fn, (unsigned long long)rec, (unsigned long long)rec - 1);
	else if (st == BCV_E_POS) bmh_set_error("%s: record %llu begins outside its contig (pos is negative or not below the contig's length)", fn, (unsigned long long)rec);
	else bmh_set_error("%s: record %llu holds the long-CIGAR placeholder (its operations are in its CG tag): coverage reads the record's own operations", fn, (unsigned long long)rec);
	return BMH_EINVAL;
}

void bcv_host_t::begin(const bcv_plan_t &plan)
{
	P = plan; R.init(P);
	pending.clear(); carry = 0; done_to = 0; n_seen = 0; last_key = 0;
	diff.assign((size_t)P.tile, 0);
}

int bcv_host_t::window(const uint8_t *recs, const uint64_t *soff, uint32_t n, const char *fn)
{
	if (!n) return BMH_OK;
	for (uint32_t j = 0; j < n; ++j, ++n_seen) {
		const uint8_t *rec = recs + soff[j];
		const uint64_t key = bsr_key(rec) >> 1;
		if (n_seen && key < last_key) return bcv_refused(n_seen, -1, fn);
		last_key = key;
		if (!bcv_counted(rec, P.n_contigs, P.min_mapq)) continue;
		const int32_t r = bsr_ref(rec);
		const int st = bcv_check(rec, soff[j + 1] - soff[j], P.len[(size_t)r]);
		if (st != BCV_OK) return bcv_refused(n_seen, st, fn);
		++R.n_reads[(size_t)r]; R.sum_mapq[(size_t)r] += bcv_mapq(rec);
		const uint64_t o = P.coff[(size_t)r];
		bcv_runs(rec, P.len[(size_t)r], P.deletions, [&](int64_t b, int64_t e) { pending.push_back(bcv_key(o + (uint64_t)b, true)); pending.push_back(bcv_key(o + (uint64_t)e, false)); });
	}
	const uint64_t f = bcv_frontier(recs + soff[n - 1], P.coff.data(), P.len.data(), P.n_contigs);
	sweep(f / P.tile * P.tile);
	return BMH_OK;
}

void bcv_host_t::add(uint64_t a, uint64_t b, uint64_t d, int &c)
{
	if (b > P.genome()) b = P.genome();                              // (no event lies behind the genome's end: the clamp)
	while (a < b) {
		if (c < 0 || a < P.coff[(size_t)c] || a >= P.coff[(size_t)c + 1]) c = bcv_contig_of(P.coff.data(), P.n_contigs, a);
		const uint64_t e = std::min(b, P.coff[(size_t)c + 1]), n = e - a;
		R.cov_bases[(size_t)c] += n; R.sum_depth[(size_t)c] += d * n;
		if (d > R.max_depth[(size_t)c]) R.max_depth[(size_t)c] = d;
		R.hist[(size_t)std::min<uint64_t>(d, BCV_HIST - 1)] += n;
		if (P.bin) {
			const uint64_t o = P.coff[(size_t)c];
			for (uint64_t k = (a - o) / P.bin; k * P.bin < e - o; ++k) {
				const uint64_t lo = std::max(a - o, k * P.bin), hi = std::min(e - o, (k + 1) * P.bin);
				R.bin_sum[(size_t)(P.bin_off[(size_t)c] + k)] += d * (hi - lo);
			}
		}
		a = e;
	}
}

// every tile that begins before ft is final: its events are added, and the stretches between such tiles at the depth they carry
void bcv_host_t::sweep(uint64_t ft)
{
	std::sort(pending.begin(), pending.end());
	const size_t n_now = ft > ~0ull >> 1 ? pending.size() : (size_t)(std::lower_bound(pending.begin(), pending.end(), ft << 1) - pending.begin());
	const uint64_t T = P.tile;
	int c = -1;
	for (size_t i = 0; i < n_now;) {
		const uint64_t t0 = (pending[i] >> 1) / T * T;
		if (carry && done_to < t0) add(done_to, t0, carry, c);
		for (; i < n_now && (pending[i] >> 1) < t0 + T; ++i) diff[(size_t)((pending[i] >> 1) - t0)] += (pending[i] & 1) ? 1 : -1;
		uint64_t d = carry, a = t0;
		for (uint64_t p = 0; p < T; ++p) {
			if (!diff[(size_t)p]) continue;
			if (d && a < t0 + p) add(a, t0 + p, d, c);
			d = (uint64_t)((int64_t)d + diff[(size_t)p]); diff[(size_t)p] = 0; a = t0 + p;
		}
		if (d) add(a, t0 + T, d, c);
		carry = d; done_to = t0 + T;
	}
	pending.erase(pending.begin(), pending.begin() + (ptrdiff_t)n_now);
}

int bcv_host_t::finish(const char *fn)
{
	sweep(~0ull);
	if (carry || !pending.empty()) { bmh_set_error("%s: internal error: a depth of %llu is left behind the last event", fn, (unsigned long long)carry); return BMH_EINVAL; }
	R.close(P);
	return BMH_OK;
}

#ifndef BCV_STANDALONE
#include "bam_sort.h"

extern "C" void bmh_coverage_opt_default(bmh_coverage_opt_t *o) { if (o) { o->min_mapq = 0; o->deletions = 0; o->bin = 0; o->tile = 0; } }

int bcv_export(const bcv_plan_t &P, const bcv_result_t &R, bmh_coverage_t *out, const char *fn)
{
	memset(out, 0, sizeof *out);
	auto dup = [](const std::vector<uint64_t> &v) { uint64_t *p = (uint64_t *)malloc(8 * v.size() + 8); if (p && !v.empty()) memcpy(p, v.data(), 8 * v.size()); return p; };
	out->n_contigs = P.n_contigs; out->n_bins = P.n_bins();
	out->n_reads = dup(R.n_reads); out->cov_bases = dup(R.cov_bases); out->sum_depth = dup(R.sum_depth); out->max_depth = dup(R.max_depth); out->sum_mapq = dup(R.sum_mapq);
	out->hist = dup(R.hist); out->bin_sum = dup(R.bin_sum);
	if (!out->n_reads || !out->cov_bases || !out->sum_depth || !out->max_depth || !out->sum_mapq || !out->hist || !out->bin_sum) {
		free(out->n_reads); free(out->cov_bases); free(out->sum_depth); free(out->max_depth); free(out->sum_mapq); free(out->hist); free(out->bin_sum);
		memset(out, 0, sizeof *out);
		bmh_set_error("%s: out of memory", fn); return BMH_ENOMEM;
	}
	return BMH_OK;
}

// the records of a stream in windows of `window` records (0: as many as hold about 64 MiB), as the sorted file's merge hands them on
extern "C" int bmh_bam_coverage_host(const uint8_t *recs, uint64_t n_bytes, int n_contigs, const int32_t *contig_len, const bmh_coverage_opt_t *opt, bmh_coverage_t *out)
{
	const char *fn = "bmh_bam_coverage_host";
	if (!out || (n_bytes && !recs)) { bmh_set_error("%s: null argument", fn); return BMH_EINVAL; }
	memset(out, 0, sizeof *out);
	bmh_coverage_opt_t o; bmh_coverage_opt_default(&o);
	if (opt) o = *opt;
	bcv_plan_t P;
	int rc = bcv_plan_make(P, o.min_mapq, o.deletions, o.bin, o.tile, n_contigs, contig_len, fn);
	if (rc != BMH_OK) return rc;
	std::vector<uint64_t> off;
	if ((rc = bsr_walk(recs, n_bytes, -1, off, fn)) != BMH_OK) return rc;
	try {
		bcv_host_t H; H.begin(P);
		const size_t n = off.size() - 1;
		const uint64_t W = std::max<uint64_t>(1, (64ull << 20) / std::max<uint64_t>(1, n ? n_bytes / n : 1));
		for (size_t a = 0; a < n; a += W) {
			const size_t b = (size_t)std::min<uint64_t>(n, a + W);
			if ((rc = H.window(recs, off.data() + a, (uint32_t)(b - a), fn)) != BMH_OK) return rc;
		}
		if ((rc = H.finish(fn)) != BMH_OK) return rc;
		return bcv_export(P, H.R, out, fn);
	} catch (const std::bad_alloc &) { bmh_set_error("%s: out of memory", fn); return BMH_ENOMEM; }
}
#endif
