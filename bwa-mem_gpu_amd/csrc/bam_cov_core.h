// Coverage depth of coordinate-sorted BAM records: the per-record rules of csrc/bam_cov_kernels.hip (one lane per record) and, compiled as plain
// C++, of csrc/bam_cov_host.cpp and tests/bam_cov_core_host.cpp (under the sanitizers).
//
//   counted   refID in 0 .. n_contigs - 1, none of the flags 0x4 0x100 0x200 0x400, mapq >= min_mapq (`samtools depth`'s default filters; 0x800 counts)
//   covered   the reference positions under M, = and X, and under D with `deletions` (`samtools depth -J`); N never; S, I, H and P take no reference.  A run that
//             passes the contig's end is clamped to its length; a counted record without operations is a read that covers nothing
//   runs      neighbouring covering operations are one run (10M3I10M covers 20 positions in one run): a run is two events, +1 at its first position and -1 behind
//             its last, in genome coordinates: the contig's offset (the sum of the lengths before it, 64 bits) + the position
//   key       an event as a sortable word: coordinate << 1 | start.  The clamp keeps every event of a contig inside [offset, offset + length], so the depth
//             that the events before a contig's first position add up to is 0: nothing is carried from one contig into the next
//   tiles     the genome is cut every T positions (the option `tile`); a tile that holds an event is swept through a difference array of T words, a stretch
//             of tiles without events has one depth -- the carry -- and is added in closed form: work and memory follow the events, not the genome
//   refused   a counted record whose pos is negative or not below its contig's length; a counted record whose operations are the long-CIGAR placeholder
//             (l_seq S, then N, with a CG:B,I tag: its real operations are in the tag, which nothing here reads)
#pragma once
#include <stdint.h>
#include "bam_sort_core.h"

#define BCV_FN BSR_FN

enum { BCV_HIST = 1001, BCV_TILE_DEFAULT = 4096, BCV_TILE_MAX = 4096, BCV_SKIP_FLAGS = 0x4 | 0x100 | 0x200 | 0x400 };
enum { BCV_OK = 0, BCV_E_POS = 1, BCV_E_PLACEHOLDER = 2 };
#define BCV_MAX_BINS (1ull << 28)

BCV_FN uint32_t bcv_mapq(const uint8_t *rec) { return rec[13]; }
BCV_FN uint32_t bcv_n_ops(const uint8_t *rec) { return bsr_u16(rec + 16); }

BCV_FN bool bcv_counted(const uint8_t *rec, int n_contigs, int min_mapq)
{
	const int32_t r = bsr_ref(rec);
	return r >= 0 && r < n_contigs && !(bsr_flag(rec) & (uint32_t)BCV_SKIP_FLAGS) && (int)bcv_mapq(rec) >= min_mapq;
}

// does the record of `size` bytes carry a CG tag of type B,I (the tags are walked by their types; a tag that cannot be walked ends the walk: no)
BCV_FN bool bcv_has_cg(const uint8_t *rec, uint64_t size)
{
	const uint64_t l_seq = bsr_u32(rec + 20);
	uint64_t p = (uint64_t)BSR_FIXED + rec[12] + 4ull * bcv_n_ops(rec) + (l_seq + 1) / 2 + l_seq;
	while (p + 3 <= size) {
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
			if (p + 5 > size) return false;
			const uint8_t s = rec[p];
			const uint64_t w = s == 'c' || s == 'C' ? 1 : s == 's' || s == 'S' ? 2 : s == 'i' || s == 'I' || s == 'f' ? 4 : 0;
			if (!w) return false;
			if (a == 'C' && b == 'G' && s == 'I') return true;
			len = 5 + w * (uint64_t)bsr_u32(rec + p + 1);
		} else return false;
		if (len > size - p) return false;
		p += len;
	}
	return false;
}

// a counted record of `size` bytes on a contig of clen bases: BCV_OK, or why it is refused
BCV_FN int bcv_check(const uint8_t *rec, uint64_t size, int64_t clen)
{
	const int64_t pos = bsr_pos(rec);
	if (pos < 0 || pos >= clen) return BCV_E_POS;
	if (bcv_n_ops(rec) == 2) {
		const uint8_t *c = rec + BSR_FIXED + rec[12];
		const uint32_t a = bsr_u32(c), b = bsr_u32(c + 4);
		if ((a & 15u) == 4u && (a >> 4) == bsr_u32(rec + 20) && (b & 15u) == 3u && bcv_has_cg(rec, size)) return BCV_E_PLACEHOLDER;
	}
	return BCV_OK;
}

// the covered runs [b, e) of a counted, checked record on its contig, clamped to clen, in order: f(b, e) for every run that holds a position; their number
template <class F> BCV_FN uint32_t bcv_runs(const uint8_t *rec, int64_t clen, bool deletions, F f)
{
	const uint8_t *c = rec + BSR_FIXED + rec[12];
	const uint32_t n = bcv_n_ops(rec);
	int64_t x = bsr_pos(rec), rb = -1;
	uint32_t runs = 0;
	for (uint32_t i = 0; i <= n; ++i) {
		uint32_t op = 3, len = 0;                              // behind the last operation: as N of no length, which ends a run
		if (i < n) { const uint32_t v = bsr_u32(c + 4 * i); op = v & 15u; len = v >> 4; }
		const bool covers = op == 0 || op == 7 || op == 8 || (op == 2 && deletions);
		if (covers) { if (rb < 0 && len) rb = x; x += len; continue; }
		if (op != 2 && op != 3) continue;                      // S I H P (and what the specification does not name): no reference, the run goes on
		if (rb >= 0 && rb < clen) { f(rb, x < clen ? x : clen); ++runs; }
		rb = -1; x += len;
	}
	return runs;
}

// the contig of genome coordinate g < coff[n]: coff [n + 1] the contigs' offsets (contigs without bases hold no coordinate)
BCV_FN int bcv_contig_of(const uint64_t *coff, int n, uint64_t g)
{
	int lo = 0, hi = n;                                        // the last c with coff[c] <= g
	while (hi - lo > 1) { const int m = lo + (hi - lo) / 2; if (coff[m] <= g) lo = m; else hi = m; }
	return lo;
}

BCV_FN uint64_t bcv_key(uint64_t g, bool start) { return g << 1 | (start ? 1u : 0u); }

// the frontier a window's last record sets: every later record begins at or behind it (a record without a contig: the genome's end)
BCV_FN uint64_t bcv_frontier(const uint8_t *rec, const uint64_t *coff, const int64_t *clen, int n_contigs)
{
	const int32_t r = bsr_ref(rec);
	if (r < 0 || r >= n_contigs) return coff[n_contigs];
	int64_t p = bsr_pos(rec);
	if (p < 0) p = 0;
	if (p > clen[r]) p = clen[r];
	return coff[r] + (uint64_t)p;
}
