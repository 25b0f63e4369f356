// Flag counts, contig counts, an alignment summary and insert sizes of BAM records: the per-record rules of csrc/bam_stats_kernels.hip (one lane
// per record) and, compiled as plain C++, of csrc/bam_stats_host.cpp and tests/bam_stats_core_host.cpp (under the sanitizers).  Every result is a uint64 sum, a
// minimum or a maximum over records, so no result depends on the order of the records, on windows or on the form.
//
//   A flags     `samtools flagstat`'s walk, in two columns (column 1: 0x200 set).  total; secondary (0x100), else supplementary (0x800), else primary -- and of a
//               primary record: paired (0x1), of a paired one proper (0x2 without 0x4), read1 (0x40), read2 (0x80), singleton (0x8 without 0x4), both mapped
//               (neither 0x4 nor 0x8), of those the mate on another contig (next_refID != refID) and that at mapq >= 5; primary mapped (no 0x4), primary
//               duplicate (0x400); of every record mapped (no 0x4) and duplicate (0x400)
//   B contigs   `samtools idxstats`: per contig the records with refID = c without 0x4 (mapped) and with it (the placed unmapped mates); refID -1: unplaced.  A
//               refID outside -1 .. n_contigs - 1 is refused
//   C summary   over primary records (neither 0x100 nor 0x800): reads, bases (l_seq); of the mapped ones (no 0x4) reads, bases, those at mapq 0, mapq [256], the
//               longest l_seq (over all primary records), from the operations bases aligned (M = X I), soft-clipped (S), insertions and deletions as events and
//               bases (H N P and the codes from 9 up add nothing), from the tags the records with NM and its sum.  The tags are walked by their types to the
//               record's end; the first NM counts, of any of the types c C s S i I
//   D inserts   Picard CollectInsertSizeMetrics' rule, once per pair: 0x1 and 0x80, none of 0x4 0x8 0x100 0x800 0x400, refID == next_refID, tlen != 0.  The size
//               is |tlen| in 64 bits; the orientation TANDEM when 0x10 and 0x20 are equal, else of a forward record FR if tlen > 0 and RF if not, of a reverse
//               record FR if next_pos + 1 < pos + reflen (M = X D N; may be 0) and RF if not.  hist [cap + 1] per orientation: sizes from cap up share bin cap
//   refused     of mapped primary records only (no other record's operations or tags are read): tags that cannot be walked to the record's end, an NM of another
//               type or below 0, the long-CIGAR placeholder (l_seq S, then N, with a CG:B,I tag: the rule of bcv_check in csrc/bam_cov_core.h)
#pragma once
#include <stdint.h>
#include "bam_sort_core.h"

#define BST_FN BSR_FN

enum { BST_TOTAL = 0, BST_PRIMARY, BST_SECONDARY, BST_SUPPLEMENTARY, BST_DUP, BST_PRIMARY_DUP, BST_MAPPED, BST_PRIMARY_MAPPED, BST_PAIRED, BST_READ1, BST_READ2, BST_PROPER,
       BST_BOTH_MAPPED, BST_SINGLETONS, BST_DIFF_CHR, BST_DIFF_CHR_Q5, BST_N_FLAG = 16 };
enum { BST_READS = 0, BST_BASES, BST_READS_MAPPED, BST_BASES_MAPPED, BST_READS_MQ0, BST_MAX_LEN, BST_BASES_ALIGNED, BST_BASES_CLIPPED, BST_INS_EVENTS, BST_INS_BASES, BST_DEL_EVENTS,
       BST_DEL_BASES, BST_READS_NM, BST_EDIT_DISTANCE, BST_N_SUM = 14 };
enum { BST_FR = 0, BST_RF = 1, BST_TANDEM = 2, BST_N_ORI = 3, BST_CAP_MIN = 2, BST_CAP_MAX = 65536 };
enum { BST_OK = 0, BST_E_REF = 1, BST_E_TAGS = 2, BST_E_NM = 3, BST_E_PLACEHOLDER = 4, BST_E_CUT = 5 };
// the accumulator's fixed words: flag [2][16], the summary, mapq [256], the smallest and the largest size per orientation, the records without a contig
enum { BST_W_FLAG = 0, BST_W_SUM = 2 * BST_N_FLAG, BST_W_MAPQ = BST_W_SUM + BST_N_SUM, BST_W_MIN = BST_W_MAPQ + 256, BST_W_MAX = BST_W_MIN + BST_N_ORI, BST_W_UNPLACED = BST_W_MAX + BST_N_ORI,
       BST_W_FIXED = BST_W_UNPLACED + 1, BST_W_LDS = BST_W_MAX + BST_N_ORI };

// what one record adds
struct bst_rec_t {
	uint32_t flags;                                                    // bit k: flag word k of column qc
	uint32_t qc;
	int32_t ref; bool placed_mapped;                                   // B: the contig (-1: unplaced) and whether 0x4 is clear
	bool primary, mapped;                                              // C: sum [] is what a primary record adds (BST_MAX_LEN: its l_seq); mapq counts with `mapped`
	uint64_t sum[BST_N_SUM]; uint32_t mapq;
	int ori; uint64_t size;                                            // D: the orientation (-1: the record does not count) and the size
};

// the tags of a mapped primary record of `size` bytes from byte p on: BST_OK (*has_nm, *nm: the first NM; *cg: a CG:B,I tag is there), BST_E_TAGS or BST_E_NM
BST_FN int bst_tags(const uint8_t *rec, uint64_t size, uint64_t p, bool *has_nm, uint64_t *nm, bool *cg)
{
	*has_nm = false; *nm = 0; *cg = false;
	if (p > size) return BST_E_TAGS;
	while (p < size) {
		if (size - p < 3) return BST_E_TAGS;
		const uint8_t a = rec[p], b = rec[p + 1], t = rec[p + 2];
		p += 3;
		const bool is_nm = a == 'N' && b == 'M' && !*has_nm;
		uint64_t len;
		if (t == 'A' || t == 'c' || t == 'C') len = 1;
		else if (t == 's' || t == 'S') len = 2;
		else if (t == 'i' || t == 'I' || t == 'f') len = 4;
		else if (t == 'Z' || t == 'H') {
			if (is_nm) return BST_E_NM;
			len = 0;
			while (p + len < size && rec[p + len]) ++len;
			if (p + len >= size) return BST_E_TAGS;
			++len;
		} else if (t == 'B') {
			if (is_nm) return BST_E_NM;
			if (size - p < 5) return BST_E_TAGS;
			const uint8_t s = rec[p];
			const uint64_t w = s == 'c' || s == 'C' ? 1 : s == 's' || s == 'S' ? 2 : s == 'i' || s == 'I' || s == 'f' ? 4 : 0;
			if (!w) return BST_E_TAGS;
			if (a == 'C' && b == 'G' && s == 'I') *cg = true;
			len = 5 + w * (uint64_t)bsr_u32(rec + p + 1);
		} else return BST_E_TAGS;
		if (len > size - p) return BST_E_TAGS;
		if (is_nm) {
			int64_t v;
			if (t == 'c') v = (int8_t)rec[p];
			else if (t == 'C') v = rec[p];
			else if (t == 's') v = (int16_t)bsr_u16(rec + p);
			else if (t == 'S') v = bsr_u16(rec + p);
			else if (t == 'i') v = (int32_t)bsr_u32(rec + p);
			else if (t == 'I') v = bsr_u32(rec + p);
			else return BST_E_NM;                                      // (A, f)
			if (v < 0) return BST_E_NM;
			*has_nm = true; *nm = (uint64_t)v;
		}
		p += len;
	}
	return BST_OK;
}

// the record of `size` bytes among n_contigs contigs -> what it adds (R), or why it is refused
BST_FN int bst_record(const uint8_t *rec, uint64_t size, int n_contigs, bst_rec_t &R)
{
	if (size < BSR_FIXED) return BST_E_CUT;
	const uint32_t n_ops = bsr_u16(rec + 16);
	const uint64_t ops_at = (uint64_t)BSR_FIXED + rec[12];
	if (ops_at + 4ull * n_ops > size) return BST_E_CUT;
	const uint32_t flag = bsr_flag(rec), mapq = rec[13];
	const int32_t ref = bsr_ref(rec), next_ref = (int32_t)bsr_u32(rec + 24);
	const uint64_t l_seq = bsr_u32(rec + 20);
	if (ref < -1 || ref >= n_contigs) return BST_E_REF;
	const bool unmapped = (flag & 0x4u) != 0, dup = (flag & 0x400u) != 0;
	R.qc = (flag & 0x200u) ? 1u : 0u;
	R.ref = ref; R.placed_mapped = !unmapped;
	R.primary = !(flag & 0x900u); R.mapped = R.primary && !unmapped; R.mapq = mapq;
	R.ori = -1; R.size = 0;
	for (int k = 0; k < BST_N_SUM; ++k) R.sum[k] = 0;
	// A
	uint32_t f = 1u << BST_TOTAL;
	if (flag & 0x100u) f |= 1u << BST_SECONDARY;
	else if (flag & 0x800u) f |= 1u << BST_SUPPLEMENTARY;
	else {
		f |= 1u << BST_PRIMARY;
		if (flag & 0x1u) {
			f |= 1u << BST_PAIRED;
			if ((flag & 0x2u) && !unmapped) f |= 1u << BST_PROPER;
			if (flag & 0x40u) f |= 1u << BST_READ1;
			if (flag & 0x80u) f |= 1u << BST_READ2;
			if ((flag & 0x8u) && !unmapped) f |= 1u << BST_SINGLETONS;
			if (!unmapped && !(flag & 0x8u)) {
				f |= 1u << BST_BOTH_MAPPED;
				if (next_ref != ref) { f |= 1u << BST_DIFF_CHR; if (mapq >= 5) f |= 1u << BST_DIFF_CHR_Q5; }
			}
		}
		if (!unmapped) f |= 1u << BST_PRIMARY_MAPPED;
		if (dup) f |= 1u << BST_PRIMARY_DUP;
	}
	if (!unmapped) f |= 1u << BST_MAPPED;
	if (dup) f |= 1u << BST_DUP;
	R.flags = f;
	if (!R.primary) return BST_OK;
	// C
	R.sum[BST_READS] = 1; R.sum[BST_BASES] = l_seq; R.sum[BST_MAX_LEN] = l_seq;
	if (!R.mapped) return BST_OK;
	R.sum[BST_READS_MAPPED] = 1; R.sum[BST_BASES_MAPPED] = l_seq; R.sum[BST_READS_MQ0] = mapq == 0;
	const uint8_t *c = rec + ops_at;
	uint64_t reflen = 0;
	for (uint32_t i = 0; i < n_ops; ++i) {
		const uint32_t v = bsr_u32(c + 4 * i), op = v & 15u; const uint64_t len = v >> 4;
		if (op == 0 || op == 7 || op == 8) { R.sum[BST_BASES_ALIGNED] += len; reflen += len; }
		else if (op == 1) { R.sum[BST_BASES_ALIGNED] += len; ++R.sum[BST_INS_EVENTS]; R.sum[BST_INS_BASES] += len; }
		else if (op == 2) { ++R.sum[BST_DEL_EVENTS]; R.sum[BST_DEL_BASES] += len; reflen += len; }
		else if (op == 3) reflen += len;
		else if (op == 4) R.sum[BST_BASES_CLIPPED] += len;
	}
	bool has_nm, cg; uint64_t nm;
	const int st = bst_tags(rec, size, ops_at + 4ull * n_ops + (l_seq + 1) / 2 + l_seq, &has_nm, &nm, &cg);
	if (st != BST_OK) return st;
	if (cg && n_ops == 2) {
		const uint32_t a = bsr_u32(c), b = bsr_u32(c + 4);
		if ((a & 15u) == 4u && (a >> 4) == l_seq && (b & 15u) == 3u) return BST_E_PLACEHOLDER;
	}
	if (has_nm) { R.sum[BST_READS_NM] = 1; R.sum[BST_EDIT_DISTANCE] = nm; }
	// D
	const int64_t tlen = (int32_t)bsr_u32(rec + 32);
	if ((flag & 0x81u) == 0x81u && !(flag & (0x8u | 0x400u)) && ref == next_ref && tlen != 0) {
		R.size = (uint64_t)(tlen < 0 ? -tlen : tlen);
		const bool rev = (flag & 0x10u) != 0, mrev = (flag & 0x20u) != 0;
		if (rev == mrev) R.ori = BST_TANDEM;
		else if (!rev) R.ori = tlen > 0 ? BST_FR : BST_RF;
		else R.ori = (int64_t)(int32_t)bsr_u32(rec + 28) + 1 < (int64_t)bsr_pos(rec) + (int64_t)reflen ? BST_FR : BST_RF;
	}
	return BST_OK;
}

BST_FN uint64_t bst_refusal(uint64_t index, int code) { return index << 3 | (uint64_t)code; }
BST_FN uint64_t bst_hist_at(int ori, uint64_t size, uint32_t cap) { return (uint64_t)ori * ((uint64_t)cap + 1) + (size < cap ? size : cap); }
