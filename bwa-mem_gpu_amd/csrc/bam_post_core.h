// Sorting, marking and indexing a BAM or SAM that another program wrote: the rules that a foreign file needs and this project's own records
// never did -- per record, for csrc/bam_post_kernels.hip (one lane per record) and, compiled as plain C++, for csrc/bam_post.cpp, csrc/bam_dup_host.cpp and
// tests/bam_post_core_host.cpp (under the sanitizers).
//
//   template  BDP_TPL_NAME: a record heads a template when it is the first of the file or its name -- l_read_name and all its bytes -- differs from the name of
//             the record before it.  A template is a maximal run of adjacent records under one name, in any internal order; primary lines, kind, score, end
//             words, role and first record are bdp_entry's, applied to the run.  Names are unaligned: they are compared in 32-bit words assembled from bytes
//   bin       bytes 14-15 are recomputed as the SAM specification's reg2bin(pos, end): end is bsr_end's (pos + 1 for an unmapped record and for one without
//             reference-consuming operations); pos -1 gives 4680, as reg2bin(-1, 0) does
//   0x400     with marking the flag is cleared on every record before the decision, so a second run over the output gives the same file
//   checks    bpo_check, in this order (the smallest code of a record is reported, the smallest record of the file first):
//             CUT     the record does not hold the fields, name, operations, bases and qualities it announces (bsr_record_bytes, bdp_record_whole)
//             REF     refID or next_refID outside -1 .. n_ref - 1
//             PLACE   marking: a primary line without 0x4 has refID -1 or pos -1
//             END     marking: the unclipped 5' end u of a mapped primary line has u + 2^30 outside [0, 2^31) -- bdp_end_word assumes this aligner's clipping
//                     bound, a foreign hard clip has none
//             LONG    marking or coverage: the record holds the long-CIGAR placeholder (l_seq S, N, and a CG:B,I tag); a plain sort takes it
//   refusal   a 64-bit word index << 3 | code, the smallest of a batch through atomicMin; BPO_NONE: nothing was refused
#pragma once
#include "bam_dup_core.h"
#include "bam_cov_core.h"

enum { BPO_OK = 0, BPO_E_CUT = 1, BPO_E_REF = 2, BPO_E_PLACE = 3, BPO_E_END = 4, BPO_E_LONG = 5, BPO_E_TEMPLATE = 6 };
enum { BPO_MARKDUP = 1, BPO_COVERAGE = 2 };                           // what a run does beyond the sort: the checks' mode bits
#define BPO_NONE (~0ull)

BSR_FN uint64_t bpo_refusal(uint64_t index, int code) { return index << 3 | (uint64_t)code; }

// a 32-bit word of a name, from its bytes (records have no alignment)
BSR_FN uint32_t bpo_word(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// are the names of two records equal: l_read_name and every byte.  sa, sb: the records' bytes -- a record too short for its own name equals nothing
BSR_FN bool bpo_name_equal(const uint8_t *a, uint64_t sa, const uint8_t *b, uint64_t sb)
{
	if (sa < BSR_FIXED || sb < BSR_FIXED) return false;
	const uint32_t l = a[12];
	if (l != b[12] || sa - BSR_FIXED < l || sb - BSR_FIXED < l) return false;
	const uint8_t *x = a + BSR_FIXED, *y = b + BSR_FIXED;
	uint32_t k = 0;
	for (; k + 4 <= l; k += 4) if (bpo_word(x + k) != bpo_word(y + k)) return false;
	for (; k < l; ++k) if (x[k] != y[k]) return false;
	return true;
}

// does record i of a stream with offsets off [n + 1] head a template under BDP_TPL_NAME
BSR_FN bool bpo_head(const uint8_t *recs, const uint64_t *off, uint32_t i)
{
	return i == 0 || !bpo_name_equal(recs + off[i], off[i + 1] - off[i], recs + off[i - 1], off[i] - off[i - 1]);
}

// the SAM specification's reg2bin of [beg, end)
BSR_FN uint32_t bpo_reg2bin(int64_t beg, int64_t end)
{
	--end;
	if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
	if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
	if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
	if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
	if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
	return 0;
}

// the bin of a record whose operations lie inside it (the low 16 bits: what the field holds)
BSR_FN uint32_t bpo_bin(const uint8_t *rec)
{
	const int64_t pos = bsr_pos(rec);
	if (pos < 0) return 4680u;
	return bpo_reg2bin(pos, bsr_end(rec)) & 0xffffu;
}

// the unclipped 5' end of a mapped record, as bdp_end_word computes it, in 64 bits
BSR_FN int64_t bpo_unclipped(const uint8_t *rec)
{
	const uint8_t *c = rec + BSR_FIXED + rec[12];
	const uint32_t n = bsr_u16(rec + 16);
	int64_t u;
	if (!(bsr_flag(rec) & 0x10u)) {
		u = bsr_pos(rec);
		for (uint32_t i = 0; i < n; ++i) { const uint32_t v = bsr_u32(c + 4 * i), op = v & 15u; if (op != 4 && op != 5) break; u -= v >> 4; }
	} else {
		u = bsr_end(rec) - 1;
		for (uint32_t i = n; i > 0; --i) { const uint32_t v = bsr_u32(c + 4 * (i - 1)), op = v & 15u; if (op != 4 && op != 5) break; u += v >> 4; }
	}
	return u;
}

// does the record hold the long-CIGAR placeholder (bcv_check's test)
BSR_FN bool bpo_placeholder(const uint8_t *rec, uint64_t sz)
{
	if (bcv_n_ops(rec) != 2) return false;
	const uint8_t *c = rec + BSR_FIXED + rec[12];
	const uint32_t a = bsr_u32(c), b = bsr_u32(c + 4);
	return (a & 15u) == 4u && (a >> 4) == bsr_u32(rec + 20) && (b & 15u) == 3u && bcv_has_cg(rec, sz);
}

// the checks of one record of sz bytes (the chain has it end inside the stream) in a file of n_ref references; mode: BPO_MARKDUP | BPO_COVERAGE
BSR_FN int bpo_check(const uint8_t *rec, uint64_t sz, int32_t n_ref, uint32_t mode)
{
	if (bsr_record_bytes(rec, sz) != sz || !bdp_record_whole(rec, sz)) return BPO_E_CUT;
	const int32_t r = bsr_ref(rec), nr = (int32_t)bsr_u32(rec + 24);
	if (r < -1 || r >= n_ref || nr < -1 || nr >= n_ref) return BPO_E_REF;
	if (mode & BPO_MARKDUP) {
		const uint32_t fl = bsr_flag(rec);
		if (bdp_primary(fl) && !(fl & 4u)) {
			if (r < 0 || bsr_pos(rec) < 0) return BPO_E_PLACE;
			const int64_t u = bpo_unclipped(rec) + ((int64_t)1 << 30);
			if (u < 0 || u >= (int64_t)1 << 31) return BPO_E_END;
		}
	}
	if (mode && bpo_placeholder(rec, sz)) return BPO_E_LONG;
	return BPO_OK;
}

// check and fix: the record's refusal code, or BPO_OK with its bin recomputed and, with marking, 0x400 cleared.  *changed: bit 0 the bin changed, bit 1 the flag
// was cleared.  Byte stores only: records have no alignment
BSR_FN int bpo_fix(uint8_t *rec, uint64_t sz, int32_t n_ref, uint32_t mode, uint32_t *changed)
{
	*changed = 0;
	const int st = bpo_check(rec, sz, n_ref, mode);
	if (st != BPO_OK) return st;
	const uint32_t bin = bpo_bin(rec);
	if (bin != bsr_bin(rec)) { rec[14] = (uint8_t)bin; rec[15] = (uint8_t)(bin >> 8); *changed |= 1u; }
	if ((mode & BPO_MARKDUP) && (rec[19] & 0x04u)) { rec[19] = (uint8_t)(rec[19] & ~0x04u); *changed |= 2u; }
	return BPO_OK;
}
