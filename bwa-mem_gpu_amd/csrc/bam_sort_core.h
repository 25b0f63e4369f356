// Coordinate order and the BAI or CSI index of BAM records (SAM spec sections 4.2 and 5.2): the per-record rules of csrc/bam_sort_kernels.hip (one lane per record)
// and, compiled as plain C++, of csrc/bam_sort_host.cpp and tests/bam_sort_core_host.cpp (under the sanitizers).
//
// A record: block_size refID pos l_read_name mapq bin n_cigar_op flag l_seq next_refID next_pos tlen | read_name\0 | cigar | ...  (little-endian, unaligned)
//
//   key      (uint32)refID << 32 | (uint32)(pos + 1) << 1 | reverse (flag 0x10) -- the order of `samtools sort`; refID -1 sorts last, equal keys keep
//            the order they came in (the sorts are stable)
//   end      pos + the reference length of the CIGAR (M, D, N, =, X), or pos + 1 when that length is 0 or the read is unmapped (flag 0x4)
//   virtual  the byte at `u` of a window's text whose members are cut every 0xff00 bytes: (file offset of member u / 0xff00) << 16 | u % 0xff00; the
//   offset   byte behind the window's text is byte 0 of the member that follows the window (its last member is short)
//   windows  a record of a reference overlaps the 16 KiB windows max(pos, 0) >> 14 .. (max(end, pos + 1) - 1) >> 14, clamped to the reference's last
//            window (n_win - 1: a record that runs off the end of its contig indexes there)
//   chunks   a record begins a chunk when it is the first of its window of records or its (refID, bin) differ from the record's before it
//
// The CSI index of the same file takes a binning scheme (min_shift, depth) in place of BAI's (14, 5):
//   min_shift  the linear windows and the deepest bins hold 2^min_shift bases (10 .. 24)
//   depth      the smallest d >= 0 with 2^(min_shift + 3 d) >= the longest contig (htslib's rule); at most 7 for contigs below 2^31
//   bin        level l (0: the deepest) begins at bin ((1 << 3 (depth - l)) - 1) / 7 and holds the windows >> 3 l; a record's bin is that of the deepest level
//              at which its first and last window (the windows above, at min_shift: pos < 0 as 0, clamped to the contig's last) fall together, 0 if none.  The
//              record's own 16-bit bin field is not read
//   pseudo-bin ((1 << 3 (depth + 1)) - 1) / 7 + 1 -- 37450 at depth 5
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BSR_FN __host__ __device__ inline
#else
#define BSR_FN inline
#endif

enum { BSR_PIECE = 0xff00, BSR_FIXED = 36, BSR_LIN_SHIFT = 14, BSR_META_BIN = 37450, BSR_MAX_CONTIG = 1 << 29 };
enum { BSR_IX_BAI = 0, BSR_IX_CSI = 1, BSR_CSI_SHIFT_MIN = 10, BSR_CSI_SHIFT_MAX = 24, BSR_BAI_DEPTH = 5 };

BSR_FN uint32_t bsr_u16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
BSR_FN uint32_t bsr_u32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

BSR_FN int32_t bsr_ref(const uint8_t *rec) { return (int32_t)bsr_u32(rec + 4); }
BSR_FN int32_t bsr_pos(const uint8_t *rec) { return (int32_t)bsr_u32(rec + 8); }
BSR_FN uint32_t bsr_bin(const uint8_t *rec) { return bsr_u16(rec + 14); }
BSR_FN uint32_t bsr_flag(const uint8_t *rec) { return bsr_u16(rec + 18); }

BSR_FN uint64_t bsr_key(const uint8_t *rec)
{
	return (uint64_t)bsr_u32(rec + 4) << 32 | (uint64_t)(uint32_t)((bsr_u32(rec + 8) + 1u) << 1) | ((bsr_flag(rec) >> 4) & 1u);
}

// the bytes of the record at rec, block_size included, when `avail` bytes are left; 0: no whole record lies there (a cut stream, or a block_size that
// cannot hold the fixed fields, the name and the operations it announces)
BSR_FN uint64_t bsr_record_bytes(const uint8_t *rec, uint64_t avail)
{
	if (avail < BSR_FIXED) return 0;
	const uint64_t sz = (uint64_t)bsr_u32(rec) + 4;
	if (sz > avail || sz < (uint64_t)BSR_FIXED + rec[12] + 4ull * bsr_u16(rec + 16)) return 0;
	return sz;
}

// the record's end on its reference, exclusive (reads the operations: bsr_record_bytes has vouched for them)
BSR_FN int64_t bsr_end(const uint8_t *rec)
{
	const int64_t pos = bsr_pos(rec);
	if (bsr_flag(rec) & 4u) return pos + 1;
	const uint8_t *c = rec + BSR_FIXED + rec[12];
	const uint32_t n = bsr_u16(rec + 16);
	int64_t rl = 0;
	for (uint32_t i = 0; i < n; ++i) {
		const uint32_t v = bsr_u32(c + 4 * i), op = v & 15u;
		if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rl += v >> 4;
	}
	return rl ? pos + rl : pos + 1;
}

// the windows of 2^shift bases the record overlaps, of a reference with n_win of them (n_win >= 1)
BSR_FN void bsr_windows_at(const uint8_t *rec, uint32_t n_win, int shift, uint32_t *lo, uint32_t *hi)
{
	int64_t b = bsr_pos(rec), e = bsr_end(rec);
	if (b < 0) b = 0;
	if (e <= b) e = b + 1;
	uint64_t l = (uint64_t)b >> shift, h = (uint64_t)(e - 1) >> shift;
	if (h >= n_win) h = n_win - 1;
	if (l > h) l = h;
	*lo = (uint32_t)l; *hi = (uint32_t)h;
}

// the windows of the linear index the record overlaps, of a reference with n_win of them (n_win >= 1)
BSR_FN void bsr_windows(const uint8_t *rec, uint32_t n_win, uint32_t *lo, uint32_t *hi) { bsr_windows_at(rec, n_win, BSR_LIN_SHIFT, lo, hi); }

// windows of 2^shift bases of a reference of `len` bases
BSR_FN uint32_t bsr_n_windows_at(int64_t len, int shift) { return len > 0 ? (uint32_t)(((uint64_t)len - 1) >> shift) + 1 : 1u; }
BSR_FN uint32_t bsr_n_windows(int64_t len) { return bsr_n_windows_at(len, BSR_LIN_SHIFT); }

// ---- the CSI binning scheme (min_shift, depth)

// the smallest d >= 0 with 2^(min_shift + 3 d) >= max_len (max_len below 2^31 and min_shift >= 10: at most 7)
BSR_FN int bsr_csi_depth(int64_t max_len, int min_shift)
{
	int d = 0;
	for (int64_t s = (int64_t)1 << min_shift; s < max_len; s <<= 3) ++d;
	return d;
}

// the first bin of level l (0: the deepest), and the pseudo-bin that holds a reference's counts
BSR_FN uint32_t bsr_csi_level_first(int depth, int l) { return ((1u << (3 * (depth - l))) - 1u) / 7u; }
BSR_FN uint32_t bsr_csi_meta_bin(int depth) { return ((1u << (3 * (depth + 1))) - 1u) / 7u + 1u; }

// the bin of a record whose first and last window are lo <= hi
BSR_FN uint32_t bsr_csi_bin(uint32_t lo, uint32_t hi, int depth)
{
	for (int l = 0; l <= depth; ++l, lo >>= 3, hi >>= 3)
		if (lo == hi) return bsr_csi_level_first(depth, l) + lo;
	return 0;
}

// the record's bin on a reference with n_win windows of 2^min_shift bases
BSR_FN uint32_t bsr_csi_rec_bin(const uint8_t *rec, uint32_t n_win, int min_shift, int depth)
{
	uint32_t lo, hi;
	bsr_windows_at(rec, n_win, min_shift, &lo, &hi);
	return bsr_csi_bin(lo, hi, depth);
}

// bsr_chunk_head (below) on (refID, CSI bin); n_win: the windows of the record's reference (not read when it has none)
BSR_FN bool bsr_csi_chunk_head(const uint8_t *rec, const uint8_t *prev, uint32_t n_win, int min_shift, int depth)
{
	if (!prev) return true;
	const int32_t r = bsr_ref(rec), p = bsr_ref(prev);
	if (r < 0) return p >= 0;
	return r != p || bsr_csi_rec_bin(rec, n_win, min_shift, depth) != bsr_csi_rec_bin(prev, n_win, min_shift, depth);
}

// the virtual offset of byte u of a window's text of `total` bytes; moff [n_members + 1]: the members' offsets from the window's first byte, `base` that
// byte's offset in the file
BSR_FN uint64_t bsr_voff(uint64_t base, const uint64_t *moff, uint64_t total, uint64_t u)
{
	if (u >= total) return (base + moff[(total + BSR_PIECE - 1) / BSR_PIECE]) << 16;
	return (base + moff[u / BSR_PIECE]) << 16 | (u % BSR_PIECE);
}

// does record j of a window begin a chunk (prev: the record before it, NULL for the window's first)
BSR_FN bool bsr_chunk_head(const uint8_t *rec, const uint8_t *prev)
{
	if (!prev) return true;
	const int32_t r = bsr_ref(rec), p = bsr_ref(prev);
	if (r < 0) return p >= 0;                     // the records without a reference form one group behind the others; it is in no bin
	return r != p || bsr_bin(rec) != bsr_bin(prev);
}
