// Coordinate order and the BAI index of BAM records (SAM spec sections 4.2 and 5.2): the per-record rules of csrc/bam_sort_kernels.hip (one lane per record)
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
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BSR_FN __host__ __device__ inline
#else
#define BSR_FN inline
#endif

enum { BSR_PIECE = 0xff00, BSR_FIXED = 36, BSR_LIN_SHIFT = 14, BSR_META_BIN = 37450, BSR_MAX_CONTIG = 1 << 29 };

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

// the windows of the linear index the record overlaps, of a reference with n_win of them (n_win >= 1)
BSR_FN void bsr_windows(const uint8_t *rec, uint32_t n_win, uint32_t *lo, uint32_t *hi)
{
	int64_t b = bsr_pos(rec), e = bsr_end(rec);
	if (b < 0) b = 0;
	if (e <= b) e = b + 1;
	uint64_t l = (uint64_t)b >> BSR_LIN_SHIFT, h = (uint64_t)(e - 1) >> BSR_LIN_SHIFT;
	if (h >= n_win) h = n_win - 1;
	if (l > h) l = h;
	*lo = (uint32_t)l; *hi = (uint32_t)h;
}

// windows of a reference of `len` bases
BSR_FN uint32_t bsr_n_windows(int64_t len) { return len > 0 ? (uint32_t)(((uint64_t)len - 1) >> BSR_LIN_SHIFT) + 1 : 1u; }

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
