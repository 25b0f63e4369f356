// What the SAM writer needs of a batch, chosen and packed ON THE DEVICE (the host side of gase_aln around the
// device path).  Until round 4 the records of the region tail went to the host, one host pass chose the records that need a CIGAR
// (bmh_sam_need_cigar: the reported ones and the XA candidates of mem_gen_alt, /root/reference/src/bwamem_extra.c:97-150), the list went
// back to the device, and the CIGAR / MD arrays came home as fixed slots of 64 + 96 bytes an alignment of which a typical alignment
// uses 4 + 4.  Both are a few microseconds of device work:
//   * bmh_sam_select_device: the same selection, one lane per read, over the records where bmh_finalize_regs_device left them;
//   * bmh_cigar_pack_sizes / bmh_cigar_pack: the operations and the MD string of every alignment back to back in one array of words.
#include <hip/hip_runtime.h>
#include <cstring>
#include <rocprim/rocprim.hpp>
#include <cstdint>
#include <cstdlib>
#include "bmh_internal.h"
#include "devmem.h"
#include "sam_core.h"

namespace {

struct sel_args_t {
	const int32_t *fin; const uint32_t *opr; const uint32_t *off; const int32_t *h_rec;
	uint32_t n_reads; uint32_t *cnt, *flag;
	int flag_all, sa, max_XA_hits, max_XA_hits_alt; double drop;
};

// bmh_sam_need_cigar (csrc/sam_format.cpp) by the same two rules of csrc/sam_core.h, one RECORD per lane (a record carries its read in field [0]; a lane per read
// spent its time in the serial loops of the few reads with hundreds of records): first cnt[k] = hits listed under primary k (bit 31: one of them on an ALT contig),
// then need = reported, or an XA candidate whose primary lists no more hits than the XA limits allow
__global__ void __launch_bounds__(256) sam_count_kernel(sel_args_t A, uint64_t m)
{
	const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
	if (g >= m) return;
	const uint32_t r = (uint32_t)A.fin[16 * g];
	const uint64_t base = A.off[r];
	const int k = sam_core::xa_primary(A.fin + 16 * base, (int)(g - base), A.sa, A.drop);
	if (k >= 0) {
		atomicAdd(A.cnt + base + (uint64_t)k, 1u);
		if (A.fin[16 * g + 15] & 2) atomicOr(A.cnt + base + (uint64_t)k, 0x80000000u);
	}
}
__global__ void __launch_bounds__(256) sam_select_kernel(sel_args_t A, uint64_t m)
{
	const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
	if (g >= m) return;
	const uint32_t r = (uint32_t)A.fin[16 * g];
	const uint64_t base = A.off[r];
	const int i = (int)(g - base);
	uint32_t need = (A.fin[16 * g + 15] & 1) ? 1u : 0u;
	if (!A.flag_all) {
		const int k = sam_core::xa_primary(A.fin + 16 * base, i, A.sa, A.drop);
		if (k >= 0) {
			const uint32_t c = A.cnt[base + (uint64_t)k];
			if (sam_core::xa_listed((int)(c & 0x7FFFFFFFu), c >> 31, A.max_XA_hits, A.max_XA_hits_alt)) need = 1u;
		}
	}
	if (A.h_rec && A.h_rec[r] == i) need = 1u;                   // pairs: the read's own alignment lends its mate the mate fields
	A.flag[g] = need;
}

__global__ void __launch_bounds__(256) sam_sel_scatter_kernel(const uint32_t *flag, const uint32_t *pos, uint64_t m, uint32_t *sel, int32_t *slot, uint32_t *total)
{
	const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
	if (i >= m) return;
	const uint32_t f = flag[i], p = pos[i];
	slot[i] = f ? (int32_t)p : -1;
	if (f) sel[p] = (uint32_t)i;
	if (i == m - 1) *total = p + f;
}

// words an alignment takes in the packed array: its operations, then its MD string with the NUL, padded to a word; an alignment that overflowed
// the fixed slots (flags 1, 8: the caller redoes it with larger ones) or was rejected takes none
__global__ void __launch_bounds__(256) cigar_words_kernel(const int32_t *aln, uint32_t n, int with_md, uint32_t *words)
{
	const uint32_t k = blockIdx.x * 256u + threadIdx.x;
	if (k > n) return;
	uint32_t w = 0;
	if (k < n) {
		const int32_t *a = aln + 8 * (size_t)k;
		if (!(a[7] & ~2)) w = (uint32_t)a[3] + (with_md ? ((uint32_t)a[6] + 4u) >> 2 : 0u);
	}
	words[k] = w;
}

__global__ void __launch_bounds__(256) cigar_pack_kernel(const int32_t *aln, const uint32_t *cigar, int max_cigar, const char *md, int md_cap, uint32_t n,
                                                         const uint32_t *off, uint32_t *packed)
{
	const uint32_t k = blockIdx.x * 256u + threadIdx.x;
	if (k >= n) return;
	const int32_t *a = aln + 8 * (size_t)k;
	if (a[7] & ~2) return;
	uint32_t *o = packed + off[k];
	const int nc = a[3];
	const uint32_t *cg = cigar + (size_t)max_cigar * k;
	for (int i = 0; i < nc; ++i) o[i] = cg[i];
	if (md) {
		const uint32_t *ms = (const uint32_t *)(md + (size_t)md_cap * k);       // (md_cap is a multiple of 4: checked by the host)
		const int nw = (a[6] + 4) >> 2;
		for (int i = 0; i < nw; ++i) o[nc + i] = ms[i];
	}
}

size_t scan_bytes(size_t n)
{
	size_t t = 0;
	(void)rocprim::exclusive_scan(nullptr, t, (uint32_t *)nullptr, (uint32_t *)nullptr, 0u, n, rocprim::plus<uint32_t>(), 0);
	return (t + 255) & ~(size_t)255;
}
inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

}   // namespace

extern "C" size_t bmh_sam_select_work(uint32_t n_reads, uint64_t m)
{
	return al256(4 * ((size_t)n_reads + 1)) + 3 * al256(4 * (size_t)(m + 1)) + scan_bytes((size_t)(m > n_reads ? m : n_reads) + 1) + 512;
}

extern "C" int64_t bmh_sam_select_device(const bmh_post_opt_t *popt, const int32_t *d_fin, const uint32_t *d_fin_per_read, const int32_t *d_h_rec,
                                         uint32_t n_reads, uint64_t m, uint32_t *d_sel, int32_t *d_slot, void *d_work, size_t work_bytes, void *stream_)
{
	if (!popt || (n_reads && !d_fin_per_read) || (m && (!d_fin || !d_sel || !d_slot)) || !d_work) { bmh_set_error("bmh_sam_select_device: null argument"); return BMH_EINVAL; }
	if (work_bytes < bmh_sam_select_work(n_reads, m)) { bmh_set_error("bmh_sam_select_device: %zu bytes of work space, bmh_sam_select_work asks for %zu", work_bytes, bmh_sam_select_work(n_reads, m)); return BMH_EINVAL; }
	if (m >> 31) { bmh_set_error("bmh_sam_select_device: 2^31 records or more in one batch"); return BMH_ECAPACITY; }
	if (n_reads == 0 || m == 0) return 0;
	hipStream_t st = (hipStream_t)stream_;
	uint8_t *w = (uint8_t *)d_work;
	uint32_t *off = (uint32_t *)w; w += al256(4 * ((size_t)n_reads + 1));
	uint32_t *cnt = (uint32_t *)w; w += al256(4 * (size_t)(m + 1));
	uint32_t *flag = (uint32_t *)w; w += al256(4 * (size_t)(m + 1));
	uint32_t *pos = (uint32_t *)w; w += al256(4 * (size_t)(m + 1));
	uint32_t *total = (uint32_t *)w; w += 256;
	void *tmp = w;
	size_t tb = scan_bytes((size_t)(m > n_reads ? m : n_reads) + 1);
	HIPCK(rocprim::exclusive_scan(tmp, tb, d_fin_per_read, off, 0u, (size_t)n_reads, rocprim::plus<uint32_t>(), st));
	sel_args_t A;
	A.fin = d_fin; A.opr = d_fin_per_read; A.off = off; A.h_rec = d_h_rec; A.n_reads = n_reads; A.cnt = cnt; A.flag = flag;
	A.flag_all = popt->flag_all; A.sa = popt->contig_is_alt ? 11 : 12; A.max_XA_hits = popt->max_XA_hits; A.max_XA_hits_alt = popt->max_XA_hits_alt;
	A.drop = (double)popt->XA_drop_ratio;
	// (field [0] of a record is its read's index in the batch: bmh_finalize_regs*, bmh_finalize_pairs*)
	HIPCK(hipMemsetAsync(cnt, 0, 4 * (size_t)m, st));
	if (!A.flag_all) sam_count_kernel<<<(unsigned)((m + 255) / 256), 256, 0, st>>>(A, m);
	sam_select_kernel<<<(unsigned)((m + 255) / 256), 256, 0, st>>>(A, m);
	tb = scan_bytes((size_t)(m > n_reads ? m : n_reads) + 1);
	HIPCK(rocprim::exclusive_scan(tmp, tb, flag, pos, 0u, (size_t)m, rocprim::plus<uint32_t>(), st));
	sam_sel_scatter_kernel<<<(unsigned)((m + 255) / 256), 256, 0, st>>>(flag, pos, m, d_sel, d_slot, total);
	uint32_t h = 0;
	HIPCK(hipMemcpyAsync(&h, total, 4, hipMemcpyDeviceToHost, st));
	HIPCK(hipStreamSynchronize(st));
	HIPCK(hipGetLastError());
	return (int64_t)h;
}

extern "C" size_t bmh_cigar_pack_work(uint32_t n) { return al256(4 * ((size_t)n + 2)) + scan_bytes((size_t)n + 2) + 256; }

extern "C" int64_t bmh_cigar_pack_sizes(const int32_t *d_aln, uint32_t n, int with_md, uint32_t *d_off, void *d_work, size_t work_bytes, void *stream_)
{
	if ((n && !d_aln) || !d_off || !d_work) { bmh_set_error("bmh_cigar_pack_sizes: null argument"); return BMH_EINVAL; }
	if (work_bytes < bmh_cigar_pack_work(n)) { bmh_set_error("bmh_cigar_pack_sizes: %zu bytes of work space, bmh_cigar_pack_work asks for %zu", work_bytes, bmh_cigar_pack_work(n)); return BMH_EINVAL; }
	hipStream_t st = (hipStream_t)stream_;
	uint8_t *w = (uint8_t *)d_work;
	uint32_t *words = (uint32_t *)w; w += al256(4 * ((size_t)n + 2));
	cigar_words_kernel<<<(n + 1 + 255) / 256, 256, 0, st>>>(d_aln, n, with_md, words);
	size_t tb = scan_bytes((size_t)n + 2);
	HIPCK(rocprim::exclusive_scan((void *)w, tb, words, d_off, 0u, (size_t)n + 1, rocprim::plus<uint32_t>(), st));      // d_off[n] = the total
	uint32_t h = 0;
	HIPCK(hipMemcpyAsync(&h, d_off + n, 4, hipMemcpyDeviceToHost, st));
	HIPCK(hipStreamSynchronize(st));
	HIPCK(hipGetLastError());
	return (int64_t)h;
}

extern "C" int bmh_cigar_pack(const int32_t *d_aln, const uint32_t *d_cigar, int max_cigar, const char *d_md, int md_cap, uint32_t n, const uint32_t *d_off,
                              uint32_t *d_packed, void *stream_)
{
	if (n == 0) return BMH_OK;
	if (!d_aln || !d_cigar || !d_off || !d_packed || max_cigar < 1 || (d_md && (md_cap < 4 || (md_cap & 3)))) { bmh_set_error("bmh_cigar_pack: bad argument (md_cap must be a multiple of 4)"); return BMH_EINVAL; }
	cigar_pack_kernel<<<(n + 255) / 256, 256, 0, (hipStream_t)stream_>>>(d_aln, d_cigar, max_cigar, d_md, md_cap, n, d_off, d_packed);
	HIPCK(hipGetLastError());
	return BMH_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// The SAM text itself on the device: bmh_format_sam / bmh_format_sam_pe (csrc/sam_format.cpp; mem_aln2sam, /root/reference/src/bwamem.c:
// 1506-1683; mem_gen_alt, src/bwamem_extra.c:97-150), one read per lane, two passes over the same code: the first counts the bytes of every
// read's records, a scan places them, the second writes.  On the host the text of a million reads was 0.9 s of CPU time (14 ms on 64
// threads) and needed the records, the alignments and the CIGAR / MD arrays in host memory: 300 MB of copies for 230 MB of text.  Here the
// text is the only thing that leaves the device.  What a record says is csrc/sam_core.h (read_records), shared with the host formatter: ALT-mode
// records (soft clips on ALT hits, the larger XA limit, pa:f) included.
namespace {

struct sam_args_t {
	bmh_sam_dev_t d;
	const uint32_t *rec_off;       // [n_reads] first record of every read
	uint32_t *len; const uint64_t *text_off; char *text; uint32_t *err;
	int flag_all, max_XA_hits, max_XA_hits_alt, no_multi, softclip; double drop;
	int sa;                        // field of a record that holds the XA tag's key: [12] secondary, with ALT contigs [11] secondary_all (bmh_post_opt_t)
	int rg_len; char rg[256];      // read group id (bmh_post_opt_t::rg_id), 0 = none
	int copy_comment;              // -C with comments given (d.d_comments): every record ends with its read's comment
};

// where the text goes: sam_core::count_out counts the bytes, ptr_out<char *> writes them to global memory, ptr_out<sam_lds_char *> into the wave's image in LDS
// (copied out in dwords afterwards: a lane's byte stores to global memory are one memory transaction each, 230 M of them for a million reads)
typedef __attribute__((address_space(3))) char sam_lds_char;

// sam_core's Src over the device arrays: ASCII reads, name blobs with [n + 1] offsets (NUL-terminated back to back: no strlen), 32-bit slots, packed words
struct sam_src_t {
	const sam_args_t &A;
	struct read_t {
		const sam_args_t &A; uint64_t base; int n; const int32_t *fin;
		__device__ __forceinline__ sam_core::aln_t aln(int i) const
		{
			sam_core::aln_t x; x.aln = nullptr; x.cigar = nullptr; x.md = nullptr;
			const int32_t s = A.d.d_slot[base + (uint64_t)i];
			if (s >= 0) {
				x.aln = A.d.d_aln + 8 * (size_t)s;
				if (x.aln[7] & ~2) { x.aln = nullptr; return x; }       // (an alignment bmh_cigar_batch flagged has no words in the packed array)
				x.cigar = A.d.d_packed + A.d.d_cig_off[s]; x.md = (const char *)(x.cigar + x.aln[3]);
			}
			return x;
		}
	};
	__device__ __forceinline__ read_t read(uint32_t r) const { const uint64_t base = A.rec_off[r]; return read_t{A, base, (int)A.d.d_fin_per_read[r], A.d.d_fin + 16 * base}; }
	__device__ __forceinline__ bool flag_all() const { return A.flag_all; }
	__device__ __forceinline__ bool softclip() const { return A.softclip; }
	__device__ __forceinline__ int sa() const { return A.sa; }
	__device__ __forceinline__ double drop() const { return A.drop; }
	__device__ __forceinline__ int max_XA_hits() const { return A.max_XA_hits; }
	__device__ __forceinline__ int max_XA_hits_alt() const { return A.max_XA_hits_alt; }
	__device__ __forceinline__ const char *rg() const { return A.rg; }
	__device__ __forceinline__ int rg_len() const { return A.rg_len; }
	// per-read read groups (d_read_group): the read's ID out of the table; an index outside it raises flag 4 and writes no tag
	__device__ __forceinline__ const char *rg_read(uint32_t r, int &len) const
	{
		if (!A.d.d_read_group) { len = A.rg_len; return A.rg; }
		const uint32_t g = A.d.d_read_group[r];
		if (g >= A.d.n_rg) { atomicOr(A.err, 4u); len = 0; return A.rg; }
		const uint32_t o = A.d.d_rg_id_off[g];
		len = (int)(A.d.d_rg_id_off[g + 1] - o);
		return A.d.d_rg_ids + o;
	}
	__device__ __forceinline__ bool paired() const { return A.d.d_h_rec != nullptr; }
	__device__ __forceinline__ int h_rec(uint32_t r) const { return A.d.d_h_rec[r]; }
	__device__ __forceinline__ int unflag(uint32_t r) const { return A.d.d_unflag ? A.d.d_unflag[r] : 0; }
	__device__ __forceinline__ int md_len(const sam_core::aln_t &x) const { return x.aln[6]; }
	__device__ __forceinline__ const char *name(uint32_t r) const { return A.d.d_names + A.d.d_name_off[r]; }
	__device__ __forceinline__ int name_len(uint32_t r) const { return (int)(A.d.d_name_off[r + 1] - A.d.d_name_off[r]) - 1; }
	__device__ __forceinline__ int l_seq(uint32_t r) const { return (int)A.d.d_lens[r]; }
	__device__ __forceinline__ const uint8_t *seq(uint32_t r) const { return A.d.d_reads + A.d.d_offs[r]; }
	__device__ __forceinline__ const uint8_t *qual(uint32_t r) const { return A.d.d_quals ? A.d.d_quals + A.d.d_offs[r] : nullptr; }       // (FASTQ: the qualities at the letters' offsets)
	__device__ __forceinline__ const char *comment(uint32_t r, int &len) const                                                        // (-C: NUL-terminated back to back like the names)
	{
		if (!A.copy_comment) return nullptr;
		len = (int)(A.d.d_comment_off[r + 1] - A.d.d_comment_off[r]) - 1;
		return A.d.d_comments + A.d.d_comment_off[r];
	}
	// the letter SEQ shows for a read's letter: upper case, N for everything that is not A C G T; complemented on the reverse strand
	// (eight letters in flight at a time, and the whole wave copying read after read in coalesced steps, were both tried: the writing pass is bound
	// by its two waves per SIMD -- 16 KB of LDS per wave -- and the dependent loads of the records, not by these bytes)
	__device__ __forceinline__ char letter(uint8_t c, bool rev) const
	{
		c &= 0xDF;
		const bool a = c == 'A', cc = c == 'C', g = c == 'G', t = c == 'T';
		if (!rev) return (a || cc || g || t) ? (char)c : 'N';
		return a ? 'T' : cc ? 'G' : g ? 'C' : t ? 'A' : 'N';
	}
	__device__ __forceinline__ int n_contigs() const { return A.d.n_contigs; }
	__device__ __forceinline__ long long ctg_off(int i) const { return A.d.d_contig_offset[i]; }
	__device__ __forceinline__ long long ctg0(int rid) const { return A.d.n_contigs > 1 ? A.d.d_contig_offset[rid] : 0; }
	__device__ __forceinline__ const char *ctg(int rid) const { return A.d.d_contig_names + A.d.d_contig_name_off[rid]; }
	__device__ __forceinline__ int ctg_len(int rid) const { return (int)(A.d.d_contig_name_off[rid + 1] - A.d.d_contig_name_off[rid]) - 1; }
};

// first pass: the bytes of every read's records
__global__ void __launch_bounds__(256) sam_text_count_kernel(sam_args_t A)
{
	const uint32_t r = blockIdx.x * 256u + threadIdx.x;
	if (r >= A.d.n_reads) return;
	sam_core::count_out o;
	const bool ok = sam_core::read_records(sam_src_t{A}, r, o) < 0;
	if (!ok) atomicOr(A.err, 1u);
	A.len[r] = ok ? o.n : 0u;
}

// second pass: a wave writes the records of its 64 reads -- one piece of the text -- into LDS, every lane its read's, and copies the piece out in
// dwords.  A piece beyond the wave's share of LDS (300 bp reads: 64 records are 24 KB) is cut into halves, quarters, .. of the wave's reads, written one after
// the other (the lanes of the others wait: still LDS stores and one coalesced copy instead of records written to global memory byte by byte -- 300 bp reads:
// 14.6 -> 11.1 ms per million reads beside the other lane's kernels); only a single read whose records exceed the share (long XA lists) writes to global memory directly
#define SAM_LDS_WAVE 16384
__global__ void __launch_bounds__(256) sam_text_write_kernel(sam_args_t A)
{
	__shared__ __attribute__((aligned(16))) char lds[4][SAM_LDS_WAVE];
	const uint32_t n = A.d.n_reads;
	const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
	const uint32_t r0 = blockIdx.x * 256u + wv * 64u, r = r0 + lane;
	if (r0 >= n) return;
	const uint32_t r1 = r0 + 64u < n ? r0 + 64u : n;
	// reads per part: the largest power of two whose parts all fit
	uint32_t per = 64u;
	for (;;) {
		bool fits = true;
		for (uint32_t b = r0; b < r1 && fits; b += per) {
			const uint32_t e = b + per < r1 ? b + per : r1;
			fits = A.text_off[e] - A.text_off[b] + 3u <= SAM_LDS_WAVE;
		}
		if (fits || per == 1u) break;
		per >>= 1;
	}
	for (uint32_t b = r0; b < r1; b += per) {                                         // (wave-uniform)
		const uint32_t e = b + per < r1 ? b + per : r1;
		const uint64_t t0 = A.text_off[b], t1 = A.text_off[e];
		const uint32_t a = (uint32_t)((uintptr_t)(A.text + t0) & 3u);              // the image starts where its first byte sits in a dword of the text
		const bool mine = r >= b && r < e;
		if (t1 - t0 + a <= SAM_LDS_WAVE) {
			sam_lds_char *img = (sam_lds_char *)lds[wv] + a;
			if (mine) {
				sam_core::ptr_out<sam_lds_char *> o{img + (uint32_t)(A.text_off[r] - t0)};
				const bool ok = sam_core::read_records(sam_src_t{A}, r, o) < 0;
				if (ok && (uint32_t)(o.p - img) != (uint32_t)(A.text_off[r + 1] - t0)) atomicOr(A.err, 2u);   // (the two passes disagree: internal error)
				if (!ok) { atomicOr(A.err, 1u); }
			}
			__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
			__builtin_amdgcn_s_waitcnt(0xC07F);                                       // (the wave's LDS stores are done: lgkmcnt 0)
			const uint32_t len = (uint32_t)(t1 - t0);
			char *dst = A.text + t0;
			const uint32_t head = len < ((4u - a) & 3u) ? len : ((4u - a) & 3u);
			if (lane < head) dst[lane] = img[lane];
			const uint32_t body = (len - head) >> 2;
			const uint32_t *src32 = (const uint32_t *)(lds[wv] + a + head);           // (a + head is a multiple of 4, or the piece ended)
			uint32_t *dst32 = (uint32_t *)(dst + head);
			for (uint32_t i = lane; i < body; i += 64u) dst32[i] = src32[i];
			const uint32_t tail0 = head + 4u * body;
			if (tail0 + lane < len) dst[tail0 + lane] = img[tail0 + lane];
			__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
			__builtin_amdgcn_s_waitcnt(0xC07F);                                       // (the copy has read the image before the next part overwrites it)
		} else if (mine) {
			sam_core::ptr_out<char *> o{A.text + A.text_off[r]};
			const bool ok = sam_core::read_records(sam_src_t{A}, r, o) < 0;
			if (!ok) atomicOr(A.err, 1u);
			else if ((uint64_t)(o.p - A.text) != A.text_off[r + 1]) atomicOr(A.err, 2u);
		}
	}
}

size_t scan64_bytes(size_t n)
{
	size_t t = 0;
	(void)rocprim::exclusive_scan(nullptr, t, (uint32_t *)nullptr, (uint64_t *)nullptr, (uint64_t)0, n, rocprim::plus<uint64_t>(), 0);
	return (t + 255) & ~(size_t)255;
}

int sam_args(const bmh_post_opt_t *popt, const bmh_sam_dev_t *d, const char *fn, sam_args_t &A)
{
	if (!popt || !d) { bmh_set_error("%s: null argument", fn); return BMH_EINVAL; }
	if (d->n_reads && (!d->d_names || !d->d_name_off || !d->d_reads || !d->d_offs || !d->d_lens || !d->d_contig_names || !d->d_contig_name_off || !d->d_fin_per_read ||
	                   !d->d_slot || !d->d_aln || !d->d_cig_off || !d->d_packed || (d->n_contigs > 1 && !d->d_contig_offset) || (d->d_h_rec && (!d->d_unflag || (d->n_reads & 1))) ||
	                   (!d->d_comments) != (!d->d_comment_off) || (d->d_read_group && (!d->d_rg_ids || !d->d_rg_id_off || !d->n_rg)))) {
		bmh_set_error("%s: null argument", fn); return BMH_EINVAL;
	}
	if (d->d_read_group && popt->rg_id && popt->rg_id[0]) { bmh_set_error("%s: per-read read groups (d_read_group) beside the options' one read group (rg_id '%s')", fn, popt->rg_id); return BMH_EINVAL; }
	memset(&A, 0, sizeof(A));
	A.d = *d;
	A.flag_all = popt->flag_all; A.max_XA_hits = popt->max_XA_hits; A.max_XA_hits_alt = popt->max_XA_hits_alt; A.no_multi = popt->no_multi; A.softclip = popt->softclip;
	A.drop = (double)popt->XA_drop_ratio;
	A.sa = popt->contig_is_alt ? 11 : 12;
	A.copy_comment = popt->copy_comment && d->d_comments ? 1 : 0;
	if (popt->rg_id && popt->rg_id[0]) {
		const size_t l = strlen(popt->rg_id);
		if (l > 255) { bmh_set_error("%s: the read group id is longer than 255 characters", fn); return BMH_EINVAL; }
		A.rg_len = (int)l; memcpy(A.rg, popt->rg_id, l);
	}
	return BMH_OK;
}

// ALT contigs in the native pipeline (csrc/align_pipeline.hip): the device tail runs without the table; its records become ALT-mode records in place ([11] = secondary_all,
// which without a hit on an ALT contig is the secondary), and the reads the host has redone with the table take theirs
__global__ void __launch_bounds__(256) alt_records_kernel(int32_t *fin, uint64_t m)
{
	const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
	if (k < m) fin[16 * k + 11] = fin[16 * k + 12];
}
__global__ void __launch_bounds__(256) alt_scatter_kernel(int32_t *fin, const uint32_t *rec_off, const uint32_t *ids, const uint32_t *sub_off, const int32_t *sub, uint32_t ns)
{
	const uint32_t t = blockIdx.x * 256u + threadIdx.x, j = t >> 4, l = t & 15u;
	if (j >= ns) return;
	const uint32_t n = sub_off[j + 1] - sub_off[j];
	const int4 *src = (const int4 *)(sub + 16 * (size_t)sub_off[j]);
	int4 *dst = (int4 *)(fin + 16 * (size_t)rec_off[ids[j]]);
	for (uint32_t q = l; q < 4 * n; q += 16) dst[q] = src[q];
}

}   // namespace

int bmh_alt_records_device(int32_t *d_fin, uint64_t m, const uint32_t *d_rec_off, const uint32_t *d_ids, const uint32_t *d_sub_off, const int32_t *d_sub, uint32_t ns, void *stream)
{
	hipStream_t st = (hipStream_t)stream;
	if (m) alt_records_kernel<<<(unsigned)((m + 255) / 256), 256, 0, st>>>(d_fin, m);
	if (ns) alt_scatter_kernel<<<(unsigned)(((size_t)ns * 16 + 255) / 256), 256, 0, st>>>(d_fin, d_rec_off, d_ids, d_sub_off, d_sub, ns);
	HIPCK(hipGetLastError());
	return BMH_OK;
}

extern "C" size_t bmh_sam_text_work(uint32_t n_reads)
{
	return 2 * al256(4 * ((size_t)n_reads + 2)) + scan_bytes((size_t)n_reads + 2) + scan64_bytes((size_t)n_reads + 2) + 512;
}

extern "C" int64_t bmh_sam_text_sizes(const bmh_post_opt_t *popt, const bmh_sam_dev_t *d, uint64_t *d_text_off, void *d_work, size_t work_bytes, void *stream_)
{
	sam_args_t A;
	const int rc = sam_args(popt, d, "bmh_sam_text_sizes", A);
	if (rc != BMH_OK) return rc;
	if (!d_text_off || !d_work || work_bytes < bmh_sam_text_work(d->n_reads)) { bmh_set_error("bmh_sam_text_sizes: the work space is smaller than bmh_sam_text_work asks for"); return BMH_EINVAL; }
	const uint32_t n = d->n_reads;
	hipStream_t st = (hipStream_t)stream_;
	if (n == 0) return 0;
	uint8_t *w = (uint8_t *)d_work;
	uint32_t *rec_off = (uint32_t *)w; w += al256(4 * ((size_t)n + 2));
	uint32_t *len = (uint32_t *)w; w += al256(4 * ((size_t)n + 2));
	uint32_t *err = (uint32_t *)w; w += 256;
	void *tmp = w;
	size_t tb = scan_bytes((size_t)n + 2);
	HIPCK(rocprim::exclusive_scan(tmp, tb, d->d_fin_per_read, rec_off, 0u, (size_t)n, rocprim::plus<uint32_t>(), st));
	HIPCK(hipMemsetAsync(err, 0, 4, st));
	HIPCK(hipMemsetAsync(len + n, 0, 4, st));
	A.rec_off = rec_off; A.len = len; A.err = err;
	sam_text_count_kernel<<<(n + 255) / 256, 256, 0, st>>>(A);
	tb = scan64_bytes((size_t)n + 2);
	HIPCK(rocprim::exclusive_scan((void *)((uint8_t *)tmp + scan_bytes((size_t)n + 2)), tb, len, d_text_off, (uint64_t)0, (size_t)n + 1, rocprim::plus<uint64_t>(), st));
	uint64_t total = 0; uint32_t h_err = 0;
	HIPCK(hipMemcpyAsync(&total, d_text_off + n, 8, hipMemcpyDeviceToHost, st));
	HIPCK(hipMemcpyAsync(&h_err, err, 4, hipMemcpyDeviceToHost, st));
	HIPCK(hipStreamSynchronize(st));
	HIPCK(hipGetLastError());
	if (h_err & 4u) { bmh_set_error("bmh_sam_text_sizes: a read's group (d_read_group) lies outside the table of n_rg read groups"); return BMH_EINVAL; }
	if (h_err) { bmh_set_error("bmh_sam_text_sizes: a record the text needs has no CIGAR (see bmh_sam_select_device), or one that bmh_cigar_batch flagged"); return BMH_EINVAL; }
	return (int64_t)total;
}

extern "C" int bmh_sam_text_write(const bmh_post_opt_t *popt, const bmh_sam_dev_t *d, const uint64_t *d_text_off, char *d_text, void *d_work, size_t work_bytes, void *stream_)
{
	sam_args_t A;
	const int rc = sam_args(popt, d, "bmh_sam_text_write", A);
	if (rc != BMH_OK) return rc;
	if (d->n_reads == 0) return BMH_OK;
	if (!d_text_off || !d_text || !d_work || work_bytes < bmh_sam_text_work(d->n_reads)) { bmh_set_error("bmh_sam_text_write: null argument, or a work space smaller than bmh_sam_text_work asks for"); return BMH_EINVAL; }
	const uint32_t n = d->n_reads;
	uint8_t *w = (uint8_t *)d_work;
	A.rec_off = (const uint32_t *)w; w += 2 * al256(4 * ((size_t)n + 2));          // (left there by bmh_sam_text_sizes)
	A.err = (uint32_t *)w;
	A.text_off = d_text_off; A.text = d_text;
	sam_text_write_kernel<<<(n + 255) / 256, 256, 0, (hipStream_t)stream_>>>(A);
	HIPCK(hipGetLastError());
	return BMH_OK;
}

// 1 = the write pass met an inconsistency (reads d_work's flag; waits for the stream)
extern "C" int bmh_sam_text_check(const void *d_work, uint32_t n_reads, void *stream_)
{
	const uint8_t *w = (const uint8_t *)d_work + 2 * al256(4 * ((size_t)n_reads + 2));
	uint32_t h = 0;
	HIPCK(hipMemcpyAsync(&h, w, 4, hipMemcpyDeviceToHost, (hipStream_t)stream_));
	HIPCK(hipStreamSynchronize((hipStream_t)stream_));
	if (h) { bmh_set_error("bmh_sam_text_write: internal error (flags %u): the text of a read differs from its counted size", h); return BMH_EINVAL; }
	return BMH_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// The alignments whose fixed slots overflowed (flags 1, 8), without a trip to the host (csrc/align_pipeline.hip): their list, and -- once
// the caller has redone them with large slots -- their records and words put in place behind the packed array.
namespace {

__global__ void __launch_bounds__(256) cigar_over_kernel(const int32_t *aln, uint32_t n, const uint32_t *sel, uint32_t *over, uint32_t *sel2, uint32_t *counter)
{
	const uint32_t k = blockIdx.x * 256u + threadIdx.x;
	if (k >= n) return;
	if (aln[8 * (size_t)k + 7] & 9) { const uint32_t t = atomicAdd(counter, 1u); over[t] = k; sel2[t] = sel ? sel[k] : k; }
}

// the redone alignments take their places: words of each (cigar_patch_words), a scan, then one wave per alignment copies
__global__ void __launch_bounds__(256) cigar_patch_words_kernel(const int32_t *aln2, uint32_t n_over, uint32_t *words)
{
	const uint32_t t = blockIdx.x * 256u + threadIdx.x;
	if (t > n_over) return;
	uint32_t w = 0;
	if (t < n_over) { const int32_t *a = aln2 + 8 * (size_t)t; if (!(a[7] & ~2)) w = (uint32_t)a[3] + (((uint32_t)a[6] + 4u) >> 2); }
	words[t] = w;
}
__global__ void __launch_bounds__(64) cigar_patch_kernel(int32_t *aln, uint32_t *off, uint32_t *packed, const uint32_t *over, uint32_t n_over,
                                                         const int32_t *aln2, const uint32_t *cigar2, int mc2, const char *md2, int mdc2, const uint32_t *start)
{
	const uint32_t t = blockIdx.x, lane = threadIdx.x;
	if (t >= n_over) return;
	const int32_t *a = aln2 + 8 * (size_t)t;
	const uint32_t k = over[t];
	if (lane < 8) aln[8 * (size_t)k + lane] = a[lane];
	if (a[7] & ~2) return;
	if (lane == 0) off[k] = start[t];
	const uint32_t nc = (uint32_t)a[3], nw = ((uint32_t)a[6] + 4u) >> 2;
	uint32_t *o = packed + start[t];
	const uint32_t *cg = cigar2 + (size_t)mc2 * t; const uint32_t *ms = (const uint32_t *)(md2 + (size_t)mdc2 * t);
	for (uint32_t i = lane; i < nc; i += 64) o[i] = cg[i];
	for (uint32_t i = lane; i < nw; i += 64) o[nc + i] = ms[i];
}

}   // namespace

// d_over / d_sel2 [n]: the overflowed alignments and the records they belong to (d_sel: the list bmh_cigar_batch ran on, NULL = identity); d_counter: one
// word of device memory.  Returns their number (waits for the stream).
int64_t bmh_cigar_overflowed(const int32_t *d_aln, uint32_t n, const uint32_t *d_sel, uint32_t *d_over, uint32_t *d_sel2, uint32_t *d_counter, void *stream_)
{
	hipStream_t st = (hipStream_t)stream_;
	if (n == 0) return 0;
	HIPCK(hipMemsetAsync(d_counter, 0, 4, st));
	cigar_over_kernel<<<(n + 255) / 256, 256, 0, st>>>(d_aln, n, d_sel, d_over, d_sel2, d_counter);
	uint32_t h = 0;
	HIPCK(hipMemcpyAsync(&h, d_counter, 4, hipMemcpyDeviceToHost, st));
	HIPCK(hipStreamSynchronize(st));
	HIPCK(hipGetLastError());
	return (int64_t)h;
}

// the redone alignments (d_aln2 / d_cigar2 [n_over][mc2] / d_md2 [n_over][mdc2], in d_over's order) take their places: d_aln[k] is replaced, the words
// are appended behind the `words` packed ones (the caller left room for n_over * (mc2 + mdc2 / 4) more) and d_off[k] points at them; d_work:
// bmh_cigar_patch_work(n_over) bytes.  Returns the new number of words (waits for the stream).
size_t bmh_cigar_patch_work(uint32_t n_over) { return 2 * al256(4 * ((size_t)n_over + 2)) + scan_bytes((size_t)n_over + 2) + 256; }
int64_t bmh_cigar_patch(int32_t *d_aln, uint32_t *d_off, uint32_t *d_packed, uint64_t words, const uint32_t *d_over, uint32_t n_over,
                        const int32_t *d_aln2, const uint32_t *d_cigar2, int mc2, const char *d_md2, int mdc2, void *d_work, size_t work_bytes, void *stream_)
{
	hipStream_t st = (hipStream_t)stream_;
	if (n_over == 0) return (int64_t)words;
	if (!d_work || work_bytes < bmh_cigar_patch_work(n_over)) { bmh_set_error("bmh_cigar_patch: work space too small"); return BMH_EINVAL; }
	uint8_t *w = (uint8_t *)d_work;
	uint32_t *wd = (uint32_t *)w; w += al256(4 * ((size_t)n_over + 2));
	uint32_t *start = (uint32_t *)w; w += al256(4 * ((size_t)n_over + 2));
	cigar_patch_words_kernel<<<(n_over + 1 + 255) / 256, 256, 0, st>>>(d_aln2, n_over, wd);
	size_t tb = scan_bytes((size_t)n_over + 2);
	HIPCK(rocprim::exclusive_scan((void *)w, tb, wd, start, (uint32_t)words, (size_t)n_over + 1, rocprim::plus<uint32_t>(), st));      // start[n_over] = the new total
	cigar_patch_kernel<<<n_over, 64, 0, st>>>(d_aln, d_off, d_packed, d_over, n_over, d_aln2, d_cigar2, mc2, d_md2, mdc2, start);
	uint32_t h = 0;
	HIPCK(hipMemcpyAsync(&h, start + n_over, 4, hipMemcpyDeviceToHost, st));
	HIPCK(hipStreamSynchronize(st));
	HIPCK(hipGetLastError());
	return (int64_t)h;
}
