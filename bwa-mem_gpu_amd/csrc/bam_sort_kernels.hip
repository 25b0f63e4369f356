// BAM records in device memory -> coordinate order, and the index pass over a window of the sorted file (csrc/bam_sort_core.h's rules).
//
//   keys     one lane per record: the 64-bit key through the record's offset, and its ordinal
//   sort     rocprim's radix sort of the (key, ordinal) pairs -- stable, so equal keys keep their order
//   gather   the permuted sizes through an exclusive scan, then 16 lanes per record copy it: the destination is written in aligned 32-bit words (64 bytes per group
//            and step, neighbouring lanes neighbouring words), every word put together from the two aligned source words that hold it (records are unaligned on
//            both sides); the up to three bytes before and behind the words go one byte per lane.  The same loop takes a record of any size.
//   index    one lane per record of a window whose members' sizes are known: the record's virtual offset, whether it begins a chunk, a 64-bit atomicMin on every
//            16 KiB window it overlaps that the record before it does not (that one lies earlier in the file, so it has the smaller offset), and the counts --
//            one atomicAdd per block where the block's records share a reference, which in a sorted file nearly every block does.  A scan and a second kernel
//            compact the chunk heads.  For a CSI index (bsr_index_marks<true>, bsr_index_heads<true>) the windows hold 2^min_shift bases and the heads are
//            keyed on the CSI bin of the record's windows.
//
// The final merge of the runs (bsr_merge_device) sorts all runs' keys once more and builds the file window by window: the host reads each run's share of the window
// (stability makes it one contiguous range of the run) into a pinned buffer, the device gathers, compresses and indexes it.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <rocprim/rocprim.hpp>
#include <stdio.h>
#include <algorithm>
#include <chrono>
#include <vector>
#include "bam_sort.h"
#include "bam_dup.h"
#include "bam_cov.h"
#include "bam_stats.h"
#include "bam_ws.h"

struct bsr_dev_t {
	dev_buf<uint8_t> keys, keys2, ord, ord2, tmp, src_off, size, soff, sorted, in, in_off;      // sort and gather
	hipEvent_t ev_flag[2] = {nullptr, nullptr};                                          // around a window's flag step (duplicate marking)
	dev_buf<uint8_t> side;                                                                      // a word per record, permuted with a batch's records (duplicate marking)
	dev_buf<uint8_t> head, hpos, heads, lin, counts, n_win, lin_off;                            // the index pass; lin, counts: of the whole file
	uint8_t *h_buf = nullptr; size_t h_cap = 0;                                          // pinned: a window's records on their way up, its members on their way down
	int n_ref = 0, ix_format = BSR_IX_BAI, ix_shift = BSR_LIN_SHIFT, ix_depth = BSR_BAI_DEPTH;   // of the index being built (bsr_index_begin)
	int pinned(size_t n)
	{
		if (n <= h_cap) return BMH_OK;
		if (h_buf) (void)hipHostFree(h_buf);
		h_buf = nullptr; h_cap = 0;
		const size_t c = n + n / 4 + 4096;
		if (hipHostMalloc((void **)&h_buf, c, hipHostMallocDefault) != hipSuccess) { bmh_set_error("sorted BAM: %zu bytes of pinned memory: %s", c, hipGetErrorString(hipGetLastError())); return BMH_ENOMEM; }
		h_cap = c;
		return BMH_OK;
	}
	~bsr_dev_t() { if (h_buf) (void)hipHostFree(h_buf); for (hipEvent_t e : ev_flag) if (e) (void)hipEventDestroy(e); }
};

namespace {

constexpr int G = 16;              // lanes per record of the gather

double bsr_now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

__global__ void __launch_bounds__(256) bsr_keys(const uint8_t *__restrict__ recs, const uint64_t *__restrict__ off, uint32_t n, uint64_t total, uint64_t *__restrict__ keys, uint32_t *__restrict__ ord)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const uint64_t o = off[i];
	keys[i] = o <= total && total - o >= BSR_FIXED ? bsr_key(recs + o) : ~0ull;
	ord[i] = i;
}

__global__ void __launch_bounds__(256) bsr_iota(uint32_t *__restrict__ ord, uint64_t n)
{
	const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (i < n) ord[i] = (uint32_t)i;
}

__global__ void __launch_bounds__(256) bsr_perm(const uint64_t *__restrict__ off, const uint32_t *__restrict__ ord, uint32_t n, uint64_t *__restrict__ src_off, uint32_t *__restrict__ size,
                                                const uint32_t *__restrict__ side, uint32_t *__restrict__ side_out)
{
	const uint32_t j = blockIdx.x * 256 + threadIdx.x;
	if (j >= n) return;
	const uint32_t i = ord[j] < n ? ord[j] : 0;
	src_off[j] = off[i]; size[j] = (uint32_t)(off[i + 1] - off[i]);
	if (side) side_out[j] = side[i];
}

// src and dst are 4-byte aligned buffers with at least 4 bytes of room behind src_bytes / dst_bytes (the last source word of a record may lie partly behind it)
__global__ void __launch_bounds__(256) bsr_gather(const uint8_t *__restrict__ src, uint64_t src_bytes, const uint64_t *__restrict__ src_off, const uint32_t *__restrict__ size,
                                                  const uint64_t *__restrict__ dst_off, uint8_t *__restrict__ dst, uint64_t dst_bytes, uint32_t n)
{
	const uint32_t j = blockIdx.x * (256 / G) + threadIdx.x / G, l = threadIdx.x % G;
	if (j >= n) return;
	const uint64_t so = src_off[j], d0 = dst_off[j];
	const uint32_t sz = size[j];
	if (so > src_bytes || sz > src_bytes - so || d0 > dst_bytes || sz > dst_bytes - d0) return;
	const uint8_t *s = src + so; uint8_t *d = dst + d0;
	uint32_t head = (uint32_t)((4 - (d0 & 3)) & 3);
	if (head > sz) head = sz;
	if (l < head) d[l] = s[l];
	const uint32_t nw = (sz - head) / 4;
	const uint64_t sa = so + head;
	const uint32_t sh = (uint32_t)(sa & 3) * 8;
	const uint32_t *sw = (const uint32_t *)(src + (sa & ~3ull)); uint32_t *dw = (uint32_t *)(d + head);
	if (sh == 0) for (uint32_t w = l; w < nw; w += G) dw[w] = sw[w];
	else for (uint32_t w = l; w < nw; w += G) dw[w] = sw[w] >> sh | sw[w + 1] << (32 - sh);
	const uint32_t t = head + nw * 4 + l;
	if (t < sz) d[t] = s[t];
}

// CSI: the windows hold 2^min_shift bases and a chunk begins where (refID, CSI bin) change -- the bin of the record's first and last window, which the lane has
// anyway, and of the windows of the record before it, which it has wherever the two share a reference; the record's bin field is not read.  The BAI form reads
// neither min_shift nor depth
template <bool CSI>
__global__ void __launch_bounds__(256) bsr_index_marks(const uint8_t *__restrict__ recs, const uint64_t *__restrict__ soff, uint32_t n, const uint64_t *__restrict__ moff, uint64_t base, int n_ref,
                                                       const uint32_t *__restrict__ n_win, const uint64_t *__restrict__ lin_off, unsigned long long *lin, unsigned long long *counts, uint32_t *__restrict__ head,
                                                       int min_shift, int depth)
{
	__shared__ int r0;
	const uint32_t j = blockIdx.x * 256 + threadIdx.x;
	const bool valid = j < n;
	int32_t r = -1; uint32_t slot = 2 * (uint32_t)n_ref;
	if (valid) {
		const uint8_t *rec = recs + soff[j], *prev = j ? recs + soff[j - 1] : nullptr;
		if (!CSI) head[j] = bsr_chunk_head(rec, prev) ? 1u : 0u;
		r = bsr_ref(rec);
		if (r >= 0 && r < n_ref) {
			slot = 2 * (uint32_t)r + ((bsr_flag(rec) & 4u) ? 1u : 0u);
			const uint64_t v = bsr_voff(base, moff, soff[n], soff[j]);
			uint32_t lo, hi, plo = 1, phi = 0;
			const bool same = prev && bsr_ref(prev) == r;
			if (CSI) { bsr_windows_at(rec, n_win[r], min_shift, &lo, &hi); if (same) bsr_windows_at(prev, n_win[r], min_shift, &plo, &phi); }
			else { bsr_windows(rec, n_win[r], &lo, &hi); if (same) bsr_windows(prev, n_win[r], &plo, &phi); }
			if (CSI) head[j] = !same || bsr_csi_bin(lo, hi, depth) != bsr_csi_bin(plo, phi, depth) ? 1u : 0u;
			for (uint32_t w = lo; w <= hi; ++w) if (w < plo || w > phi) atomicMin(lin + lin_off[r] + w, (unsigned long long)v);
		} else {
			if (CSI) head[j] = bsr_csi_chunk_head(rec, prev, 1u, min_shift, depth) ? 1u : 0u;      // (no reference: a head behind a record that has one)
			r = -1;
		}
	}
	if (threadIdx.x == 0) r0 = r;                           // (lane 0 of a launched block always has a record)
	__syncthreads();
	const int ref0 = r0;
	if (__syncthreads_and(!valid || r == ref0)) {
		const uint32_t s0 = ref0 < 0 ? 2 * (uint32_t)n_ref : 2 * (uint32_t)ref0;
		const int c0 = __syncthreads_count(valid && slot == s0), c1 = __syncthreads_count(valid && slot == s0 + 1 && ref0 >= 0);
		if (threadIdx.x == 0) { if (c0) atomicAdd(counts + s0, (unsigned long long)c0); if (c1) atomicAdd(counts + s0 + 1, (unsigned long long)c1); }
	} else if (valid) atomicAdd(counts + slot, 1ull);
}

template <bool CSI>
__global__ void __launch_bounds__(256) bsr_index_heads(const uint8_t *__restrict__ recs, const uint64_t *__restrict__ soff, uint32_t n, const uint64_t *__restrict__ moff, uint64_t base, int n_ref,
                                                       const uint32_t *__restrict__ head, const uint32_t *__restrict__ hpos, bsr_head_t *__restrict__ out,
                                                       const uint32_t *__restrict__ n_win, int min_shift, int depth)
{
	const uint32_t j = blockIdx.x * 256 + threadIdx.x;
	if (j >= n || !head[j] || hpos[j] >= n) return;
	const uint8_t *rec = recs + soff[j];
	const int32_t r = bsr_ref(rec);
	bsr_head_t h; h.ref = r >= 0 && r < n_ref ? r : -1;
	h.bin = CSI ? bsr_csi_rec_bin(rec, h.ref >= 0 ? n_win[r] : 1u, min_shift, depth) : bsr_bin(rec);
	h.beg = bsr_voff(base, moff, soff[n], soff[j]);
	out[hpos[j]] = h;
}

// size [n] on the device -> soff [n + 1], then the n records src + src_off[j] into d->sorted at soff[j]
int scan_and_gather(bsr_dev_t *d, const uint8_t *d_src, uint64_t src_bytes, uint32_t n, uint64_t total, hipStream_t st)
{
	size_t tb = scan_tmp_bytes<uint32_t, uint64_t>((size_t)n + 1);
	RCK(d->tmp.need(tb)); RCK(d->soff.need(8 * ((size_t)n + 2))); RCK(d->sorted.need((size_t)total + 16));
	HIPCK(hipMemsetAsync((uint32_t *)d->size.p + n, 0, 4, st));
	HIPCK(rocprim::exclusive_scan(d->tmp.p, tb, (uint32_t *)d->size.p, (uint64_t *)d->soff.p, (uint64_t)0, (size_t)n + 1, rocprim::plus<uint64_t>(), st));
	if (n) bsr_gather<<<(n + 256 / G - 1) / (256 / G), 256, 0, st>>>(d_src, src_bytes, (const uint64_t *)d->src_off.p, (const uint32_t *)d->size.p, (const uint64_t *)d->soff.p, (uint8_t *)d->sorted.p, total, n);
	HIPCK(hipGetLastError());
	return BMH_OK;
}

}   // namespace

bsr_dev_t *bsr_dev_create(void) { return new bsr_dev_t(); }
void bsr_dev_free(bsr_dev_t *d) { delete d; }

int bsr_sort_run_device(bsr_dev_t *d, const uint8_t *d_recs, const uint64_t *d_off, uint32_t n, uint64_t total, void *stream, const uint8_t **d_sorted, const uint64_t **d_keys, const uint64_t **d_soff,
                        const uint32_t *d_side, const uint32_t **d_side_sorted)
{
	hipStream_t st = (hipStream_t)stream;
	size_t sb = sort_pairs_tmp_bytes<uint64_t, uint32_t>(n);
	RCK(d->keys.need(8 * ((size_t)n + 1))); RCK(d->keys2.need(8 * ((size_t)n + 1))); RCK(d->ord.need(4 * ((size_t)n + 1))); RCK(d->ord2.need(4 * ((size_t)n + 1)));
	RCK(d->src_off.need(8 * ((size_t)n + 1))); RCK(d->size.need(4 * ((size_t)n + 2))); RCK(d->tmp.need(sb));
	if (d_side) RCK(d->side.need(4 * ((size_t)n + 1)));
	if (n) {
		bsr_keys<<<(n + 255) / 256, 256, 0, st>>>(d_recs, d_off, n, total, (uint64_t *)d->keys.p, (uint32_t *)d->ord.p);
		HIPCK(rocprim::radix_sort_pairs(d->tmp.p, sb, (uint64_t *)d->keys.p, (uint64_t *)d->keys2.p, (uint32_t *)d->ord.p, (uint32_t *)d->ord2.p, (size_t)n, 0, 64, st));
		bsr_perm<<<(n + 255) / 256, 256, 0, st>>>(d_off, (const uint32_t *)d->ord2.p, n, (uint64_t *)d->src_off.p, (uint32_t *)d->size.p, d_side, d_side ? (uint32_t *)d->side.p : nullptr);
	}
	RCK(scan_and_gather(d, d_recs, total, n, total, st));
	*d_sorted = (const uint8_t *)d->sorted.p; *d_keys = (const uint64_t *)d->keys2.p; *d_soff = (const uint64_t *)d->soff.p;
	if (d_side_sorted) *d_side_sorted = d_side ? (const uint32_t *)d->side.p : nullptr;
	return BMH_OK;
}

int bsr_sort_keys_device(bsr_dev_t *d, const uint64_t *keys, uint64_t n, void *stream, uint32_t *ord)
{
	hipStream_t st = (hipStream_t)stream;
	if (n == 0) return BMH_OK;
	if (n > 0xfffffff0ull) { bmh_set_error("sorted BAM: %llu records: the final sort takes fewer than 2^32", (unsigned long long)n); return BMH_EINVAL; }
	size_t sb = sort_pairs_tmp_bytes<uint64_t, uint32_t>((size_t)n);
	// keys and ordinals, in and out, and the sort's work space must fit the device: 24 bytes per record and the work space
	size_t fr = 0, tot = 0;
	HIPCK(hipMemGetInfo(&fr, &tot));
	// (a buffer that has to grow is freed and allocated anew a quarter larger than asked: that is what is counted; one that is large enough costs nothing)
	dev_buf<uint8_t> *const buf[5] = {&d->keys, &d->keys2, &d->ord, &d->ord2, &d->tmp};
	const size_t ask[5] = {8 * (size_t)n, 8 * (size_t)n, 4 * (size_t)n, 4 * (size_t)n, sb};
	size_t have = 0, want = 64u << 20;
	for (int k = 0; k < 5; ++k) if (ask[k] > buf[k]->cap) { have += buf[k]->cap; want += ask[k] + ask[k] / 4 + 1024; }
	if (want > fr + have) {
		bmh_set_error("sorted BAM: the final sort of %llu records needs %zu bytes of device memory, %zu are free (sort fewer reads per run, or on a device with more memory)", (unsigned long long)n, want, fr + have);
		return BMH_ENOMEM;
	}
	for (int k = 0; k < 5; ++k)
		if (buf[k]->need(ask[k]) != BMH_OK) {                  // (fragmentation, or another process took the memory in between)
			bmh_set_error("sorted BAM: the final sort of %llu records: no %zu bytes of device memory for its keys and work space", (unsigned long long)n, ask[k] + ask[k] / 4 + 1024);
			return BMH_ENOMEM;
		}
	HIPCK(hipMemcpyAsync(d->keys.p, keys, 8 * (size_t)n, hipMemcpyHostToDevice, st));
	bsr_iota<<<(unsigned)((n + 255) / 256), 256, 0, st>>>((uint32_t *)d->ord.p, n);
	HIPCK(rocprim::radix_sort_pairs(d->tmp.p, sb, (uint64_t *)d->keys.p, (uint64_t *)d->keys2.p, (uint32_t *)d->ord.p, (uint32_t *)d->ord2.p, (size_t)n, 0, 64, st));
	HIPCK(hipMemcpyAsync(ord, d->ord2.p, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
	HIPCK(hipStreamSynchronize(st));
	return BMH_OK;
}

int bsr_index_begin(bsr_dev_t *d, const bsr_index_t &ix, void *stream)
{
	hipStream_t st = (hipStream_t)stream;
	d->n_ref = ix.n_ref; d->ix_format = ix.format; d->ix_shift = ix.min_shift; d->ix_depth = ix.depth;
	if (8 * ix.lin.size() > d->lin.cap) {                   // the lin array grows with the contigs and shrinks with min_shift (16 MB for 2^31 bases at 10): counted before it is allocated
		size_t fr = 0, tot = 0;
		HIPCK(hipMemGetInfo(&fr, &tot));
		const size_t want = 8 * ix.lin.size() + 2 * ix.lin.size() + 1024 + (64u << 20);
		if (want > fr + d->lin.cap) {
			bmh_set_error("sorted BAM: the index's %zu windows of 2^%d bases need %zu bytes of device memory, %zu are free (choose a larger min_shift)", ix.lin.size(), ix.min_shift, want, fr + d->lin.cap);
			return BMH_ENOMEM;
		}
	}
	RCK(d->lin.need(8 * ix.lin.size())); RCK(d->counts.need(8 * ix.counts.size())); RCK(d->n_win.need(4 * ((size_t)ix.n_ref + 1))); RCK(d->lin_off.need(8 * ix.lin_off.size()));
	HIPCK(hipMemsetAsync(d->lin.p, 0xff, 8 * ix.lin.size(), st));
	HIPCK(hipMemsetAsync(d->counts.p, 0, 8 * ix.counts.size(), st));
	if (ix.n_ref) HIPCK(hipMemcpyAsync(d->n_win.p, ix.n_win.data(), 4 * (size_t)ix.n_ref, hipMemcpyHostToDevice, st));
	HIPCK(hipMemcpyAsync(d->lin_off.p, ix.lin_off.data(), 8 * ix.lin_off.size(), hipMemcpyHostToDevice, st));
	HIPCK(hipStreamSynchronize(st));
	return BMH_OK;
}

int bsr_index_finish(bsr_dev_t *d, bsr_index_t &ix, void *stream)
{
	hipStream_t st = (hipStream_t)stream;
	HIPCK(hipMemcpyAsync(ix.lin.data(), d->lin.p, 8 * ix.lin.size(), hipMemcpyDeviceToHost, st));
	HIPCK(hipMemcpyAsync(ix.counts.data(), d->counts.p, 8 * ix.counts.size(), hipMemcpyDeviceToHost, st));
	HIPCK(hipStreamSynchronize(st));
	return BMH_OK;
}

int bsr_window_device(bsr_dev_t *d, bmh_bam_ws_t *ws, const uint8_t *src, uint64_t src_bytes, const uint64_t *src_off, const uint32_t *size, uint32_t n, int level,
                      void *stream, bsr_index_t &ix, bsr_sink_t sink, void *user, bdp_dev_t *dup, const uint32_t *tord, double *flag_ms, bcv_dev_t *cov, double *cov_ms,
                      bst_dev_t *stats, double *stats_ms, brc_dev_t *recal, double *recal_ms, brq_dev_t *requal, double *requal_ms)
{
	hipStream_t st = (hipStream_t)stream;
	if (n == 0) return BMH_OK;
	uint64_t total = 0;
	for (uint32_t j = 0; j < n; ++j) {
		if (src_off[j] > src_bytes || size[j] > src_bytes - src_off[j] || size[j] < BSR_FIXED) { bmh_set_error("sorted BAM: internal error: record %u of a window lies outside its run", j); return BMH_EINVAL; }
		total += size[j];
	}
	RCK(d->in.need((size_t)src_bytes + 16)); RCK(d->src_off.need(8 * ((size_t)n + 1))); RCK(d->size.need(4 * ((size_t)n + 2)));
	HIPCK(hipMemcpyAsync(d->in.p, src, (size_t)src_bytes, hipMemcpyHostToDevice, st));
	HIPCK(hipMemcpyAsync(d->src_off.p, src_off, 8 * (size_t)n, hipMemcpyHostToDevice, st));
	HIPCK(hipMemcpyAsync(d->size.p, size, 4 * (size_t)n, hipMemcpyHostToDevice, st));
	RCK(scan_and_gather(d, (const uint8_t *)d->in.p, src_bytes, n, total, st));
	if (dup) {                                                  // (sort key, bin and index do not read 0x400)
		if (flag_ms) { for (hipEvent_t &e : d->ev_flag) if (!e) HIPCK(hipEventCreate(&e)); HIPCK(hipEventRecord(d->ev_flag[0], st)); }
		RCK(bdp_flag_device(dup, (uint8_t *)d->sorted.p, (const uint64_t *)d->soff.p, tord, n, total, st));
		if (flag_ms) HIPCK(hipEventRecord(d->ev_flag[1], st));
	}
	// the table applied to the qualities: one kernel that rewrites the window in place; every step below reads the qualities as written
	if (requal) RCK(brq_window_device(requal, (uint8_t *)d->sorted.p, (const uint64_t *)d->soff.p, n, st, requal_ms));
	// coverage reads the records in their final order with their final flags; the window's last record (host) sets its frontier
	if (cov) RCK(bcv_window_device(cov, (const uint8_t *)d->sorted.p, (const uint64_t *)d->soff.p, n, src + src_off[n - 1], st, "sorted BAM", cov_ms));
	// the statistics read the same records: one kernel, nothing waits for it here
	if (stats) RCK(bst_window_device(stats, (const uint8_t *)d->sorted.p, (const uint64_t *)d->soff.p, n, st, stats_ms));
	// the recalibration table reads them too, and the reference: one kernel, nothing waits for it here
	if (recal) RCK(brc_window_device(recal, (const uint8_t *)d->sorted.p, (const uint64_t *)d->soff.p, n, st, recal_ms));
	const uint8_t *d_members = nullptr; uint64_t mb = 0;
	RCK(bmh_bgzf_deflate_device(ws, (const uint8_t *)d->sorted.p, total, level, st, &d_members, &mb));
	// the index pass: the members' offsets are the compressor's scan (ws->moff [n_members + 1])
	size_t tb = scan_tmp_bytes<uint32_t, uint32_t>((size_t)n + 1);
	RCK(d->head.need(4 * ((size_t)n + 2))); RCK(d->hpos.need(4 * ((size_t)n + 2))); RCK(d->heads.need(sizeof(bsr_head_t) * ((size_t)n + 1))); RCK(d->tmp.need(tb));
	HIPCK(hipMemsetAsync((uint32_t *)d->head.p + n, 0, 4, st));
	const bool csi = d->ix_format == BSR_IX_CSI;
	(csi ? bsr_index_marks<true> : bsr_index_marks<false>)<<<(n + 255) / 256, 256, 0, st>>>((const uint8_t *)d->sorted.p, (const uint64_t *)d->soff.p, n, (const uint64_t *)ws->moff.p, ix.file_pos, d->n_ref,
	                                                 (const uint32_t *)d->n_win.p, (const uint64_t *)d->lin_off.p, (unsigned long long *)d->lin.p, (unsigned long long *)d->counts.p, (uint32_t *)d->head.p,
	                                                 d->ix_shift, d->ix_depth);
	HIPCK(rocprim::exclusive_scan(d->tmp.p, tb, (uint32_t *)d->head.p, (uint32_t *)d->hpos.p, 0u, (size_t)n + 1, rocprim::plus<uint32_t>(), st));
	(csi ? bsr_index_heads<true> : bsr_index_heads<false>)<<<(n + 255) / 256, 256, 0, st>>>((const uint8_t *)d->sorted.p, (const uint64_t *)d->soff.p, n, (const uint64_t *)ws->moff.p, ix.file_pos, d->n_ref,
	                                                 (const uint32_t *)d->head.p, (const uint32_t *)d->hpos.p, (bsr_head_t *)d->heads.p, (const uint32_t *)d->n_win.p, d->ix_shift, d->ix_depth);
	uint32_t nh = 0;
	HIPCK(hipMemcpyAsync(&nh, (const uint32_t *)d->hpos.p + n, 4, hipMemcpyDeviceToHost, st));
	RCK(d->pinned((size_t)mb + 16));
	HIPCK(hipMemcpyAsync(d->h_buf, d_members, (size_t)mb, hipMemcpyDeviceToHost, st));
	HIPCK(hipStreamSynchronize(st));
	HIPCK(hipGetLastError());
	if (dup && flag_ms) { float ms = 0; HIPCK(hipEventElapsedTime(&ms, d->ev_flag[0], d->ev_flag[1])); *flag_ms += ms; }
	if (cov && cov_ms) RCK(bcv_window_ms(cov, cov_ms));
	if (stats) RCK(bst_window_ms(stats, stats_ms, "sorted BAM"));        // (a refused record ends the run before the window's members reach the sink)
	if (recal) RCK(brc_window_ms(recal, recal_ms, "sorted BAM"));
	if (requal) RCK(brq_window_ms(requal, requal_ms, "sorted BAM"));
	if (nh == 0 || nh > n) { bmh_set_error("sorted BAM: internal error: %u chunk heads among %u records", nh, n); return BMH_EINVAL; }
	const size_t h0 = ix.heads.size();
	ix.heads.resize(h0 + nh);
	HIPCK(hipMemcpy(ix.heads.data() + h0, d->heads.p, sizeof(bsr_head_t) * (size_t)nh, hipMemcpyDeviceToHost));
	ix.file_pos += mb;
	if (sink(user, (const char *)d->h_buf, (size_t)mb) != 0) { bmh_set_error("the sink refused the text"); return BMH_EINVAL; }
	return BMH_OK;
}

// every run of the store -> the sorted file's record members (to the sink) and its index
int bsr_merge_device(bsr_dev_t *d, bmh_bam_ws_t *ws, const bsr_store_t &S, bsr_out_t &J, void *stream, bsr_sink_t sink, void *user, bcv_dev_t *cov, bst_dev_t *stats, brc_dev_t *recal, brq_dev_t *requal)
{
	const bdp_plan_t &P = J.P; bsr_index_t &ix = J.ix; const int level = J.level; const uint32_t window = J.window;
	uint64_t *const dup_counts = J.markdup ? J.dup_counts : nullptr;
	double *const cov_ms = J.timed && cov ? J.cov_ms : nullptr, *const stats_ms = J.timed && stats ? J.stats_ms : nullptr, *const recal_ms = J.timed && recal ? J.recal_ms : nullptr,
	       *const requal_ms = J.timed && requal ? J.requal_ms : nullptr;
	const bdp_optical_t *optical = P.optical(); const bool barcode = P.barcode() != nullptr;
	uint64_t n = 0, bytes = 0;
	std::vector<uint64_t> first;
	for (const bsr_run_t &r : S.runs) { first.push_back(n); n += r.n; bytes += r.bytes; }
	RCK(bsr_index_begin(d, ix, stream));
	// duplicate marking: the decision over every template's entry comes first (its work space is freed before the final sort takes its own); the bitmap stays
	struct dup_own_t { bdp_dev_t *p = nullptr; ~dup_own_t() { if (p) bdp_dev_free(p); } } dup;
	std::vector<uint32_t> tord; double decide_ms = 0, flag_ms = 0, o_ms = 0;
	if (dup_counts) {
		for (int k = 0; k < BDP_N_COUNTS; ++k) dup_counts[k] = 0;
		for (const bsr_run_t &r : S.runs) if (r.tpl.size() != r.n) { bmh_set_error("sorted BAM: internal error: a run without its records' template ordinals"); return BMH_EINVAL; }
		if (!(dup.p = bdp_dev_create())) return BMH_ENOMEM;
		const double t0 = bsr_now_ms();
		if (optical && S.locs.size() != S.entries.size()) { bmh_set_error("sorted BAM: internal error: %zu locations for %zu templates", S.locs.size(), S.entries.size()); return BMH_EINVAL; }
		if (barcode && S.bcs.size() != S.entries.size()) { bmh_set_error("sorted BAM: internal error: %zu barcode words for %zu templates", S.bcs.size(), S.entries.size()); return BMH_EINVAL; }
		RCK(bdp_decide_device(dup.p, S.entries.data(), S.locs.data(), barcode ? S.bcs.data() : nullptr, S.entries.size(), stream, dup_counts, P, n, &o_ms));
		dup_counts[BDP_SECSUP] = S.dup_info[0]; dup_counts[BDP_UNMAPPED] = S.dup_info[1]; dup_counts[BDP_TEMPLATES] = S.entries.size();
		decide_ms = bsr_now_ms() - t0;
	}
	if (n) {
		std::vector<uint64_t> keys; keys.reserve((size_t)n);
		for (const bsr_run_t &r : S.runs) keys.insert(keys.end(), r.keys.begin(), r.keys.end());
		std::vector<uint32_t> ord((size_t)n);
		RCK(bsr_sort_keys_device(d, keys.data(), n, stream, ord.data()));
		std::vector<uint64_t>().swap(keys);
		const uint64_t W = window ? window : std::max<uint64_t>(1, (64ull << 20) / std::max<uint64_t>(1, bytes / n));
		const size_t nr = S.runs.size();
		std::vector<uint64_t> lo(nr), hi(nr), place(nr), src_off; std::vector<uint32_t> run_of, size;
		for (uint64_t a = 0; a < n; a += W) {
			const uint64_t b = std::min(n, a + W); const uint32_t m = (uint32_t)(b - a);
			std::fill(lo.begin(), lo.end(), ~0ull); std::fill(hi.begin(), hi.end(), 0);
			run_of.resize(m); src_off.resize(m); size.resize(m); if (dup.p) tord.resize(m);
			for (uint32_t j = 0; j < m; ++j) {
				const uint64_t g = ord[(size_t)(a + j)];
				const size_t r = (size_t)(std::upper_bound(first.begin(), first.end(), g) - first.begin()) - 1;
				const uint64_t i = g - first[r];
				run_of[j] = (uint32_t)r; lo[r] = std::min(lo[r], i); hi[r] = std::max(hi[r], i + 1);
			}
			uint64_t sb = 0, cnt = 0;
			for (size_t r = 0; r < nr; ++r) if (hi[r]) { place[r] = sb; sb += S.runs[r].off[hi[r]] - S.runs[r].off[lo[r]]; cnt += hi[r] - lo[r]; }
			if (cnt != m) { bmh_set_error("sorted BAM: internal error: a window's share of a run is not one range (%llu records for %u places)", (unsigned long long)cnt, m); return BMH_EINVAL; }
			RCK(d->pinned((size_t)sb + 16));
			for (size_t r = 0; r < nr; ++r) if (hi[r]) RCK(S.read(S.runs[r], S.runs[r].off[lo[r]], S.runs[r].off[hi[r]], d->h_buf + place[r]));
			for (uint32_t j = 0; j < m; ++j) {
				const bsr_run_t &R = S.runs[run_of[j]];
				const uint64_t i = ord[(size_t)(a + j)] - first[run_of[j]];
				src_off[j] = place[run_of[j]] + (R.off[i] - R.off[lo[run_of[j]]]); size[j] = (uint32_t)(R.off[i + 1] - R.off[i]);
				if (dup.p) tord[j] = (uint32_t)(R.tbase + R.tpl[i]);
			}
			// (the pinned buffer takes the members once the records are on the device: the compressor waits for the stream in between)
			RCK(bsr_window_device(d, ws, d->h_buf, sb, src_off.data(), size.data(), m, level, stream, ix, sink, user, dup.p, dup.p ? tord.data() : nullptr, dup.p ? &flag_ms : nullptr, cov, cov_ms, stats, stats_ms, recal, recal_ms, requal, requal_ms));
		}
	}
	if (dup_counts) {
		if (J.timed) { J.dup_ms[0] += decide_ms; J.dup_ms[1] += flag_ms; }
		if (getenv("BMH_ALIGNER_TRACE"))
			fprintf(stderr, "[aligner] duplicate marking: %zu templates (%zu bytes of entries, %llu of ordinals kept) decided in %.2f ms, the windows' flags set in %.2f ms\n", S.entries.size(),
			        sizeof(bdp_entry_t) * S.entries.size(), 4ull * (unsigned long long)n, decide_ms, flag_ms);
		if (J.timed) J.opt_ms += o_ms;
		if (optical && getenv("BMH_ALIGNER_TRACE"))
			fprintf(stderr, "[aligner] optical duplicates: %zu bytes of locations, %llu optical pairs among %llu located ones (%llu sets skipped) counted in %.1f of the decision's ms\n",
			        sizeof(bdp_loc_t) * S.locs.size(), (unsigned long long)optical->out[BDP_OPT_DUPS], (unsigned long long)optical->out[BDP_OPT_LOCATED], (unsigned long long)optical->out[BDP_OPT_SKIPPED], o_ms);
	}
	return bsr_index_finish(d, ix, stream);
}

int bsr_write_device(bsr_dev_t *d, bmh_bam_ws_t *ws, const bsr_store_t &S, bsr_out_t &J, void *stream, bsr_sink_t sink, void *user, const char *fn)
{
	struct cov_own_t { bcv_dev_t *p = nullptr; ~cov_own_t() { if (p) bcv_dev_free(p); } } cov;            // the run's device state, from the first window to the results
	struct stats_own_t { bst_dev_t *p = nullptr; ~stats_own_t() { if (p) bst_dev_free(p); } } stats;
	if (J.markdup && J.P.no_barcode) *J.P.no_barcode = J.P.barcode() ? bdp_no_barcode(S.bcs.data(), S.bcs.size()) : 0;
	if (J.coverage) {
		if (!(cov.p = bcv_dev_create())) return BMH_ENOMEM;
		RCK(bcv_begin_device(cov.p, J.CP, stream));
	}
	if (J.stats) {
		if (!(stats.p = bst_dev_create())) return BMH_ENOMEM;
		RCK(bst_begin_device(stats.p, J.SP, stream));
	}
	struct recal_own_t { brc_dev_t *p = nullptr; ~recal_own_t() { if (p) brc_dev_free(p); } } recal;
	if (J.recal) {
		if (!J.recal_d_pac && !J.RU.pac && J.RU.l_pac) { bmh_set_error("%s: the recalibration table needs the reference (pac, l_pac)", fn); return BMH_EINVAL; }
		if (!(recal.p = brc_dev_create())) return BMH_ENOMEM;
		RCK(brc_begin_device(recal.p, J.RU, J.recal_d_pac, stream));
	}
	struct requal_own_t { brq_dev_t *p = nullptr; ~requal_own_t() { if (p) brq_dev_free(p); } } requal;
	if (J.requal) {
		if (!(requal.p = brq_dev_create())) return BMH_ENOMEM;
		RCK(brq_begin_device(requal.p, J.QU, stream));
	}
	RCK(bsr_merge_device(d, ws, S, J, stream, sink, user, cov.p, stats.p, recal.p, requal.p));
	if (requal.p) RCK(brq_finish_device(requal.p, stream, J.QR, fn));
	if (recal.p) RCK(brc_finish_device(recal.p, stream, J.RR, fn));
	if (stats.p) RCK(bst_finish_device(stats.p, stream, J.SR, fn));
	if (cov.p) RCK(bcv_finish_device(cov.p, stream, J.CR, fn, J.timed ? J.cov_ms : nullptr));
	if (J.markdup && J.P.groups() && J.P.lib_counts)                   // every library's line counts and templates, as the batches counted them
		for (size_t k = 0; k < S.lib_info.size() && k / 3 < J.P.n_lib(); ++k) J.P.lib_counts[BDP_N_COUNTS * (k / 3) + BDP_SECSUP + k % 3] = S.lib_info[k];
	return BMH_OK;
}

// ---------------------------------------------------------------------------------------------------------------- the stand-alone entry points

namespace {
// what duplicate marking keeps of a stream: its records' template ordinals in sorted order, the templates' entries, the line counts
struct dup_host_t { std::vector<uint32_t> tpl; std::vector<bdp_entry_t> entries; uint64_t secsup = 0, unmapped = 0; std::vector<uint64_t> bcs; };
int to_store(bsr_dev_t *d, const uint8_t *recs, uint64_t n_bytes, const std::vector<uint64_t> &off, hipStream_t st, std::vector<uint8_t> &sorted, std::vector<uint64_t> &keys, std::vector<uint64_t> &soff,
             dup_host_t *dh, const char *fn, const bdp_plan_t &P)
{
	const bdp_table_t *G = P.groups(); const bdp_bc_t *bc = P.barcode();
	const uint32_t n = (uint32_t)(off.size() - 1);
	RCK(d->in.need((size_t)n_bytes + 16)); RCK(d->in_off.need(8 * off.size()));
	HIPCK(hipMemcpyAsync(d->in.p, recs, (size_t)n_bytes, hipMemcpyHostToDevice, st));
	HIPCK(hipMemcpyAsync(d->in_off.p, off.data(), 8 * off.size(), hipMemcpyHostToDevice, st));
	const uint8_t *ds; const uint64_t *dk, *dso;
	struct dup_own_t { bdp_dev_t *p = nullptr; ~dup_own_t() { if (p) bdp_dev_free(p); } } dup;
	const uint32_t *d_tpl = nullptr, *d_info = nullptr, *d_tpl_sorted = nullptr; const bdp_entry_t *d_e = nullptr; const uint64_t *d_b = nullptr;
	if (dh) {
		if (!(dup.p = bdp_dev_create())) return BMH_ENOMEM;
		RCK(bdp_dev_set_groups(dup.p, G, st));
		RCK(bdp_batch_device(dup.p, (const uint8_t *)d->in.p, (const uint64_t *)d->in_off.p, n, n_bytes, st, &d_tpl, &d_e, &d_info, nullptr, bc, bc ? &d_b : nullptr));
	}
	RCK(bsr_sort_run_device(d, (const uint8_t *)d->in.p, (const uint64_t *)d->in_off.p, n, n_bytes, st, &ds, &dk, &dso, d_tpl, &d_tpl_sorted));
	if (dh) {
		uint32_t info[BDP_INFO_WORDS_PACK];
		HIPCK(hipMemcpyAsync(info, d_info, 4 * bdp_info_words(bc), hipMemcpyDeviceToHost, st));
		HIPCK(hipStreamSynchronize(st));
		RCK(bdp_batch_check(n, info, G != nullptr, fn, bc != nullptr, bc && bc->pack));
		if (info[0] > n) { bmh_set_error("%s: internal error: %u templates among %u records", fn, info[0], n); return BMH_EINVAL; }
		dh->tpl.resize(n); dh->entries.resize(n ? info[0] : 0); dh->secsup = info[2]; dh->unmapped = info[3];
		if (n) HIPCK(hipMemcpyAsync(dh->tpl.data(), d_tpl_sorted, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
		if (!dh->entries.empty()) HIPCK(hipMemcpyAsync(dh->entries.data(), d_e, sizeof(bdp_entry_t) * dh->entries.size(), hipMemcpyDeviceToHost, st));
		if (bc) dh->bcs.resize(dh->entries.size());
		if (bc && !dh->bcs.empty()) HIPCK(hipMemcpyAsync(dh->bcs.data(), d_b, 8 * dh->bcs.size(), hipMemcpyDeviceToHost, st));
	}
	sorted.resize((size_t)n_bytes + 1); keys.resize((size_t)n + 1); soff.resize((size_t)n + 1);
	if (n_bytes) HIPCK(hipMemcpyAsync(sorted.data(), ds, (size_t)n_bytes, hipMemcpyDeviceToHost, st));
	if (n) HIPCK(hipMemcpyAsync(keys.data(), dk, 8 * (size_t)n, hipMemcpyDeviceToHost, st));
	HIPCK(hipMemcpyAsync(soff.data(), dso, 8 * ((size_t)n + 1), hipMemcpyDeviceToHost, st));
	HIPCK(hipStreamSynchronize(st));
	HIPCK(hipGetLastError());
	if (soff[n] != n_bytes) { bmh_set_error("sorted BAM: internal error: the sorted records hold %llu bytes, the input %llu", (unsigned long long)soff[n], (unsigned long long)n_bytes); return BMH_EINVAL; }
	return BMH_OK;
}
}   // namespace

extern "C" int bmh_bam_sort_device(const uint8_t *recs, uint64_t n_bytes, void *stream, uint8_t **out)
{
	const char *fn = "bmh_bam_sort_device";
	if (!out || (n_bytes && !recs)) { bmh_set_error("%s: null argument", fn); return BMH_EINVAL; }
	*out = nullptr;
	std::vector<uint64_t> off, keys, soff; std::vector<uint8_t> sorted;
	RCK(bsr_walk(recs, n_bytes, -1, off, fn));
	bsr_dev_t d;
	RCK(to_store(&d, recs, n_bytes, off, (hipStream_t)stream, sorted, keys, soff, nullptr, fn, bdp_plan_t()));
	uint8_t *o = (uint8_t *)malloc((size_t)n_bytes + 1);
	if (!o) { bmh_set_error("%s: out of memory", fn); return BMH_ENOMEM; }
	memcpy(o, sorted.data(), (size_t)n_bytes);
	*out = o;
	return BMH_OK;
}

// the records of a checked stand-alone file (csrc/bam_sort.h: bsr_file_t) -> one sorted run, merged into F.file
static int sorted_file_device(bsr_file_t &F, const uint8_t *recs, uint64_t n_bytes, void *stream)
{
	const char *fn = F.fn; bsr_out_t &J = F.J; const std::vector<uint64_t> &off = F.off; const bdp_plan_t &P = J.P;
	std::vector<uint64_t> keys, soff; std::vector<uint8_t> sorted;
	bsr_dev_t d;
	bsr_store_t S;
	if (J.markdup)
		for (size_t i = 0; i + 1 < off.size(); ++i)
			if (!bdp_record_whole(recs + off[i], off[i + 1] - off[i])) { bmh_set_error("%s: record %zu is cut: its bases and qualities do not lie inside its block_size", fn, i); return BMH_EINVAL; }
	dup_host_t dh;
	if (off.size() > 1) {
		RCK(to_store(&d, recs, n_bytes, off, (hipStream_t)stream, sorted, keys, soff, J.markdup ? &dh : nullptr, fn, P));
		bsr_dup_t bd = {dh.tpl.data(), dh.entries.data(), (uint32_t)dh.entries.size(), dh.secsup, dh.unmapped};
		if (P.barcode()) bd.bcs = dh.bcs.data();
		RCK(S.append(sorted.data(), n_bytes, keys.data(), soff.data(), off.size() - 1, J.markdup ? &bd : nullptr));
	}
	bmh_bam_ws_t *ws = bmh_bam_ws_create();
	const int rc = bsr_write_device(&d, ws, S, J, stream, bsr_sink_string, &F.file, fn);
	bmh_bam_ws_free(ws);
	if (rc != BMH_OK) return rc;
	if (P.groups() && P.lib_counts && off.size() > 1)
		bdp_lib_tally_host(sorted.data(), soff.data(), (uint32_t)(off.size() - 1), dh.tpl.data(), dh.entries.data(), dh.entries.size(), P.n_lib(), P.lib_counts);
	return BMH_OK;
}

extern "C" int bmh_bam_sorted_file_device(const char *header_text, int n_contigs, const char *const *contig_names, const int32_t *contig_len, const uint8_t *recs, uint64_t n_bytes,
                                          const bmh_sorted_opt_t *opt, void *stream, uint8_t **bam, uint64_t *bam_bytes, uint8_t **index, uint64_t *index_bytes, bmh_sorted_results_t *res)
{
	const char *fn = "bmh_bam_sorted_file_device";
	bsr_file_t F;
	int rc = F.begin(fn, header_text, n_contigs, contig_names, contig_len, recs, n_bytes, opt, bam, bam_bytes, index, index_bytes, res);
	if (rc == BMH_OK) rc = sorted_file_device(F, recs, n_bytes, stream);
	return F.end(rc, res);
}
