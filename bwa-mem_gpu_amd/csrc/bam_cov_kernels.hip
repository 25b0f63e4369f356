// Coverage depth of the sorted file's windows on the device (csrc/bam_cov_core.h's rules).  A window's records are in coordinate order and carry
// their final flags when this runs (csrc/bam_sort_kernels.hip, behind the flag step).
//
//   count    one lane per record: the filters, the refusals (the smallest record index of a window wins, through a 64-bit atomicMin; a window is refused before the next one runs), the record's events (two per covered
//            run), and n_reads / sum_mapq -- one atomicAdd each per block where the block's counted records share a contig, which in a sorted file nearly every block's do
//   emit     an exclusive scan of the counts, then one lane per record walks its operations again and writes its event keys behind the events kept from the
//            windows before
//   order    rocprim's radix sort of the keys; an event is final when its tile begins before the frontier -- the tile of the window's last record's start, since
//            every later record begins there or behind it.  One lane per event: its difference (+1 / -1, 0 when it is kept), whether it is the first of its tile;
//            an inclusive scan of the differences gives the depth behind every event, an exclusive scan of the heads numbers the tiles that hold events
//   tile     one block per such tile: the events go into a difference array of `tile` words in LDS -- integer atomics, so the sum does not depend on the order of
//            arrival; lanes of a wave that hold one position (sorted events: neighbours) are combined by ballots before one of them adds -- then a block scan
//            with the depth carried into the tile, and per lane a walk over its positions: covered bases, depth sum and maximum (through LDS where the tile lies
//            in one contig, then one atomic each per block), the histogram in LDS (flushed once per block) and the bins (added: a bin may straddle tiles).  The
//            stretch between this tile and the one before it has no event: its depth is the carry, and it is added in closed form when that is not 0
//   carry    the events of tiles at or behind the frontier stay for the next window (the sorted keys' tail); the depth behind the last final event and the
//            first position not added yet stay on the device.  Depth 0 is never visited: hist[0] is the genome's length less the other bins
// The tile pass is laid out for the default tile (4096 positions: 16 per lane).  Tiles of a few positions are taken because the tests move the carry's edges into
// small inputs with them; each still costs a block of 256 lanes and a histogram of 1001 words, which no run that is timed should pay.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <rocprim/rocprim.hpp>
#include <algorithm>
#include <vector>
#include "bam_cov.h"
#include "bam_sort.h"
#include "devmem.h"

enum { ST_ERR = 0, ST_NNOW, ST_NA, ST_CARRY, ST_DONE, ST_WORDS = 8 };

struct bcv_dev_t {
	bcv_plan_t P;
	dev_buf<uint8_t> coff, clen, binoff, stats, hist, bins, st;       // the plan and the results; st: the state words
	dev_buf<uint8_t> cnt, eoff, ev, ev2, delta, depth, head, tidx, tfirst, tmp;
	uint64_t n_pending = 0, n_seen = 0;
	hipEvent_t evt[2] = {nullptr, nullptr};
	bool combine = true, timing = false;                              // timing: evt[1] is recorded and not read yet
	~bcv_dev_t() { for (hipEvent_t e : evt) if (e) (void)hipEventDestroy(e); }
};

namespace {

__global__ void __launch_bounds__(256) bcv_count(const uint8_t *__restrict__ recs, const uint64_t *__restrict__ soff, uint32_t n, int n_contigs, int min_mapq, bool deletions,
                                                 const int64_t *__restrict__ clen, uint64_t rec_base, uint32_t *__restrict__ cnt, unsigned long long *st,
                                                 unsigned long long *n_reads, unsigned long long *sum_mapq)
{
	__shared__ int rc; __shared__ unsigned int mq;
	const uint32_t j = blockIdx.x * 256 + threadIdx.x;
	if (threadIdx.x == 0) { rc = -1; mq = 0; }
	__syncthreads();
	int32_t r = -1; uint32_t m = 0, c = 0;
	if (j < n) {
		const uint8_t *rec = recs + soff[j];
		const uint64_t size = soff[j + 1] - soff[j];
		if (size >= BSR_FIXED && bcv_counted(rec, n_contigs, min_mapq)) {
			r = bsr_ref(rec);
			const int e = bcv_check(rec, size, clen[r]);
			if (e != BCV_OK) { atomicMin(st + ST_ERR, (unsigned long long)((rec_base + j) << 2 | (uint64_t)e)); r = -1; }
			else { m = bcv_mapq(rec); c = 2 * bcv_runs(rec, clen[r], deletions, [](int64_t, int64_t) {}); }
		}
		cnt[j] = c;
	}
	if (r >= 0) rc = r;                                               // (any counted lane's contig)
	__syncthreads();
	const int r0 = rc;
	if (r0 < 0) return;
	if (__syncthreads_and(r < 0 || r == r0)) {
		const int k = __syncthreads_count(r >= 0);
		if (m) atomicAdd(&mq, m);
		__syncthreads();
		if (threadIdx.x == 0) { atomicAdd(n_reads + r0, (unsigned long long)k); if (mq) atomicAdd(sum_mapq + r0, (unsigned long long)mq); }
	} else if (r >= 0) { atomicAdd(n_reads + r, 1ull); if (m) atomicAdd(sum_mapq + r, (unsigned long long)m); }
}

__global__ void __launch_bounds__(256) bcv_emit(const uint8_t *__restrict__ recs, const uint64_t *__restrict__ soff, uint32_t n, bool deletions, const int64_t *__restrict__ clen,
                                                const uint64_t *__restrict__ coff, const uint32_t *__restrict__ cnt, const uint64_t *__restrict__ eoff, uint64_t first, uint64_t cap,
                                                uint64_t *__restrict__ ev)
{
	const uint32_t j = blockIdx.x * 256 + threadIdx.x;
	if (j >= n) return;
	const uint32_t c = cnt[j];
	if (!c) return;                                                  // (counted and checked: only such records have events)
	const uint8_t *rec = recs + soff[j];
	const int32_t r = bsr_ref(rec);
	const uint64_t o = coff[r], base = first + eoff[j];
	uint32_t w = 0;
	bcv_runs(rec, clen[r], deletions, [&](int64_t b, int64_t e) {
		if (w + 2 <= c && base + w + 2 <= cap) { ev[base + w] = bcv_key(o + (uint64_t)b, true); ev[base + w + 1] = bcv_key(o + (uint64_t)e, false); }
		w += 2;
	});
}

__global__ void __launch_bounds__(256) bcv_mark(const uint64_t *__restrict__ ev, uint32_t n_all, uint64_t ft, uint32_t T, uint32_t *__restrict__ delta, uint32_t *__restrict__ head,
                                                unsigned long long *st)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n_all) return;
	const uint64_t key = ev[i], g = key >> 1;
	const bool now = g < ft;
	delta[i] = now ? ((key & 1) ? 1u : 0xffffffffu) : 0u;
	head[i] = now && (i == 0 || (ev[i - 1] >> 1) / T != g / T) ? 1u : 0u;
	if (now && (i + 1 == n_all || (ev[i + 1] >> 1) >= ft)) st[ST_NNOW] = i + 1;
}

__global__ void __launch_bounds__(256) bcv_tile_first(const uint32_t *__restrict__ head, const uint32_t *__restrict__ tidx, uint32_t n_all, uint32_t *__restrict__ tfirst, unsigned long long *st)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n_all) return;
	if (head[i] && tidx[i] < n_all) tfirst[tidx[i]] = i;
	if (i == 0) st[ST_NA] = tidx[n_all];
}

// lanes of a wave that hold one position add once: the first of them, the sum of their +1 and -1 (every lane of the wave calls this)
template <bool COMBINE> __device__ inline void bcv_diff_add(uint32_t *diff, bool valid, uint32_t idx, bool start)
{
	if (!COMBINE) { if (valid) atomicAdd(diff + idx, start ? 1u : 0xffffffffu); return; }
	unsigned long long todo = __ballot(valid);
	const uint32_t lane = threadIdx.x & 63u;
	while (todo) {
		const int leader = __ffsll((long long)todo) - 1;
		const uint32_t at = __shfl(idx, leader);
		const bool mine = valid && idx == at;
		const unsigned long long grp = __ballot(mine), plus = __ballot(mine && start);
		if (lane == (uint32_t)leader) atomicAdd(diff + at, (uint32_t)__popcll(plus) - (uint32_t)(__popcll(grp) - __popcll(plus)));
		todo &= ~grp;
	}
}

// positions [a, b) without events at depth d > 0, by the whole block: the words by lane 0, the bins by all lanes
__device__ void bcv_stretch(uint64_t a, uint64_t b, uint32_t d, const uint64_t *__restrict__ coff, const uint64_t *__restrict__ binoff, int n_contigs, uint32_t bin,
                            unsigned long long *stats, unsigned long long *hist, unsigned long long *bins)
{
	const uint64_t G = coff[n_contigs];
	if (b > G) b = G;
	while (a < b) {
		const int c = bcv_contig_of(coff, n_contigs, a);
		const uint64_t o = coff[c], e = b < coff[c + 1] ? b : coff[c + 1], len = e - a;
		if (threadIdx.x == 0) {
			atomicAdd(stats + 1ull * n_contigs + c, (unsigned long long)len); atomicAdd(stats + 2ull * n_contigs + c, (unsigned long long)d * len);
			atomicMax(stats + 3ull * n_contigs + c, (unsigned long long)d);
			atomicAdd(hist + (d < BCV_HIST - 1 ? d : BCV_HIST - 1), (unsigned long long)len);
		}
		if (bin) {
			const uint64_t k1 = (e - 1 - o) / bin;
			for (uint64_t k = (a - o) / bin + threadIdx.x; k <= k1; k += 256) {
				const uint64_t lo = a - o > k * bin ? a - o : k * bin, hi = e - o < (k + 1) * bin ? e - o : (k + 1) * bin;
				atomicAdd(bins + binoff[c] + k, (unsigned long long)d * (hi - lo));
			}
		}
		a = e;
	}
}

template <bool COMBINE>
__global__ void __launch_bounds__(256) bcv_tile(const uint64_t *__restrict__ ev, const uint32_t *__restrict__ depth, const uint32_t *__restrict__ tfirst, const unsigned long long *__restrict__ st,
                                                uint32_t T, const uint64_t *__restrict__ coff, const uint64_t *__restrict__ binoff, int n_contigs, uint32_t bin,
                                                unsigned long long *stats, unsigned long long *hist, unsigned long long *bins)
{
	using scan_t = rocprim::block_scan<uint32_t, 256>;
	__shared__ uint32_t diff[BCV_TILE_MAX];
	__shared__ uint32_t lh[BCV_HIST];
	__shared__ unsigned long long acc[3];
	__shared__ typename scan_t::storage_type scan_mem;
	const uint32_t k = blockIdx.x, tid = threadIdx.x, na = (uint32_t)st[ST_NA], n_now = (uint32_t)st[ST_NNOW];
	if (k >= na || T == 0 || T > (uint32_t)BCV_TILE_MAX) return;
	const uint32_t e0 = tfirst[k], e1 = k + 1 < na ? tfirst[k + 1] : n_now;
	if (e0 >= e1 || e1 > n_now) return;
	const uint64_t G = coff[n_contigs], t0 = (ev[e0] >> 1) / T * T;
	const uint32_t cin = (uint32_t)st[ST_CARRY] + (e0 ? depth[e0 - 1] : 0u);
	const uint64_t prev_end = k ? ((ev[tfirst[k - 1]] >> 1) / T + 1) * T : (uint64_t)st[ST_DONE];
	for (uint32_t p = tid; p < T; p += 256) diff[p] = 0;
	for (uint32_t h = tid; h < (uint32_t)BCV_HIST; h += 256) lh[h] = 0;
	if (tid < 3) acc[tid] = 0;
	__syncthreads();
	for (uint32_t base = e0; base < e1; base += 256) {
		const uint32_t i = base + tid;
		bool valid = i < e1, start = false; uint32_t idx = 0;
		if (valid) { const uint64_t key = ev[i], at = (key >> 1) - t0; start = key & 1; valid = at < T; idx = (uint32_t)at; }
		bcv_diff_add<COMBINE>(diff, valid, idx, start);
	}
	__syncthreads();
	if (cin && prev_end < t0) bcv_stretch(prev_end, t0, cin, coff, binoff, n_contigs, bin, stats, hist, bins);
	// the scan: every lane a stretch of the tile, the stretches' sums through the block scan
	const uint32_t per = (T + 255) / 256, p0 = tid * per < T ? tid * per : T, p1 = p0 + per < T ? p0 + per : T;
	uint32_t s = 0, ex = 0;
	for (uint32_t p = p0; p < p1; ++p) s += diff[p];
	scan_t().exclusive_scan(s, ex, 0u, scan_mem);
	uint32_t d = cin + ex;
	// the tile within one contig (nearly every tile): the three words through LDS, one atomic each per block
	const uint64_t t_end = t0 + T < G ? t0 + T : G;
	int cs = -1;
	if (t0 < G) { cs = bcv_contig_of(coff, n_contigs, t0); if (bcv_contig_of(coff, n_contigs, t_end - 1) != cs) cs = -1; }
	int c = -1; uint64_t c_beg = 0, c_end = 0, cov = 0, sum = 0, mx = 0, bk = ~0ull, bacc = 0; uint32_t hd = 0, hn = 0;
	for (uint32_t p = p0; p < p1; ++p) {
		d += diff[p];
		const uint64_t g = t0 + p;
		if (!d || g >= G) continue;
		if (c < 0 || g >= c_end) {
			if (c >= 0 && cs < 0) {
				atomicAdd(stats + 1ull * n_contigs + c, (unsigned long long)cov); atomicAdd(stats + 2ull * n_contigs + c, (unsigned long long)sum); atomicMax(stats + 3ull * n_contigs + c, (unsigned long long)mx);
				cov = sum = mx = 0;
			}
			c = cs >= 0 ? cs : bcv_contig_of(coff, n_contigs, g); c_beg = coff[c]; c_end = coff[c + 1];
		}
		++cov; sum += d; if (d > mx) mx = d;
		const uint32_t hb = d < (uint32_t)BCV_HIST - 1 ? d : (uint32_t)BCV_HIST - 1;
		if (hb == hd) ++hn; else { if (hn) atomicAdd(lh + hd, hn); hd = hb; hn = 1; }
		if (bin) {
			const uint64_t b = binoff[c] + (uint32_t)(g - c_beg) / bin;
			if (b != bk) { if (bacc) atomicAdd(bins + bk, (unsigned long long)bacc); bk = b; bacc = 0; }
			bacc += d;
		}
	}
	if (hn) atomicAdd(lh + hd, hn);
	if (bacc) atomicAdd(bins + bk, (unsigned long long)bacc);
	if (c >= 0 && cs < 0) { atomicAdd(stats + 1ull * n_contigs + c, (unsigned long long)cov); atomicAdd(stats + 2ull * n_contigs + c, (unsigned long long)sum); atomicMax(stats + 3ull * n_contigs + c, (unsigned long long)mx); }
	if (c >= 0 && cs >= 0) { atomicAdd(acc + 0, (unsigned long long)cov); atomicAdd(acc + 1, (unsigned long long)sum); atomicMax(acc + 2, (unsigned long long)mx); }
	__syncthreads();
	if (tid == 0 && cs >= 0 && acc[0]) { atomicAdd(stats + 1ull * n_contigs + cs, acc[0]); atomicAdd(stats + 2ull * n_contigs + cs, acc[1]); atomicMax(stats + 3ull * n_contigs + cs, acc[2]); }
	for (uint32_t h = tid; h < (uint32_t)BCV_HIST; h += 256) if (lh[h]) atomicAdd(hist + h, (unsigned long long)lh[h]);
}

// behind a sweep's tiles: the depth behind the last final event, the first position not added
__global__ void bcv_state(const uint64_t *__restrict__ ev, const uint32_t *__restrict__ depth, const uint32_t *__restrict__ tfirst, uint32_t T, unsigned long long *st)
{
	const uint32_t na = (uint32_t)st[ST_NA], n_now = (uint32_t)st[ST_NNOW];
	if (!na || !n_now) return;
	st[ST_DONE] = ((ev[tfirst[na - 1]] >> 1) / T + 1) * T;
	st[ST_CARRY] = (uint32_t)((uint32_t)st[ST_CARRY] + depth[n_now - 1]);
}

// a buffer of at least n bytes that keeps its first `keep`
int grow_keep(dev_buf<uint8_t> &b, size_t n, size_t keep, hipStream_t st)
{
	if (n <= b.cap) return BMH_OK;
	dev_buf<uint8_t> nb;
	RCK(nb.resize(bmh_grow_cap(n)));
	if (keep) { HIPCK(hipMemcpyAsync(nb.p, b.p, keep, hipMemcpyDeviceToDevice, st)); HIPCK(hipStreamSynchronize(st)); }
	b.swap(nb);
	return BMH_OK;
}

// the events ev [n_all] (kept ones first, unsorted) -> every tile that begins before ft added; the rest kept
int sweep(bcv_dev_t *d, uint64_t n_all, uint64_t ft, hipStream_t st, const char *fn)
{
	if (!n_all) return BMH_OK;
	if (n_all >= 0xfffffff0ull) { bmh_set_error("%s: %llu coverage events in one window: fewer than 2^32 are taken (a smaller window holds fewer)", fn, (unsigned long long)n_all); return BMH_EINVAL; }
	const uint32_t n = (uint32_t)n_all, T = (uint32_t)d->P.tile;
	size_t sb = 0, t1 = scan_tmp_bytes<uint32_t, uint32_t, true>((size_t)n), t2 = scan_tmp_bytes<uint32_t, uint32_t>((size_t)n + 1);
	HIPCK(rocprim::radix_sort_keys(nullptr, sb, (uint64_t *)nullptr, (uint64_t *)nullptr, (size_t)n, 0, 64, st));
	RCK(d->tmp.need(std::max(sb + 256, std::max(t1, t2))));
	RCK(d->ev2.need(8 * ((size_t)n + 1))); RCK(d->delta.need(4 * ((size_t)n + 1))); RCK(d->depth.need(4 * ((size_t)n + 1))); RCK(d->head.need(4 * ((size_t)n + 2)));
	RCK(d->tidx.need(4 * ((size_t)n + 2))); RCK(d->tfirst.need(4 * ((size_t)n + 2)));
	sb = d->tmp.cap;
	HIPCK(rocprim::radix_sort_keys(d->tmp.p, sb, (uint64_t *)d->ev.p, (uint64_t *)d->ev2.p, (size_t)n, 0, 64, st));
	unsigned long long *S = (unsigned long long *)d->st.p;
	HIPCK(hipMemsetAsync(S + ST_NNOW, 0, 16, st));                      // (ST_NNOW, ST_NA)
	HIPCK(hipMemsetAsync((uint32_t *)d->head.p + n, 0, 4, st));
	bcv_mark<<<(n + 255) / 256, 256, 0, st>>>((const uint64_t *)d->ev2.p, n, ft, T, (uint32_t *)d->delta.p, (uint32_t *)d->head.p, S);
	HIPCK(rocprim::inclusive_scan(d->tmp.p, t1, (uint32_t *)d->delta.p, (uint32_t *)d->depth.p, (size_t)n, rocprim::plus<uint32_t>(), st));
	HIPCK(rocprim::exclusive_scan(d->tmp.p, t2, (uint32_t *)d->head.p, (uint32_t *)d->tidx.p, 0u, (size_t)n + 1, rocprim::plus<uint32_t>(), st));
	bcv_tile_first<<<(n + 255) / 256, 256, 0, st>>>((const uint32_t *)d->head.p, (const uint32_t *)d->tidx.p, n, (uint32_t *)d->tfirst.p, S);
	uint64_t h[ST_WORDS];
	HIPCK(hipMemcpyAsync(h, S, sizeof h, hipMemcpyDeviceToHost, st));
	HIPCK(hipStreamSynchronize(st));
	HIPCK(hipGetLastError());
	const uint64_t n_now = h[ST_NNOW], na = h[ST_NA];
	if (n_now > n || na > n_now || (n_now && !na)) { bmh_set_error("%s: internal error: %llu tiles for %llu of %u coverage events", fn, (unsigned long long)na, (unsigned long long)n_now, n); return BMH_EINVAL; }
	if (na) {
		const uint32_t bin = (uint32_t)d->P.bin; const int nc = d->P.n_contigs;
		(d->combine ? bcv_tile<true> : bcv_tile<false>)<<<(unsigned)na, 256, 0, st>>>((const uint64_t *)d->ev2.p, (const uint32_t *)d->depth.p, (const uint32_t *)d->tfirst.p, S, T,
		        (const uint64_t *)d->coff.p, (const uint64_t *)d->binoff.p, nc, bin, (unsigned long long *)d->stats.p, (unsigned long long *)d->hist.p, (unsigned long long *)d->bins.p);
		bcv_state<<<1, 1, 0, st>>>((const uint64_t *)d->ev2.p, (const uint32_t *)d->depth.p, (const uint32_t *)d->tfirst.p, T, S);
	}
	d->n_pending = n - n_now;
	if (d->n_pending) HIPCK(hipMemcpyAsync(d->ev.p, (const uint64_t *)d->ev2.p + n_now, 8 * (size_t)d->n_pending, hipMemcpyDeviceToDevice, st));
	HIPCK(hipGetLastError());
	return BMH_OK;
}

// events around a step when its milliseconds are asked for: they are only recorded here and read behind the caller's own wait for the stream (bcv_window_ms), as
// the flag step's are.  The span runs from the step's first kernel to its last, so it holds the step's host reads (the event count, the tile count) as well
struct timed_t {
	bcv_dev_t *d; hipStream_t st; double *ms;
	int begin() { if (!ms) return BMH_OK; for (hipEvent_t &e : d->evt) if (!e) HIPCK(hipEventCreate(&e)); HIPCK(hipEventRecord(d->evt[0], st)); return BMH_OK; }
	int end() { if (!ms) return BMH_OK; HIPCK(hipEventRecord(d->evt[1], st)); d->timing = true; return BMH_OK; }
};

}   // namespace

bcv_dev_t *bcv_dev_create(void) { return new bcv_dev_t(); }
void bcv_dev_free(bcv_dev_t *d) { delete d; }

int bcv_begin_device(bcv_dev_t *d, const bcv_plan_t &P, void *stream)
{
	hipStream_t st = (hipStream_t)stream;
	d->P = P; d->n_pending = 0; d->n_seen = 0; d->combine = bmh_tune("COV_COMBINE", 1) != 0;
	const size_t n = (size_t)P.n_contigs, nb = (size_t)P.n_bins();
	if (8 * nb > d->bins.cap) {                                       // the bins are the one buffer that grows with the genome (divided by the bin): counted before it is allocated
		size_t fr = 0, tot = 0;
		HIPCK(hipMemGetInfo(&fr, &tot));
		const size_t want = bmh_grow_cap(8 * nb) + (64u << 20);
		if (want > fr + d->bins.cap) { bmh_set_error("coverage: %zu bins need %zu bytes of device memory, %zu are free (choose a larger bin)", nb, want, fr + d->bins.cap); return BMH_ENOMEM; }
	}
	RCK(d->coff.need(8 * (n + 1))); RCK(d->clen.need(8 * (n + 1))); RCK(d->binoff.need(8 * (n + 1))); RCK(d->stats.need(8 * (5 * n + 1))); RCK(d->hist.need(8 * (size_t)BCV_HIST));
	RCK(d->bins.need(8 * (nb + 1))); RCK(d->st.need(8 * (size_t)ST_WORDS));
	HIPCK(hipMemcpyAsync(d->coff.p, P.coff.data(), 8 * (n + 1), hipMemcpyHostToDevice, st));
	if (n) HIPCK(hipMemcpyAsync(d->clen.p, P.len.data(), 8 * n, hipMemcpyHostToDevice, st));
	HIPCK(hipMemcpyAsync(d->binoff.p, P.bin_off.data(), 8 * (n + 1), hipMemcpyHostToDevice, st));
	HIPCK(hipMemsetAsync(d->stats.p, 0, 8 * (5 * n + 1), st)); HIPCK(hipMemsetAsync(d->hist.p, 0, 8 * (size_t)BCV_HIST, st)); HIPCK(hipMemsetAsync(d->bins.p, 0, 8 * (nb + 1), st));
	HIPCK(hipMemsetAsync(d->st.p, 0, 8 * (size_t)ST_WORDS, st));
	HIPCK(hipMemsetAsync(d->st.p, 0xff, 8, st));                       // (ST_ERR: no record refused)
	HIPCK(hipStreamSynchronize(st));                                   // (the plan's vectors are the caller's)
	return BMH_OK;
}

int bcv_window_device(bcv_dev_t *d, const uint8_t *d_recs, const uint64_t *d_soff, uint32_t n, const uint8_t *last, void *stream, const char *fn, double *ms)
{
	hipStream_t st = (hipStream_t)stream;
	if (!n) return BMH_OK;
	timed_t tm = {d, st, ms};
	RCK(tm.begin());
	const bcv_plan_t &P = d->P;
	size_t tb = scan_tmp_bytes<uint32_t, uint64_t>((size_t)n + 1);
	RCK(d->cnt.need(4 * ((size_t)n + 2))); RCK(d->eoff.need(8 * ((size_t)n + 2))); RCK(d->tmp.need(tb));
	unsigned long long *S = (unsigned long long *)d->st.p, *stats = (unsigned long long *)d->stats.p;
	HIPCK(hipMemsetAsync((uint32_t *)d->cnt.p + n, 0, 4, st));
	bcv_count<<<(n + 255) / 256, 256, 0, st>>>(d_recs, d_soff, n, P.n_contigs, P.min_mapq, P.deletions, (const int64_t *)d->clen.p, d->n_seen, (uint32_t *)d->cnt.p, S, stats, stats + 4ull * P.n_contigs);
	HIPCK(rocprim::exclusive_scan(d->tmp.p, tb, (uint32_t *)d->cnt.p, (uint64_t *)d->eoff.p, (uint64_t)0, (size_t)n + 1, rocprim::plus<uint64_t>(), st));
	uint64_t n_ev = 0, err = 0;
	HIPCK(hipMemcpyAsync(&n_ev, (const uint64_t *)d->eoff.p + n, 8, hipMemcpyDeviceToHost, st));
	HIPCK(hipMemcpyAsync(&err, S + ST_ERR, 8, hipMemcpyDeviceToHost, st));
	HIPCK(hipStreamSynchronize(st));
	HIPCK(hipGetLastError());
	if (err != ~0ull) return bcv_refused(err >> 2, (int)(err & 3), fn);
	const uint64_t n_all = d->n_pending + n_ev;
	RCK(grow_keep(d->ev, 8 * ((size_t)n_all + 1), 8 * (size_t)d->n_pending, st));
	if (n_ev) bcv_emit<<<(n + 255) / 256, 256, 0, st>>>(d_recs, d_soff, n, P.deletions, (const int64_t *)d->clen.p, (const uint64_t *)d->coff.p, (const uint32_t *)d->cnt.p, (const uint64_t *)d->eoff.p,
	                                                    d->n_pending, n_all, (uint64_t *)d->ev.p);
	d->n_seen += n;
	const uint64_t f = bcv_frontier(last, P.coff.data(), P.len.data(), P.n_contigs);
	RCK(sweep(d, n_all, f / P.tile * P.tile, st, fn));
	return tm.end();
}

int bcv_window_ms(bcv_dev_t *d, double *ms)
{
	if (!d->timing || !ms) return BMH_OK;
	float t = 0;
	HIPCK(hipEventElapsedTime(&t, d->evt[0], d->evt[1]));
	ms[0] += t; ms[1] += 1; d->timing = false;
	return BMH_OK;
}

int bcv_finish_device(bcv_dev_t *d, void *stream, bcv_result_t &R, const char *fn, double *ms)
{
	hipStream_t st = (hipStream_t)stream;
	timed_t tm = {d, st, ms};
	RCK(tm.begin());
	const bcv_plan_t &P = d->P;
	RCK(sweep(d, d->n_pending, ~0ull, st, fn));
	RCK(tm.end());
	R.init(P);
	const size_t n = (size_t)P.n_contigs;
	std::vector<uint64_t> s(5 * n + 1); uint64_t h[ST_WORDS];
	HIPCK(hipMemcpyAsync(s.data(), d->stats.p, 8 * (5 * n + 1), hipMemcpyDeviceToHost, st));
	HIPCK(hipMemcpyAsync(R.hist.data(), d->hist.p, 8 * (size_t)BCV_HIST, hipMemcpyDeviceToHost, st));
	if (!R.bin_sum.empty()) HIPCK(hipMemcpyAsync(R.bin_sum.data(), d->bins.p, 8 * R.bin_sum.size(), hipMemcpyDeviceToHost, st));
	HIPCK(hipMemcpyAsync(h, d->st.p, sizeof h, hipMemcpyDeviceToHost, st));
	HIPCK(hipStreamSynchronize(st));
	HIPCK(hipGetLastError());
	if (d->timing && ms) { float t = 0; HIPCK(hipEventElapsedTime(&t, d->evt[0], d->evt[1])); ms[0] += t; d->timing = false; }      // (the last sweep: no window of its own)
	if (d->n_pending || h[ST_CARRY]) { bmh_set_error("%s: internal error: a depth of %llu is left behind the last event", fn, (unsigned long long)h[ST_CARRY]); return BMH_EINVAL; }
	for (size_t c = 0; c < n; ++c) { R.n_reads[c] = s[c]; R.cov_bases[c] = s[n + c]; R.sum_depth[c] = s[2 * n + c]; R.max_depth[c] = s[3 * n + c]; R.sum_mapq[c] = s[4 * n + c]; }
	R.close(P);
	return BMH_OK;
}

extern "C" int bmh_bam_coverage_device(const uint8_t *recs, uint64_t n_bytes, int n_contigs, const int32_t *contig_len, const bmh_coverage_opt_t *opt, void *stream, bmh_coverage_t *out)
{
	const char *fn = "bmh_bam_coverage_device";
	hipStream_t st = (hipStream_t)stream;
	if (!out || (n_bytes && !recs)) { bmh_set_error("%s: null argument", fn); return BMH_EINVAL; }
	memset(out, 0, sizeof *out);
	bmh_coverage_opt_t o; bmh_coverage_opt_default(&o);
	if (opt) o = *opt;
	bcv_plan_t P;
	RCK(bcv_plan_make(P, o.min_mapq, o.deletions, o.bin, o.tile, n_contigs, contig_len, fn));
	std::vector<uint64_t> off;
	RCK(bsr_walk(recs, n_bytes, -1, off, fn));
	size_t n = off.size() - 1, bad = 0;
	// the order is the one thing the walk can see that a lane cannot: a record against the one before it, across windows.  The first record out of order ends the
	// stream here; the lanes refuse what lies before it, so the first refusal of any kind is the one reported, as on the host
	for (size_t i = 1; i < n && !bad; ++i) if ((bsr_key(recs + off[i]) >> 1) < (bsr_key(recs + off[i - 1]) >> 1)) bad = i;
	if (bad) n = bad;
	bcv_dev_t d; bcv_result_t R;
	RCK(bcv_begin_device(&d, P, stream));
	dev_buf<uint8_t> in, in_off;
	const uint64_t W = std::max<uint64_t>(1, (64ull << 20) / std::max<uint64_t>(1, n ? n_bytes / n : 1));
	std::vector<uint64_t> rel;
	for (size_t a = 0; a < n; a += W) {                                // windows of about 64 MiB of records, as the sorted file's merge hands them on
		const size_t b = (size_t)std::min<uint64_t>(n, a + W), m = b - a;
		const uint64_t bytes = off[b] - off[a];
		rel.resize(m + 1);
		for (size_t j = 0; j <= m; ++j) rel[j] = off[a + j] - off[a];
		RCK(in.need((size_t)bytes + 16)); RCK(in_off.need(8 * (m + 1)));
		HIPCK(hipMemcpyAsync(in.p, recs + off[a], (size_t)bytes, hipMemcpyHostToDevice, st));
		HIPCK(hipMemcpyAsync(in_off.p, rel.data(), 8 * (m + 1), hipMemcpyHostToDevice, st));
		RCK(bcv_window_device(&d, (const uint8_t *)in.p, (const uint64_t *)in_off.p, (uint32_t)m, recs + off[b - 1], stream, fn, nullptr));
		HIPCK(hipStreamSynchronize(st));
	}
	if (bad) return bcv_refused(bad, -1, fn);
	RCK(bcv_finish_device(&d, stream, R, fn, nullptr));
	return bcv_export(P, R, out, fn);
}
