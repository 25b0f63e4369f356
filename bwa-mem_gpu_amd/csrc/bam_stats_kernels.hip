// Flagstat, idxstats, alignment summary and insert sizes of the sorted file's windows on the device (csrc/bam_stats_core.h's rules).  A window's
// records are in their final order and carry their final flags when this runs (csrc/bam_sort_kernels.hip, behind the flag step, beside the coverage step).
//
//   count    one kernel, one lane per record, blocks of 256: bst_record gives what the record adds.  The sixteen pairs of flag words, the summary words, the 256
//            mapq bins and the smallest and largest insert size per orientation are accumulated in LDS with 64-bit integer atomics; every word of the block that
//            is not empty goes to the accumulator in global memory with one 64-bit atomic (add, or min / max).  Integer sums do not depend on the order of
//            arrival, so the words equal the host form's exactly
//   contigs  one atomic per block and kind where the block's placed records share a contig (in a sorted file nearly every block's do, as in bsr_index_marks and
//            bcv_count), one per lane otherwise; the records without a contig are counted per block
//   inserts  one 64-bit atomicAdd to the histogram in global memory per counted record -- at most one record in two counts
//   refused  the smallest index << 3 | code of a window through a 64-bit atomicMin; the word travels to pinned host memory behind the kernel and is read behind
//            the window's own wait (bst_window_ms), before the window's members reach the sink
// Nothing passes between windows but the accumulator and the number of records seen; the accumulator is read once, at the end of the run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "bam_stats.h"
#include "bam_sort.h"
#include "devmem.h"

struct bst_dev_t {
	bst_plan_t P;
	dev_buf<uint64_t> acc, err;                                        // the accumulator (bst_plan_t's layout); the refusal word
	pin_buf<uint64_t> h_err;
	uint64_t n_seen = 0;
	hipEvent_t evt[2] = {nullptr, nullptr};
	bool timing = false, pending = false;                              // timing: evt[1] is recorded and not read yet; pending: a window's refusal word is not read yet
	~bst_dev_t() { for (hipEvent_t e : evt) if (e) (void)hipEventDestroy(e); }
};

namespace {

__global__ void __launch_bounds__(256) bst_count(const uint8_t *__restrict__ recs, const uint64_t *__restrict__ soff, uint32_t n, int n_contigs, uint32_t cap, uint64_t rec_base,
                                                 unsigned long long *acc, unsigned long long *err)
{
	__shared__ unsigned long long lw[BST_W_LDS];
	__shared__ int rc;
	const uint32_t tid = threadIdx.x, j = blockIdx.x * 256 + tid;
	for (uint32_t k = tid; k < (uint32_t)BST_W_LDS; k += 256) lw[k] = k >= (uint32_t)BST_W_MIN && k < (uint32_t)BST_W_MAX ? ~0ull : 0ull;
	if (tid == 0) rc = -1;
	__syncthreads();
	int32_t ref = -2; bool pm = false;                                 // ref -2: no record here, or a refused one
	const uint64_t w_contig = (uint64_t)BST_W_FIXED, w_hist = w_contig + 2ull * (uint64_t)n_contigs;
	if (j < n) {
		bst_rec_t r;
		const uint64_t a = soff[j], b = soff[j + 1];
		const int st = b >= a ? bst_record(recs + a, b - a, n_contigs, r) : (int)BST_E_CUT;
		if (st != BST_OK) atomicMin(err, (unsigned long long)bst_refusal(rec_base + j, st));
		else {
			ref = r.ref; pm = r.placed_mapped;
			for (uint32_t f = r.flags; f; f &= f - 1) atomicAdd(&lw[BST_W_FLAG + BST_N_FLAG * r.qc + (uint32_t)(__ffs((int)f) - 1)], 1ull);
			if (r.primary) {
				for (int k = 0; k < BST_N_SUM; ++k) {
					if (!r.sum[k]) continue;
					if (k == BST_MAX_LEN) atomicMax(&lw[BST_W_SUM + k], (unsigned long long)r.sum[k]); else atomicAdd(&lw[BST_W_SUM + k], (unsigned long long)r.sum[k]);
				}
				if (r.mapped) atomicAdd(&lw[BST_W_MAPQ + r.mapq], 1ull);
				if (r.ori >= 0) {
					atomicAdd(acc + w_hist + bst_hist_at(r.ori, r.size, cap), 1ull);
					atomicMin(&lw[BST_W_MIN + r.ori], (unsigned long long)r.size); atomicMax(&lw[BST_W_MAX + r.ori], (unsigned long long)r.size);
				}
			}
		}
	}
	if (ref >= 0) rc = ref;                                            // (any placed lane's contig)
	__syncthreads();
	const int r0 = rc;
	const int un = __syncthreads_count(ref == -1);
	if (tid == 0 && un) atomicAdd(acc + BST_W_UNPLACED, (unsigned long long)un);
	if (r0 >= 0) {                                                     // (r0 is the block's: every lane takes the same way)
		if (__syncthreads_and(ref < 0 || ref == r0)) {
			const int km = __syncthreads_count(ref >= 0 && pm), ku = __syncthreads_count(ref >= 0 && !pm);
			if (tid == 0) {
				if (km) atomicAdd(acc + w_contig + (uint64_t)r0, (unsigned long long)km);
				if (ku) atomicAdd(acc + w_contig + (uint64_t)n_contigs + (uint64_t)r0, (unsigned long long)ku);
			}
		} else if (ref >= 0) atomicAdd(acc + w_contig + (pm ? 0ull : (uint64_t)n_contigs) + (uint64_t)ref, 1ull);
	}
	// (the barriers above stand between the lanes' LDS atomics and the flush)
	for (uint32_t k = tid; k < (uint32_t)BST_W_LDS; k += 256) {
		const unsigned long long v = lw[k];
		if (k >= (uint32_t)BST_W_MIN && k < (uint32_t)BST_W_MAX) { if (v != ~0ull) atomicMin(acc + k, v); }
		else if (!v) continue;
		else if (k >= (uint32_t)BST_W_MAX || k == (uint32_t)(BST_W_SUM + BST_MAX_LEN)) atomicMax(acc + k, v);
		else atomicAdd(acc + k, v);
	}
}

}   // namespace

bst_dev_t *bst_dev_create(void) { return new bst_dev_t(); }
void bst_dev_free(bst_dev_t *d) { delete d; }

int bst_begin_device(bst_dev_t *d, const bst_plan_t &P, void *stream)
{
	hipStream_t st = (hipStream_t)stream;
	d->P = P; d->n_seen = 0; d->timing = d->pending = false;
	RCK(d->acc.need(P.words())); RCK(d->err.need(1)); RCK(d->h_err.need(1));
	HIPCK(hipMemsetAsync(d->acc.p, 0, 8 * P.words(), st));
	HIPCK(hipMemsetAsync(d->acc.p + BST_W_MIN, 0xff, 8 * (size_t)BST_N_ORI, st));      // (no size seen yet)
	HIPCK(hipMemsetAsync(d->err.p, 0xff, 8, st));                                      // (no record refused)
	d->h_err.p[0] = ~0ull;
	return BMH_OK;
}

int bst_window_device(bst_dev_t *d, const uint8_t *d_recs, const uint64_t *d_soff, uint32_t n, void *stream, double *ms)
{
	hipStream_t st = (hipStream_t)stream;
	if (!n) return BMH_OK;
	if (ms) { for (hipEvent_t &e : d->evt) if (!e) HIPCK(hipEventCreate(&e)); HIPCK(hipEventRecord(d->evt[0], st)); }
	bst_count<<<(n + 255) / 256, 256, 0, st>>>(d_recs, d_soff, n, d->P.n_contigs, d->P.cap, d->n_seen, (unsigned long long *)d->acc.p, (unsigned long long *)d->err.p);
	HIPCK(hipGetLastError());
	if (ms) { HIPCK(hipEventRecord(d->evt[1], st)); d->timing = true; }
	HIPCK(hipMemcpyAsync(d->h_err.p, d->err.p, 8, hipMemcpyDeviceToHost, st));
	d->n_seen += n; d->pending = true;
	return BMH_OK;
}

int bst_window_ms(bst_dev_t *d, double *ms, const char *fn)
{
	if (d->timing && ms) {
		float t = 0;
		HIPCK(hipEventElapsedTime(&t, d->evt[0], d->evt[1]));
		ms[0] += t; ms[1] += 1;
	}
	d->timing = false;
	if (d->pending) {
		d->pending = false;
		const uint64_t e = d->h_err.p[0];
		if (e != ~0ull) return bst_refused(e >> 3, (int)(e & 7u), fn);
	}
	return BMH_OK;
}

int bst_finish_device(bst_dev_t *d, void *stream, bst_result_t &R, const char *fn)
{
	hipStream_t st = (hipStream_t)stream;
	const bst_plan_t &P = d->P;
	R.init(P);
	HIPCK(hipMemcpyAsync(R.w.data(), d->acc.p, 8 * P.words(), hipMemcpyDeviceToHost, st));
	HIPCK(hipStreamSynchronize(st));
	HIPCK(hipGetLastError());
	RCK(bst_window_ms(d, nullptr, fn));                                // (a window whose word nobody has read yet)
	R.close(P);
	return BMH_OK;
}

extern "C" int bmh_bam_stats_device(const uint8_t *recs, uint64_t n_bytes, int n_contigs, const bmh_bam_stats_opt_t *opt, void *stream, bmh_bam_stats_t *out)
{
	const char *fn = "bmh_bam_stats_device";
	hipStream_t st = (hipStream_t)stream;
	if (!out || (n_bytes && !recs)) { bmh_set_error("%s: null argument", fn); return BMH_EINVAL; }
	memset(out, 0, sizeof *out);
	bmh_bam_stats_opt_t o; bmh_bam_stats_opt_default(&o);
	if (opt) o = *opt;
	bst_plan_t P;
	RCK(bst_plan_make(P, o.insert_cap, n_contigs, fn));
	std::vector<uint64_t> off;
	RCK(bst_walk(recs, n_bytes, off, fn));
	const size_t n = off.size() - 1;
	bst_dev_t d; bst_result_t R;
	RCK(bst_begin_device(&d, P, stream));
	dev_buf<uint8_t> in; dev_buf<uint64_t> in_off;
	const uint64_t W = std::max<uint64_t>(1, (64ull << 20) / std::max<uint64_t>(1, n ? n_bytes / n : 1));
	std::vector<uint64_t> rel;
	for (size_t a = 0; a < n; a += W) {                                // windows of about 64 MiB of records, as the sorted file's merge hands them on
		const size_t b = (size_t)std::min<uint64_t>(n, a + W), m = b - a;
		const uint64_t bytes = off[b] - off[a];
		rel.resize(m + 1);
		for (size_t j = 0; j <= m; ++j) rel[j] = off[a + j] - off[a];
		RCK(in.need((size_t)bytes + 16)); RCK(in_off.need(m + 1));
		HIPCK(hipMemcpyAsync(in.p, recs + off[a], (size_t)bytes, hipMemcpyHostToDevice, st));
		HIPCK(hipMemcpyAsync(in_off.p, rel.data(), 8 * (m + 1), hipMemcpyHostToDevice, st));
		RCK(bst_window_device(&d, in.p, in_off.p, (uint32_t)m, stream, nullptr));
		HIPCK(hipStreamSynchronize(st));
		RCK(bst_window_ms(&d, nullptr, fn));
	}
	RCK(bst_finish_device(&d, stream, R, fn));
	return bst_export(P, R, out, fn);
}
