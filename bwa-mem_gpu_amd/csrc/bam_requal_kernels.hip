// Applying a recalibration table to the base qualities of the sorted file's windows on the device (csrc/bam_requal_core.h's rules).  A window's
// records are in their final order and carry their final flags when this runs (csrc/bam_sort_kernels.hip: behind the flag step, in front of the coverage, the
// statistics, the counting of a table and the compressor, which all read the qualities as written).
//
//   apply    one kernel, blocks of 256 lanes that take BRQ_BLOCK_RECS records each, BRQ_LANES lanes to a record: lane 0 of a group decides the record (brq_prep:
//            rewritten, without qualities, refused) and leaves what the others need in LDS; then the group's lanes stride over the stored bases.  A base costs
//            its quality byte, its own nibble and its neighbour's, three int16 loads from the (group, quality) row and, where the quality changes, one byte
//            store.  Only bytes are stored: records lie back to back at every alignment, and a byte store cannot touch a neighbour's field
//   counts   every lane keeps its counts in registers and the two histogram bins it met last with their run lengths; a run ends in one 32-bit LDS atomic, a
//            record in one per count that is not 0.  A record of more than BRQ_LDS_BASES bases, whose counts 32-bit words might not hold, ends its runs in 64-bit
//            atomics on the accumulator instead.  There is no atomic per base
//   flush    every word of the block that is not empty: one 64-bit atomicAdd.  Integer sums do not depend on the order of arrival: the words equal the host's
//   refused  the smallest index << 4 | code of a window through a 64-bit atomicMin; the word travels to pinned host memory behind the kernel and is read behind
//            the window's own wait (brq_window_ms), before the window's members reach the sink
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "bam_recal.h"
#include "bam_stats.h"
#include "devmem.h"

enum { BRQ_LANES = 16, BRQ_BLOCK = 256, BRQ_GROUPS = BRQ_BLOCK / BRQ_LANES, BRQ_BLOCK_RECS = 512, BRQ_LDS_BASES = 1 << 16 };

struct brq_dev_t {
	brq_plan_t P; brq_tab_t T;
	dev_buf<int16_t> tab; dev_buf<uint64_t> acc, err; dev_buf<uint32_t> rg_off; dev_buf<char> rg;
	pin_buf<uint64_t> h_err;
	uint64_t n_seen = 0;
	hipEvent_t evt[2] = {nullptr, nullptr};
	bool timing = false, pending = false;
	~brq_dev_t() { for (hipEvent_t e : evt) if (e) (void)hipEventDestroy(e); }
};

namespace {

// a histogram bin's run of a lane (at most 2^28 entries: a lane's share of a record); the run of another bin goes out first
struct brq_run_of_t { uint32_t bin, n; };
__device__ inline void brq_run_end(brq_run_of_t &r, uint32_t *hist, unsigned long long *acc_hist, bool local)
{
	if (!r.n) return;
	if (local) atomicAdd(&hist[r.bin], r.n); else atomicAdd(acc_hist + r.bin, (unsigned long long)r.n);
	r.n = 0;
}
__device__ inline void brq_run_add(brq_run_of_t &r, uint32_t bin, uint32_t *hist, unsigned long long *acc_hist, bool local)
{
	if (r.n && r.bin != bin) brq_run_end(r, hist, acc_hist, local);
	r.bin = bin; ++r.n;
}

__global__ void __launch_bounds__(BRQ_BLOCK) brq_apply(uint8_t *recs, const uint64_t *__restrict__ soff, uint32_t n, brq_plan_t P, brq_tab_t T, uint64_t rec_base,
                                                       unsigned long long *acc, unsigned long long *err)
{
	__shared__ uint32_t sw[BRQ_N_SUM];
	__shared__ uint32_t hist[BRQ_HIST];
	__shared__ brq_rec_t rr[BRQ_GROUPS];
	__shared__ int rst[BRQ_GROUPS];
	const uint32_t tid = threadIdx.x, grp = tid / BRQ_LANES, lane = tid % BRQ_LANES;
	if (tid < (uint32_t)BRQ_N_SUM) sw[tid] = 0;
	if (tid < (uint32_t)BRQ_HIST) hist[tid] = 0;
	__syncthreads();
	for (uint32_t it = 0; it < (uint32_t)(BRQ_BLOCK_RECS / BRQ_GROUPS); ++it) {        // (the same count for every lane: the barriers below are the block's)
		const uint64_t j = (uint64_t)blockIdx.x * BRQ_BLOCK_RECS + (uint64_t)it * BRQ_GROUPS + grp;
		if (lane == 0) {
			int st = -1;
			if (j < n) {
				const uint64_t a = soff[j], b = soff[j + 1];
				st = b >= a ? brq_prep(recs + a, b - a, P, T, rr[grp]) : (int)BRC_E_CUT;
				atomicAdd(&sw[BRQ_SEEN], 1u);
				if (st == BRQ_SKIP) atomicAdd(&sw[BRQ_NOQUAL], 1u);
				else if (st != BRC_OK) atomicMin(err, (unsigned long long)brc_refusal(rec_base + j, st));
				else {
					atomicAdd(&sw[BRQ_REWRITTEN], 1u);
					if (rr[grp].l_seq <= (uint32_t)BRQ_LDS_BASES) atomicAdd(&sw[BRQ_BASES], rr[grp].l_seq); else atomicAdd(acc + BRQ_BASES, (unsigned long long)rr[grp].l_seq);
				}
			}
			rst[grp] = st;
		}
		__syncthreads();
		if (rst[grp] == BRC_OK) {
			const brq_rec_t r = rr[grp];
			uint8_t *rec = recs + soff[j];
			const bool local = r.l_seq <= (uint32_t)BRQ_LDS_BASES;
			uint32_t low = 0, changed = 0, same = 0, capped = 0, noctx = 0;      // (a lane sees at most 2^32 / 16 bases of a record)
			brq_run_of_t before = {0, 0}, after = {0, 0};
			for (uint64_t i = lane; i < r.l_seq; i += BRQ_LANES) {
				brq_obs_t o;
				const uint32_t q0 = rec[r.qual_at + i], q1 = brq_base(rec, r, P, T.t, i, q0, o);
				brq_run_add(before, q0 < (uint32_t)BRQ_MAX_Q ? q0 : (uint32_t)BRQ_MAX_Q, hist, acc + BRQ_N_SUM, local);
				brq_run_add(after, q1 < (uint32_t)BRQ_MAX_Q ? q1 : (uint32_t)BRQ_MAX_Q, hist + BRC_NQ, acc + BRQ_N_SUM + BRC_NQ, local);
				if (o.low) { ++low; continue; }
				capped += o.capped; noctx += o.noctx;
				if (q1 != q0) { ++changed; rec[r.qual_at + i] = (uint8_t)q1; } else ++same;      // (a byte store, inside the record's own qualities: i < l_seq)
			}
			brq_run_end(before, hist, acc + BRQ_N_SUM, local); brq_run_end(after, hist + BRC_NQ, acc + BRQ_N_SUM + BRC_NQ, local);
			const uint32_t v[5] = {low, changed, same, capped, noctx};
			for (int k = 0; k < 5; ++k)
				if (v[k]) { if (local) atomicAdd(&sw[BRQ_LOW + k], v[k]); else atomicAdd(acc + (BRQ_LOW + k), (unsigned long long)v[k]); }
		}
		__syncthreads();                                                   // (rr and rst are written again; and, behind the last record, the flush reads the counts)
	}
	if (tid < (uint32_t)BRQ_N_SUM && sw[tid]) atomicAdd(acc + tid, (unsigned long long)sw[tid]);
	if (tid < (uint32_t)BRQ_HIST && hist[tid]) atomicAdd(acc + BRQ_N_SUM + tid, (unsigned long long)hist[tid]);
}

}   // namespace

brq_dev_t *brq_dev_create(void) { return new brq_dev_t(); }
void brq_dev_free(brq_dev_t *d) { delete d; }

extern "C" void bmh_requal_kernel_limits(uint32_t out[3])
{
	out[0] = BRQ_LANES; out[1] = BRQ_BLOCK_RECS; out[2] = BRQ_LDS_BASES;
}

int brq_begin_device(brq_dev_t *d, const brq_run_t &U, void *stream)
{
	hipStream_t st = (hipStream_t)stream;
	d->P = U.P; d->n_seen = 0; d->timing = d->pending = false;
	RCK(d->tab.need(U.t.size() + 8)); RCK(d->acc.need((size_t)BRQ_WORDS)); RCK(d->err.need(1)); RCK(d->h_err.need(1));
	RCK(d->rg.need(U.rg.size() + 1)); RCK(d->rg_off.need(U.rg_off.size()));
	HIPCK(hipMemsetAsync(d->acc.p, 0, 8 * (size_t)BRQ_WORDS, st));
	HIPCK(hipMemsetAsync(d->err.p, 0xff, 8, st));                                      // (no record refused)
	d->h_err.p[0] = ~0ull;
	// (the run's vectors outlive the copies: the stream is waited for below)
	HIPCK(hipMemcpyAsync(d->tab.p, U.t.data(), 2 * U.t.size(), hipMemcpyHostToDevice, st));
	HIPCK(hipMemcpyAsync(d->rg.p, U.rg.data(), U.rg.size(), hipMemcpyHostToDevice, st));
	HIPCK(hipMemcpyAsync(d->rg_off.p, U.rg_off.data(), 4 * U.rg_off.size(), hipMemcpyHostToDevice, st));
	HIPCK(hipStreamSynchronize(st));
	d->T = brq_tab_t{d->tab.p, d->rg.p, d->rg_off.p};
	return BMH_OK;
}

int brq_window_device(brq_dev_t *d, uint8_t *d_recs, const uint64_t *d_soff, uint32_t n, void *stream, double *ms)
{
	hipStream_t st = (hipStream_t)stream;
	if (!n) return BMH_OK;
	if (ms) { for (hipEvent_t &e : d->evt) if (!e) HIPCK(hipEventCreate(&e)); HIPCK(hipEventRecord(d->evt[0], st)); }
	brq_apply<<<(uint32_t)(((uint64_t)n + BRQ_BLOCK_RECS - 1) / BRQ_BLOCK_RECS), BRQ_BLOCK, 0, st>>>(d_recs, d_soff, n, d->P, d->T, d->n_seen, (unsigned long long *)d->acc.p, (unsigned long long *)d->err.p);
	HIPCK(hipGetLastError());
	if (ms) { HIPCK(hipEventRecord(d->evt[1], st)); d->timing = true; }
	HIPCK(hipMemcpyAsync(d->h_err.p, d->err.p, 8, hipMemcpyDeviceToHost, st));
	d->n_seen += n; d->pending = true;
	return BMH_OK;
}

int brq_window_ms(brq_dev_t *d, double *ms, const char *fn)
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
		if (e != ~0ull) return brq_refused(e >> 4, (int)(e & 15u), fn);
	}
	return BMH_OK;
}

int brq_finish_device(brq_dev_t *d, void *stream, brq_result_t &R, const char *fn)
{
	hipStream_t st = (hipStream_t)stream;
	R.w.assign((size_t)BRQ_WORDS, 0);
	HIPCK(hipMemcpyAsync(R.w.data(), d->acc.p, 8 * (size_t)BRQ_WORDS, hipMemcpyDeviceToHost, st));
	HIPCK(hipStreamSynchronize(st));
	HIPCK(hipGetLastError());
	RCK(brq_window_ms(d, nullptr, fn));                                // (a window whose word nobody has read yet)
	return BMH_OK;
}

extern "C" int bmh_bam_requal_device(const uint8_t *recs, uint64_t n_bytes, const bmh_recal_apply_opt_t *apply, void *stream, uint8_t **out, bmh_recal_t *counts)
{
	const char *fn = "bmh_bam_requal_device";
	hipStream_t st = (hipStream_t)stream;
	if (out) *out = nullptr;
	if (!out || !counts || (n_bytes && !recs)) { bmh_set_error("%s: null argument", fn); return BMH_EINVAL; }
	memset(counts, 0, sizeof *counts);
	brq_run_t U;
	RCK(brq_run_from_opt(U, apply, fn));
	std::vector<uint64_t> off;
	RCK(bst_walk(recs, n_bytes, off, fn));
	const size_t n = off.size() - 1;
	struct own_t { uint8_t *p = nullptr; ~own_t() { free(p); } } res;
	if (!(res.p = (uint8_t *)malloc((size_t)n_bytes + 1))) { bmh_set_error("%s: out of memory", fn); return BMH_ENOMEM; }
	brq_dev_t d; brq_result_t R;
	RCK(brq_begin_device(&d, U, stream));
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
		RCK(brq_window_device(&d, in.p, in_off.p, (uint32_t)m, stream, nullptr));
		HIPCK(hipMemcpyAsync(res.p + off[a], in.p, (size_t)bytes, hipMemcpyDeviceToHost, st));
		HIPCK(hipStreamSynchronize(st));
		RCK(brq_window_ms(&d, nullptr, fn));
	}
	RCK(brq_finish_device(&d, stream, R, fn));
	RCK(brc_export(nullptr, nullptr, counts, fn, &R));
	*out = res.p; res.p = nullptr;
	return BMH_OK;
}
