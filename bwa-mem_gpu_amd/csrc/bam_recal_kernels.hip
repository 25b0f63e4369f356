// The covariate table of base quality score recalibration over the sorted file's windows on the device (csrc/bam_recal_core.h's rules).  A
// window's records are in their final order and carry their final flags when this runs (csrc/bam_sort_kernels.hip, behind the flag step, beside the coverage and
// the statistics steps).
//
//   count    one kernel, blocks of 256 lanes that take BRC_BLOCK_RECS records each, BRC_LANES lanes to a record: lane 0 of a group decides the record
//            (brc_prep: counted, left out, refused) and leaves what the others need in LDS; then the group's lanes stride over the kept bases, every lane with
//            its own cursor into the operations (brc_cur_seek only moves forward), and brc_base gives what a base adds
//   tables   the observations -- four increments a base -- go to 32-bit counters in LDS.  A block keeps BRC_SLOTS slots, each the cycle row (magnitudes up to
//            BRC_LDS_CYC, both signs) and the context row of one key: (group, quality) for event M, (group, 94) for I and D, which see the same bases and are
//            counted once.  A key finds its slot by open addressing over the slot keys (atomicCAS); a lane remembers the slot of the key it used last.  What
//            finds no slot -- a key beyond the slots, a cycle beyond the row, a record of more than BRC_LDS_BASES kept bases, whose counts a 32-bit word
//            might not hold -- goes to the accumulator in global memory with 64-bit atomics.  Errors are rare and always go there
//   flush    every word of the block's slots that is not empty: one 64-bit atomicAdd.  Integer sums do not depend on the order of arrival, so the words equal
//            the host form's exactly
//   refused  the smallest index << 4 | code of a window through a 64-bit atomicMin; the word travels to pinned host memory behind the kernel and is read behind
//            the window's own wait (brc_window_ms), before the window's members reach the sink
// Nothing passes between windows but the accumulator and the number of records seen; the accumulator is read once, at the end of the run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "bam_recal.h"
#include "bam_stats.h"
#include "devmem.h"

enum { BRC_LANES = 16, BRC_BLOCK = 256, BRC_GROUPS = BRC_BLOCK / BRC_LANES, BRC_BLOCK_RECS = 512, BRC_SLOTS = 48, BRC_LDS_CYC = 160, BRC_SLOT_WORDS = 2 * BRC_LDS_CYC + BRC_ICTX,
       BRC_LDS_BASES = 1 << 16, BRC_NO_KEY = 0xffffffff };

struct brc_dev_t {
	brc_plan_t P; brc_ref_t F;
	dev_buf<uint64_t> acc, err, coff, mask;
	dev_buf<int32_t> clen; dev_buf<uint32_t> rg_off; dev_buf<char> rg; dev_buf<uint8_t> pac;
	pin_buf<uint64_t> h_err;
	uint64_t n_seen = 0, masked = 0;
	hipEvent_t evt[2] = {nullptr, nullptr};
	bool timing = false, pending = false;                              // timing: evt[1] is recorded and not read yet; pending: a window's refusal word is not read yet
	~brc_dev_t() { for (hipEvent_t e : evt) if (e) (void)hipEventDestroy(e); }
};

namespace {

// the slot of `key` among the block's, claimed if it has none yet; -1: every slot holds another key
__device__ inline int brc_slot(uint32_t *keys, uint32_t key)
{
	const uint32_t h = ((key & 0xffu) + 7u * (key >> 8)) % (uint32_t)BRC_SLOTS;
	for (uint32_t p = 0; p < (uint32_t)BRC_SLOTS; ++p) {
		const uint32_t e = h + p < (uint32_t)BRC_SLOTS ? h + p : h + p - (uint32_t)BRC_SLOTS;
		uint32_t k = ((volatile uint32_t *)keys)[e];
		if (k == (uint32_t)BRC_NO_KEY) k = atomicCAS(&keys[e], (uint32_t)BRC_NO_KEY, key);
		if (k == key || k == (uint32_t)BRC_NO_KEY) return (int)e;
	}
	return -1;
}

// the cycle slot ci of a run at max_cycle C -> its place in a slot's cycle row, or -1 (a magnitude beyond BRC_LDS_CYC); and back
__device__ inline int brc_lds_cycle(uint32_t ci, uint32_t C)
{
	const uint32_t mag = ci >= C ? ci - C + 1 : C - ci;
	if (mag > (uint32_t)BRC_LDS_CYC) return -1;
	return ci >= C ? (int)((uint32_t)BRC_LDS_CYC + mag - 1) : (int)((uint32_t)BRC_LDS_CYC - mag);
}
__device__ inline uint32_t brc_run_cycle(uint32_t l, uint32_t C)
{
	return l >= (uint32_t)BRC_LDS_CYC ? C + (l - (uint32_t)BRC_LDS_CYC) : C - ((uint32_t)BRC_LDS_CYC - l);
}

__global__ void __launch_bounds__(BRC_BLOCK) brc_count(const uint8_t *__restrict__ recs, const uint64_t *__restrict__ soff, uint32_t n, brc_plan_t P, brc_ref_t F, uint64_t rec_base,
                                                       unsigned long long *acc, unsigned long long *err)
{
	__shared__ uint32_t tab[BRC_SLOTS * BRC_SLOT_WORDS];
	__shared__ uint32_t keys[BRC_SLOTS];
	__shared__ uint32_t sw[BRC_N_SUM];
	__shared__ brc_rec_t rr[BRC_GROUPS];
	__shared__ int rst[BRC_GROUPS];
	const uint32_t tid = threadIdx.x, grp = tid / BRC_LANES, lane = tid % BRC_LANES;
	for (uint32_t k = tid; k < (uint32_t)(BRC_SLOTS * BRC_SLOT_WORDS); k += BRC_BLOCK) tab[k] = 0;
	if (tid < (uint32_t)BRC_SLOTS) keys[tid] = (uint32_t)BRC_NO_KEY;
	if (tid < (uint32_t)BRC_N_SUM) sw[tid] = 0;
	__syncthreads();
	const uint32_t C = (uint32_t)P.max_cycle;
	for (uint32_t it = 0; it < (uint32_t)(BRC_BLOCK_RECS / BRC_GROUPS); ++it) {        // (the same count for every lane: the barriers below are the block's)
		const uint64_t j = (uint64_t)blockIdx.x * BRC_BLOCK_RECS + (uint64_t)it * BRC_GROUPS + grp;
		if (lane == 0) {
			int st = -1;
			if (j < n) {
				const uint64_t a = soff[j], b = soff[j + 1];
				st = b >= a ? brc_prep(recs + a, b - a, P, F, rr[grp]) : (int)BRC_E_CUT;
				atomicAdd(&sw[BRC_SEEN], 1u);
				if (st >= BRC_FILTERED) atomicAdd(&sw[BRC_F_REF + (st - BRC_FILTERED)], 1u);
				else if (st != BRC_OK) atomicMin(err, (unsigned long long)brc_refusal(rec_base + j, st));
				else {
					atomicAdd(&sw[BRC_COUNTED], 1u);
					if (rr[grp].n <= (uint32_t)BRC_LDS_BASES) atomicAdd(&sw[BRC_KEPT], rr[grp].n); else atomicAdd(acc + BRC_KEPT, (unsigned long long)rr[grp].n);
				}
			}
			rst[grp] = st;
		}
		__syncthreads();
		if (rst[grp] == BRC_OK) {
			const brc_rec_t r = rr[grp];
			const uint8_t *rec = recs + soff[j];
			const bool local = r.n <= (uint32_t)BRC_LDS_BASES;
			const int ids = local ? brc_slot(keys, r.group << 8 | (uint32_t)BRC_NQ) : -1;
			uint32_t last_key = (uint32_t)BRC_NO_KEY; int ms = -1;
			brc_cur_t cur; brc_cur_begin(cur);
			for (uint64_t i = (uint64_t)r.s0 + lane; i < (uint64_t)r.s0 + r.n; i += BRC_LANES) {
				brc_obs_t o;
				brc_cur_seek(rec, r, i, cur);
				const int sk = brc_base(rec, r, P, F, i, cur, o);
				if (sk) { if (local) atomicAdd(&sw[BRC_SK_BASE + sk - 1], 1u); else atomicAdd(acc + (BRC_SK_BASE + sk - 1), 1ull); continue; }
				if (o.capped) { if (local) atomicAdd(&sw[BRC_CAPPED], 1u); else atomicAdd(acc + BRC_CAPPED, 1ull); }
				const uint32_t key = r.group << 8 | o.q;
				if (local && key != last_key) { ms = brc_slot(keys, key); last_key = key; }
				const int lc = brc_lds_cycle(o.ci, C);
				if (ms >= 0 && lc >= 0) atomicAdd(&tab[ms * BRC_SLOT_WORDS + lc], 1u); else atomicAdd(acc + P.at_cy_m(r.group, o.q, o.ci), 1ull);
				if (ms >= 0) atomicAdd(&tab[ms * BRC_SLOT_WORDS + 2 * BRC_LDS_CYC + o.mctx], 1u); else atomicAdd(acc + P.at_cx_m(r.group, o.q, o.mctx), 1ull);
				if (ids >= 0 && lc >= 0) atomicAdd(&tab[ids * BRC_SLOT_WORDS + lc], 1u); else atomicAdd(acc + P.at_cy_id(r.group, o.ci), 1ull);
				if (ids >= 0) atomicAdd(&tab[ids * BRC_SLOT_WORDS + 2 * BRC_LDS_CYC + o.ictx], 1u); else atomicAdd(acc + P.at_cx_id(r.group, o.ictx), 1ull);
				if (o.snp) { atomicAdd(acc + P.at_cy_m(r.group, o.q, o.ci) + 1, 1ull); atomicAdd(acc + P.at_cx_m(r.group, o.q, o.mctx) + 1, 1ull); }
				if (o.ins) { atomicAdd(acc + P.at_cy_id(r.group, o.ci) + 1, 1ull); atomicAdd(acc + P.at_cx_id(r.group, o.ictx) + 1, 1ull); }
				if (o.del) { atomicAdd(acc + P.at_cy_id(r.group, o.ci) + 2, 1ull); atomicAdd(acc + P.at_cx_id(r.group, o.ictx) + 2, 1ull); }
			}
		}
		__syncthreads();                                                   // (rr and rst are written again; and, behind the last record, the flush reads the slots)
	}
	if (tid < (uint32_t)BRC_N_SUM && sw[tid]) atomicAdd(acc + tid, (unsigned long long)sw[tid]);
	for (uint32_t k = tid; k < (uint32_t)(BRC_SLOTS * BRC_SLOT_WORDS); k += BRC_BLOCK) {
		const uint32_t v = tab[k];
		if (!v) continue;
		const uint32_t s = k / (uint32_t)BRC_SLOT_WORDS, l = k % (uint32_t)BRC_SLOT_WORDS, key = keys[s], g = key >> 8, q = key & 0xffu;
		uint64_t at;
		if (l < 2u * BRC_LDS_CYC) { const uint32_t ci = brc_run_cycle(l, C); at = q == (uint32_t)BRC_NQ ? P.at_cy_id(g, ci) : P.at_cy_m(g, q, ci); }
		else { const uint32_t c = l - 2u * BRC_LDS_CYC; at = q == (uint32_t)BRC_NQ ? P.at_cx_id(g, c) : P.at_cx_m(g, q, c); }
		atomicAdd(acc + at, (unsigned long long)v);
	}
}

}   // namespace

brc_dev_t *brc_dev_create(void) { return new brc_dev_t(); }
void brc_dev_free(brc_dev_t *d) { delete d; }

extern "C" void bmh_recal_kernel_limits(uint32_t out[5])
{
	out[0] = BRC_SLOTS; out[1] = BRC_LANES; out[2] = BRC_LDS_CYC; out[3] = BRC_BLOCK_RECS; out[4] = BRC_LDS_BASES;
}

int brc_begin_device(brc_dev_t *d, const brc_run_t &U, const uint8_t *d_pac, void *stream)
{
	hipStream_t st = (hipStream_t)stream;
	const brc_plan_t &P = U.P;
	d->P = P; d->n_seen = 0; d->masked = U.masked; d->timing = d->pending = false;
	const size_t nc = (size_t)P.n_contigs + 1, mw = (size_t)((U.l_pac + 63) / 64);
	RCK(d->acc.need((size_t)P.words())); RCK(d->err.need(1)); RCK(d->h_err.need(1));
	RCK(d->coff.need(nc)); RCK(d->clen.need(nc)); RCK(d->rg.need(U.rg.size() + 1)); RCK(d->rg_off.need(U.rg_off.size()));
	HIPCK(hipMemsetAsync(d->acc.p, 0, 8 * (size_t)P.words(), st));
	HIPCK(hipMemsetAsync(d->err.p, 0xff, 8, st));                                      // (no record refused)
	d->h_err.p[0] = ~0ull;
	// (the run's vectors outlive the copies: the stream is waited for below)
	HIPCK(hipMemcpyAsync(d->coff.p, U.coff.data(), 8 * nc, hipMemcpyHostToDevice, st));
	HIPCK(hipMemcpyAsync(d->clen.p, U.clen.data(), 4 * nc, hipMemcpyHostToDevice, st));
	HIPCK(hipMemcpyAsync(d->rg.p, U.rg.data(), U.rg.size(), hipMemcpyHostToDevice, st));
	HIPCK(hipMemcpyAsync(d->rg_off.p, U.rg_off.data(), 4 * U.rg_off.size(), hipMemcpyHostToDevice, st));
	const uint64_t *d_mask = nullptr;
	if (U.mask) {
		RCK(d->mask.need(mw + 1));
		HIPCK(hipMemcpyAsync(d->mask.p, U.mask, 8 * mw, hipMemcpyHostToDevice, st));
		d_mask = d->mask.p;
	}
	if (!d_pac) {
		RCK(d->pac.need((size_t)(U.l_pac / 4 + 1) + 16));
		if (U.l_pac) HIPCK(hipMemcpyAsync(d->pac.p, U.pac, (size_t)((U.l_pac + 3) / 4), hipMemcpyHostToDevice, st));
		d_pac = d->pac.p;
	}
	HIPCK(hipStreamSynchronize(st));
	d->F = brc_ref_t{d_pac, d_mask, d->coff.p, d->clen.p, d->rg.p, d->rg_off.p};
	return BMH_OK;
}

int brc_window_device(brc_dev_t *d, const uint8_t *d_recs, const uint64_t *d_soff, uint32_t n, void *stream, double *ms)
{
	hipStream_t st = (hipStream_t)stream;
	if (!n) return BMH_OK;
	if (ms) { for (hipEvent_t &e : d->evt) if (!e) HIPCK(hipEventCreate(&e)); HIPCK(hipEventRecord(d->evt[0], st)); }
	brc_count<<<(uint32_t)(((uint64_t)n + BRC_BLOCK_RECS - 1) / BRC_BLOCK_RECS), BRC_BLOCK, 0, st>>>(d_recs, d_soff, n, d->P, d->F, d->n_seen, (unsigned long long *)d->acc.p, (unsigned long long *)d->err.p);
	HIPCK(hipGetLastError());
	if (ms) { HIPCK(hipEventRecord(d->evt[1], st)); d->timing = true; }
	HIPCK(hipMemcpyAsync(d->h_err.p, d->err.p, 8, hipMemcpyDeviceToHost, st));
	d->n_seen += n; d->pending = true;
	return BMH_OK;
}

int brc_window_ms(brc_dev_t *d, double *ms, const char *fn)
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
		if (e != ~0ull) return brc_refused(e >> 4, (int)(e & 15u), fn);
	}
	return BMH_OK;
}

int brc_finish_device(brc_dev_t *d, void *stream, brc_result_t &R, const char *fn)
{
	hipStream_t st = (hipStream_t)stream;
	const brc_plan_t &P = d->P;
	R.w.assign((size_t)P.words(), 0);
	HIPCK(hipMemcpyAsync(R.w.data(), d->acc.p, 8 * (size_t)P.words(), hipMemcpyDeviceToHost, st));
	HIPCK(hipStreamSynchronize(st));
	HIPCK(hipGetLastError());
	RCK(brc_window_ms(d, nullptr, fn));                                // (a window whose word nobody has read yet)
	R.w[BRC_MASKED] = d->masked;
	return BMH_OK;
}

extern "C" int bmh_bam_recal_device(const uint8_t *recs, uint64_t n_bytes, int n_contigs, const int32_t *contig_len, const bmh_recal_opt_t *opt, void *stream, bmh_recal_t *out)
{
	const char *fn = "bmh_bam_recal_device";
	hipStream_t st = (hipStream_t)stream;
	if (!out || (n_bytes && !recs)) { bmh_set_error("%s: null argument", fn); return BMH_EINVAL; }
	memset(out, 0, BRC_RECAL_OLD_BYTES);
	brc_run_t U;
	RCK(brc_run_from_opt(U, opt, n_contigs, contig_len, true, fn));
	std::vector<uint64_t> off;
	RCK(bst_walk(recs, n_bytes, off, fn));
	const size_t n = off.size() - 1;
	brc_dev_t d; brc_result_t R;
	RCK(brc_begin_device(&d, U, nullptr, stream));
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
		RCK(brc_window_device(&d, in.p, in_off.p, (uint32_t)m, stream, nullptr));
		HIPCK(hipStreamSynchronize(st));
		RCK(brc_window_ms(&d, nullptr, fn));
	}
	RCK(brc_finish_device(&d, stream, R, fn));
	return brc_export(&U, &R, out, fn);
}
