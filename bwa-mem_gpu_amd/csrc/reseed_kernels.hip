// BWA-MEM's second and third seeding rounds on gfx950 (mem_collect_intv with re_seed, src/bwamem.c:266-297), wave64.
//
// Input: the first round's SMEMs as bmh_seed_batch leaves them in HBM after its filter (res_a / res_k / occ, kept = occ != 0, in
// (read, end) order; occ_off = the scan that counts the kept ones in its high bits).  Output: the groups of all three rounds merged per
// read by info = begin << 32 | end (ks_introsort(mem_intv) -- equal keys are the same substring, hence the same interval: their order
// does not matter, their number does), with occurrence counts, offsets and per-read sums; expand / locate of seed_kernels.hip then
// write the bmh_seeds_t columns from them exactly as they do for the first round alone.
//
//   select   scan over the first round's results: length >= split_len, occurrences <= split_width -> one task
//            {read, (begin + end) >> 1, min_intv = occurrences + 1} (compacted by the scan's offsets)
//   round 2  one lane per task: bwt_smem1a(x, min_intv, max_intv = 0) (src/bwt.c:483-556), one rank pair per loop iteration so the
//            lanes stay convergent on the gathers.  The forward list lives in a private HBM column of RESEED_CAP entries (a knob,
//            32) and the backward rounds compact it in place (curr is prev minus some entries, in the same order); the SMEMs go to
//            a second column (never more of them than forward entries).  A task whose forward list does not fit is listed and run
//            again in a second launch whose columns hold max_len + 1 entries (the forward list has at most len - x), so nothing is
//            cut short.  A lane walks its task alone, as the reference does: a 65 535-base homopolymer read is one task of some
//            5e8 sequential rank steps, so the case table (tests/reseed_cases.py) keeps every task below 100 000 of them.
//   round 3  one lane per read: the sequential bwt_seed_strategy1 scan (src/bwt.c:568-590) with its N handling, one forward extension
//            per iteration; the seeds are at least min_seed_len + 1 long and disjoint, so a read has at most len / (k + 1) of them:
//            a per-read column of that size, placed by a scan of the lengths.  Lanes of equal-length reads run equal iteration counts
//            (every base is extended once); an empty interval is carried without rank queries, as its size stays 0.
//   merge    the three rounds' groups -> keys (read << 32 | begin << 16 | end) + radix sort -> res / occ columns, per-read sums
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "bmh_internal.h"
#include "devmem.h"
#include "fmd_dev.h"
#include "seed_dev.h"

struct rs_task_t { uint32_t read, x, m, pad; };

// list entry: k (48 bits), end (16 bits), s (64 bits)
__device__ __forceinline__ uint4 rs_pack(uint64_t k, uint64_t s, int end)
{
	return make_uint4((uint32_t)k, (uint32_t)(k >> 32) | ((uint32_t)end << 16), (uint32_t)s, (uint32_t)(s >> 32));
}

// sum of v over the wave; lane 0 adds it to *ctr
__device__ __forceinline__ void rs_wave_add(unsigned long long *ctr, uint32_t v)
{
	unsigned long long t = v;
	for (int off = 32; off; off >>= 1) t += __shfl_down(t, off);
	if (__lane_id() == 0 && t) atomicAdd(ctr, t);
}

// the selection flag of first-round result t (mem_collect_intv: end - start >= split_len and x[2] <= split_width)
struct rs_flag_in {
	const res_t *res_a; const uint32_t *occ; uint64_t n; int split_len; int split_width;
	__device__ uint32_t operator()(uint64_t t) const
	{
		if (t >= n) return 0u;
		const uint32_t s = occ[t];
		if (!s) return 0u;
		const uint32_t be = res_a[t].be;
		const int len = (int)(be & 0xFFFFu) - (int)(be >> 16);
		return (len >= split_len && (int64_t)s <= (int64_t)split_width) ? 1u : 0u;
	}
};

// round-3 column size of a read: at most len / (k + 1) seeds
struct rs_bound_in {
	const uint32_t *lens; uint32_t n; int k;
	__device__ uint64_t operator()(uint64_t r) const { return r < n ? (uint64_t)(lens[r] / (uint32_t)(k + 1) + 1u) : 0ull; }
};

__global__ void __launch_bounds__(256) reseed_task_kernel(const res_t *__restrict__ res_a, const uint32_t *__restrict__ occ, uint64_t n,
                                                          int split_len, int split_width, const uint32_t *__restrict__ tsk_off, rs_task_t *__restrict__ tasks)
{
	const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= n) return;
	rs_flag_in fl = {res_a, occ, n, split_len, split_width};
	if (!fl(t)) return;
	const res_t e = res_a[t];
	rs_task_t o = {e.read, ((e.be >> 16) + (e.be & 0xFFFFu)) >> 1, occ[t] + 1u, 0u};
	tasks[tsk_off[t]] = o;
}

// ---------------------------------------------------------------- round 2: bwt_smem1a from the middle of a task's SMEM

enum { R2_FWD = 0, R2_BWD, R2_DONE };

__global__ void __launch_bounds__(256) reseed_r2_kernel(fmd_dev_t f, read_view_t rv, const uint32_t *__restrict__ lens, int min_seed_len,
                                                        const rs_task_t *__restrict__ tasks, const uint32_t *__restrict__ ids, uint32_t n, uint32_t cap,
                                                        uint4 *__restrict__ list, uint4 *__restrict__ out, uint32_t *__restrict__ n_out,
                                                        uint32_t *__restrict__ ovf_ids, unsigned long long *__restrict__ counters,
                                                        unsigned long long *__restrict__ n_steps)
{
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	const bool live = t < n;
	rs_task_t tk = {0, 0, 0, 0};
	const uint32_t tid = live ? (ids ? ids[t] : t) : 0u;
	if (live) tk = tasks[tid];
	const size_t base = (size_t)t * cap;
	const uint32_t r = tk.read;
	const int len = live ? (int)lens[r] : 0, x = (int)tk.x;
	const uint64_t m = tk.m;                 // min_intv
	int st = R2_DONE;
	uint64_t k = 0, l = 0, s = 0;
	int i = 0, end = 0, nl = 0;
	uint32_t steps = 0;                      // rank pairs of this lane (bmh_reseed_last_counts)
	bool ovf = false;
	if (live) {
		const int b = read_base(rv, r, x);
		if (b < 4) { k = fmd_L2(f, b) + 1; s = fmd_L2(f, b + 1) - fmd_L2(f, b); l = fmd_L2(f, 3 - b) + 1; end = x + 1; i = x + 1; st = R2_FWD; }
	}
	// backward rounds: position bi, its symbol c (-1: before the read or an N), the list's live part [lo, hi], the entry j being
	// extended, the write cursor w (>= j: curr is written over prev from the top), curr's length cn and last size
	int bi = 0, c = -1, lo = 0, hi = -1, j = -1, w = -1, cn = 0, last_beg = 0, nmem = 0, nout = 0;
	uint64_t last_s = 0;
	while (__any(st != R2_DONE)) {
		if (st == R2_FWD) {
			bool push = false, stop = false;
			uint64_t nk = 0, nlv = 0, ns = 0;
			if (i >= len) { push = true; stop = true; }                     // reached the end: push the last interval
			else {
				const int b = read_base(rv, r, i);
				if (b > 3) { push = true; stop = true; }                    // an ambiguous base ends the extension
				else {
					uint64_t ak[4], al[4], as[4];
					fmd_forward_ext(f, k, l, s, ak, al, as); ++steps;
					const int cb = 3 - b;
					ns = sel4(cb, as[0], as[1], as[2], as[3]); nk = sel4(cb, ak[0], ak[1], ak[2], ak[3]); nlv = sel4(cb, al[0], al[1], al[2], al[3]);
					if (ns != s) { push = true; stop = ns < m; }            // change of the interval size; too small to extend further
				}
			}
			if (push) {
				if ((uint32_t)nl == cap) { ovf = true; st = R2_DONE; }
				else list[base + nl++] = rs_pack(k, s, end);
			}
			if (st == R2_FWD) {
				if (!stop) { k = nk; l = nlv; s = ns; end = i + 1; ++i; }
				else {                                                       // longest match first: from the top of the list down
					bi = x - 1; lo = 0; hi = nl - 1; j = hi; w = hi; cn = 0;
					c = bi < 0 ? -1 : read_base(rv, r, bi); if (c > 3) c = -1;
					st = R2_BWD;
				}
			}
		} else if (st == R2_BWD) {
			if (j < lo) {                                                    // the round at bi is over
				if (cn == 0) st = R2_DONE;
				else {
					lo = w + 1; --bi; j = hi; w = hi; cn = 0;
					c = bi < 0 ? -1 : read_base(rv, r, bi); if (c > 3) c = -1;
				}
			}
			if (st == R2_BWD) {
				const uint4 e = list[base + j];
				const uint64_t pk = (uint64_t)e.x | ((uint64_t)(e.y & 0xFFFFu) << 32), ps = (uint64_t)e.z | ((uint64_t)e.w << 32);
				const int pend = (int)(e.y >> 16);
				uint64_t nk = 0, ns = 0;
				if (c >= 0) {
					uint64_t ol, ou;
					fmd_occ1_pair<false>(f, pk - 1, pk + ps - 1, c, ol, ou); ++steps;
					nk = fmd_L2(f, c) + ol + 1; ns = ou - ol;
				}
				if (c < 0 || ns < m) {                                       // keep the hit unless a longer one of this round is still growing
					if (cn == 0 && (nmem == 0 || bi + 1 < last_beg)) {       // ... and unless it is contained in the last one kept
						++nmem; last_beg = bi + 1;
						if (pend - (bi + 1) >= min_seed_len)
							out[base + nout++] = make_uint4(((uint32_t)(bi + 1) << 16) | (uint32_t)pend, (uint32_t)ps, (uint32_t)pk, (uint32_t)(pk >> 32));
					}
				} else if (cn == 0 || ns != last_s) {
					list[base + w] = rs_pack(nk, ns, pend); --w; ++cn; last_s = ns;
				}
				--j;
			}
		}
	}
	if (live) {
		if (ovf) { nout = 0; ovf_ids[atomicAdd((unsigned int *)(counters + 1), 1u)] = tid; }
		n_out[t] = (uint32_t)nout;
	}
	rs_wave_add(counters, (uint32_t)nout);
	rs_wave_add(n_steps, steps);
}

// ---------------------------------------------------------------- round 3: bwt_seed_strategy1 along the read

enum { R3_OPEN = 0, R3_EXT, R3_DONE };

__global__ void __launch_bounds__(256) reseed_r3_kernel(fmd_dev_t f, read_view_t rv, const uint32_t *__restrict__ lens, int min_seed_len, uint64_t max_intv,
                                                        const uint64_t *__restrict__ off3, uint4 *__restrict__ out, uint32_t *__restrict__ n_out,
                                                        unsigned long long *__restrict__ counter, unsigned long long *__restrict__ n_steps)
{
	const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
	const bool live = r < rv.n_reads;
	const int len = live ? (int)lens[r] : 0;
	const size_t base = live ? (size_t)off3[r] : 0;
	int st = live && len > 0 ? R3_OPEN : R3_DONE;
	int x = 0, i = 0, nout = 0;
	uint32_t steps = 0;
	uint64_t k = 0, l = 0, s = 0;
	while (__any(st != R3_DONE)) {
		if (st == R3_OPEN) {
			if (x >= len) st = R3_DONE;
			else {
				const int b = read_base(rv, r, x);
				if (b > 3) ++x;
				else { k = fmd_L2(f, b) + 1; s = fmd_L2(f, b + 1) - fmd_L2(f, b); l = fmd_L2(f, 3 - b) + 1; i = x + 1; st = R3_EXT; }
			}
		} else if (st == R3_EXT) {
			if (i >= len) { x = len; st = R3_DONE; }
			else {
				const int b = read_base(rv, r, i);
				if (b > 3) { x = i + 1; st = R3_OPEN; }
				else if (s == 0) {                                           // an empty interval stays empty: ok[c].x[2] == 0 < max_intv
					if (i - x >= min_seed_len) { x = i + 1; st = R3_OPEN; }  // (returned with m.x[2] == 0: not pushed)
					else ++i;
				} else {
					uint64_t ak[4], al[4], as[4];
					fmd_forward_ext(f, k, l, s, ak, al, as); ++steps;
					const int cb = 3 - b;
					const uint64_t ns = sel4(cb, as[0], as[1], as[2], as[3]), nk = sel4(cb, ak[0], ak[1], ak[2], ak[3]), nlv = sel4(cb, al[0], al[1], al[2], al[3]);
					if (ns < max_intv && i - x >= min_seed_len) {
						if (ns > 0) out[base + nout++] = make_uint4(((uint32_t)x << 16) | (uint32_t)(i + 1), (uint32_t)ns, (uint32_t)nk, (uint32_t)(nk >> 32));
						x = i + 1; st = R3_OPEN;
					} else { k = nk; l = nlv; s = ns; ++i; }
				}
			}
		}
	}
	if (live) n_out[r] = (uint32_t)nout;
	rs_wave_add(counter, (uint32_t)nout);
	rs_wave_add(n_steps, steps);
}

// ---------------------------------------------------------------- merge

__device__ __forceinline__ uint64_t rs_key(uint32_t read, uint32_t be) { return ((uint64_t)read << 32) | (uint64_t)be; }

// the first round's kept groups -> slots [0, n_kept) (their rank among the kept ones: the high bits of occ_off)
__global__ void __launch_bounds__(256) reseed_copy_r1_kernel(const res_t *__restrict__ res_a, const uint64_t *__restrict__ res_k, const uint32_t *__restrict__ occ,
                                                             const uint64_t *__restrict__ occ_off, uint64_t n, uint64_t *__restrict__ keys,
                                                             uint32_t *__restrict__ vals, uint64_t *__restrict__ mk, uint32_t *__restrict__ ms)
{
	const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= n) return;
	const uint32_t s = occ[t];
	if (!s) return;
	const uint64_t pos = occ_off[t] >> OCC_OFF_SHIFT;
	const res_t e = res_a[t];
	keys[pos] = rs_key(e.read, e.be); vals[pos] = (uint32_t)pos; mk[pos] = res_k[t]; ms[pos] = s;
}

// a round's groups (unit u: n_out[u] of them at out[off ? off[u] : u * cap]) -> the slots behind *cursor (one atomic per wave)
__global__ void __launch_bounds__(256) reseed_copy_out_kernel(const uint4 *__restrict__ out, const uint32_t *__restrict__ n_out, const uint64_t *__restrict__ off,
                                                              uint32_t cap, uint32_t n_units, const rs_task_t *__restrict__ tasks, const uint32_t *__restrict__ ids,
                                                              unsigned long long *__restrict__ cursor, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals,
                                                              uint64_t *__restrict__ mk, uint32_t *__restrict__ ms)
{
	const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
	const int lane = __lane_id();
	const bool live = u < n_units;
	const uint32_t cnt = live ? n_out[u] : 0u;
	uint32_t incl = cnt;
	for (int d = 1; d < 64; d <<= 1) { const uint32_t v = __shfl_up(incl, d); if (lane >= d) incl += v; }
	const uint32_t tot = __shfl(incl, 63);
	unsigned long long b0 = 0;
	if (lane == 0 && tot) b0 = atomicAdd(cursor, (unsigned long long)tot);
	b0 = __shfl(b0, 0);
	if (!cnt) return;
	const uint64_t pos = b0 + incl - cnt;
	const uint32_t read = tasks ? tasks[ids ? ids[u] : u].read : u;
	const size_t src = off ? (size_t)off[u] : (size_t)u * cap;
	for (uint32_t q = 0; q < cnt; ++q) {
		const uint4 e = out[src + q];
		keys[pos + q] = rs_key(read, e.x); vals[pos + q] = (uint32_t)(pos + q);
		mk[pos + q] = (uint64_t)e.z | ((uint64_t)e.w << 32); ms[pos + q] = e.y;
	}
}

__global__ void reseed_set_kernel(unsigned long long *p, unsigned long long v) { *p = v; }

// sorted keys -> the res / occ columns expand_kernel reads, occurrences per read
__global__ void __launch_bounds__(256) reseed_gather_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals, uint64_t n,
                                                            const uint64_t *__restrict__ mk, const uint32_t *__restrict__ ms, res_t *__restrict__ ra,
                                                            uint64_t *__restrict__ rk, uint32_t *__restrict__ rocc, uint32_t *__restrict__ n_ref_pos)
{
	const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (t > n) return;
	if (t == n) { rocc[n] = 0; return; }
	const uint64_t key = keys[t];
	const uint32_t src = vals[t], s = ms[src], read = (uint32_t)(key >> 32);
	res_t o = {read, (uint32_t)key, s, 0u};
	ra[t] = o; rk[t] = mk[src]; rocc[t] = s;
	atomicAdd(&n_ref_pos[read], s);
}

// ---------------------------------------------------------------- host side

struct reseed_state_t {
	dev_buf<uint8_t> tsk_off, tasks, list, out2, n2, ovf, list_b, out_b, n2b, off3, out3, n3, keys, keys2, vals, vals2, mk, ms, ra, rk, rocc, roff, tmp;
	dev_buf<unsigned long long> ctr;        // [0] round-2 groups [1] overflowing tasks [2] round-3 groups [3] groups of the second round-2 launch [4] merge cursor
	                                        // [5] rank steps of round 2, both launches [6] of round 3
};

void reseed_state_free(reseed_state_t *R) { delete R; }

// round-2 tasks, tasks that overflowed, groups of rounds 1, 2, 3, rank steps of rounds 2 and 3 of the thread's last bmh_seed_batch_reseed (tests: which
// path a batch took, and how much work it was)
static thread_local uint64_t g_rs_last[7] = {0, 0, 0, 0, 0, 0, 0};
void reseed_counts_reset(void) { memset(g_rs_last, 0, sizeof(g_rs_last)); }
extern "C" int bmh_reseed_last_counts(uint64_t *out)
{
	if (!out) { bmh_set_error("bmh_reseed_last_counts: null argument"); return BMH_EINVAL; }
	memcpy(out, g_rs_last, sizeof(g_rs_last));
	return BMH_OK;
}

static inline unsigned rs_nblk(uint64_t n) { return (unsigned)((n + 255) / 256); }

int reseed_merge(reseed_state_t **Rp, const reseed_in_t &in, hipStream_t st, reseed_out_t *out)
{
	if (!*Rp) {
		*Rp = new reseed_state_t();
		RCK((*Rp)->ctr.resize(8));
	}
	reseed_state_t &R = **Rp;
	memset(out, 0, sizeof(*out));
	const int k = in.min_seed_len;
	const int split_len = (int)(in.min_seed_len * in.opt.split_factor + .499);      // as mem_collect_intv: int * float + .499
	const uint64_t n_cands = in.n_cands, n_reads = in.n_reads;
	const bool r3 = in.opt.max_mem_intv > 0;
	// forward entries per round-2 task in the first launch (~17 on a 6 Gbase text; the rest runs again, larger).  No list is longer than max_len, so a
	// larger column holds nothing more
	const int cap_knob = bmh_tune("RESEED_CAP", 32);
	const uint32_t cap_a = cap_knob < 1 ? 1u : ((uint32_t)cap_knob > in.max_len + 1 ? in.max_len + 1 : (uint32_t)cap_knob);
	HIPCK(hipMemsetAsync(R.ctr.p, 0, 64, st));

	// ---- select the round-2 tasks (scan of the flags) and size the round-3 columns (scan of the bounds): one wait for both totals
	size_t tb = 0, t2 = 0;
	rs_flag_in fl = {in.res_a, in.occ, n_cands, split_len, in.opt.split_width};
	auto fit = rocprim::make_transform_iterator(rocprim::counting_iterator<uint64_t>(0), fl);
	rs_bound_in bd = {in.lens, in.n_reads, k};
	auto bit = rocprim::make_transform_iterator(rocprim::counting_iterator<uint64_t>(0), bd);
	HIPCK(rocprim::exclusive_scan(nullptr, tb, fit, (uint32_t *)nullptr, 0u, (size_t)n_cands + 1, rocprim::plus<uint32_t>(), st));
	HIPCK(rocprim::exclusive_scan(nullptr, t2, bit, (uint64_t *)nullptr, (uint64_t)0, (size_t)n_reads + 1, rocprim::plus<uint64_t>(), st));
	RCK(R.tmp.need(tb > t2 ? tb : t2));
	RCK(R.tsk_off.need(4 * (n_cands + 1)));
	RCK(R.off3.need(8 * (n_reads + 1)));
	tb = R.tmp.cap;
	HIPCK(rocprim::exclusive_scan(R.tmp.p, tb, fit, R.tsk_off.as<uint32_t>(), 0u, (size_t)n_cands + 1, rocprim::plus<uint32_t>(), st));
	if (r3) { tb = R.tmp.cap; HIPCK(rocprim::exclusive_scan(R.tmp.p, tb, bit, R.off3.as<uint64_t>(), (uint64_t)0, (size_t)n_reads + 1, rocprim::plus<uint64_t>(), st)); }
	uint32_t n_tasks = 0; uint64_t n_slots3 = 0;
	HIPCK(hipMemcpyAsync(&n_tasks, R.tsk_off.as<uint32_t>() + n_cands, 4, hipMemcpyDeviceToHost, st));
	if (r3) HIPCK(hipMemcpyAsync(&n_slots3, R.off3.as<uint64_t>() + n_reads, 8, hipMemcpyDeviceToHost, st));
	HIPCK(hipStreamSynchronize(st));

	// ---- round 2 (first launch) and round 3
	if (n_tasks) {
		RCK(R.tasks.need(sizeof(rs_task_t) * (size_t)n_tasks));
		RCK(R.list.need(16 * (size_t)n_tasks * cap_a)); RCK(R.out2.need(16 * (size_t)n_tasks * cap_a));
		RCK(R.n2.need(4 * (size_t)n_tasks)); RCK(R.ovf.need(4 * (size_t)n_tasks));
		reseed_task_kernel<<<rs_nblk(n_cands), 256, 0, st>>>(in.res_a, in.occ, n_cands, split_len, in.opt.split_width, R.tsk_off.as<uint32_t>(), R.tasks.as<rs_task_t>());
		reseed_r2_kernel<<<rs_nblk(n_tasks), 256, 0, st>>>(in.f, in.rv, in.lens, k, R.tasks.as<rs_task_t>(), nullptr, n_tasks, cap_a,
		                                                   R.list.as<uint4>(), R.out2.as<uint4>(), R.n2.as<uint32_t>(), R.ovf.as<uint32_t>(), R.ctr.p, R.ctr.p + 5);
	}
	if (r3) {
		RCK(R.out3.need(16 * (n_slots3 + 1))); RCK(R.n3.need(4 * (n_reads + 1)));
		reseed_r3_kernel<<<rs_nblk(n_reads), 256, 0, st>>>(in.f, in.rv, in.lens, k, (uint64_t)in.opt.max_mem_intv, R.off3.as<uint64_t>(),
		                                                   R.out3.as<uint4>(), R.n3.as<uint32_t>(), R.ctr.p + 2, R.ctr.p + 6);
	}
	unsigned long long c[7] = {0, 0, 0, 0, 0, 0, 0};
	HIPCK(hipMemcpyAsync(c, R.ctr.p, 56, hipMemcpyDeviceToHost, st));
	HIPCK(hipStreamSynchronize(st));
	// ---- the tasks whose forward list did not fit: again, with columns of max_len + 1 entries (the list holds at most len - x)
	const uint32_t n_ovf = (uint32_t)(c[1] & 0xFFFFFFFFull);
	const uint32_t cap_b = in.max_len + 1;
	if (n_ovf) {
		RCK(R.list_b.need(16 * (size_t)n_ovf * cap_b)); RCK(R.out_b.need(16 * (size_t)n_ovf * cap_b)); RCK(R.n2b.need(4 * (size_t)n_ovf));
		reseed_r2_kernel<<<rs_nblk(n_ovf), 256, 0, st>>>(in.f, in.rv, in.lens, k, R.tasks.as<rs_task_t>(), R.ovf.as<uint32_t>(), n_ovf, cap_b,
		                                                 R.list_b.as<uint4>(), R.out_b.as<uint4>(), R.n2b.as<uint32_t>(), R.ovf.as<uint32_t>() /* (cannot overflow) */, R.ctr.p + 3, R.ctr.p + 5);
		HIPCK(hipMemcpyAsync(&c[3], R.ctr.p + 3, 24, hipMemcpyDeviceToHost, st));      // (c[4] is not read again)
		HIPCK(hipStreamSynchronize(st));
	}
	const uint64_t n1 = in.n_kept, n2 = c[0] + c[3], n3 = c[2], n = n1 + n2 + n3;
	if (n >> 32) { bmh_set_error("bmh_seed_batch_reseed: more than 2^32 seed groups in one batch"); return BMH_ECAPACITY; }
	out->n_round[0] = n1; out->n_round[1] = n2; out->n_round[2] = n3;
	g_rs_last[0] = n_tasks; g_rs_last[1] = n_ovf; g_rs_last[2] = n1; g_rs_last[3] = n2; g_rs_last[4] = n3;
	g_rs_last[5] = c[5]; g_rs_last[6] = c[6];

	// ---- merge: keys of every group, radix sort, columns
	RCK(R.keys.need(8 * (n + 1))); RCK(R.keys2.need(8 * (n + 1))); RCK(R.vals.need(4 * (n + 1))); RCK(R.vals2.need(4 * (n + 1)));
	RCK(R.mk.need(8 * (n + 1))); RCK(R.ms.need(4 * (n + 1)));
	RCK(R.ra.need(sizeof(res_t) * (n + 1))); RCK(R.rk.need(8 * (n + 1))); RCK(R.rocc.need(4 * (n + 1))); RCK(R.roff.need(8 * (n + 1)));
	uint64_t *keys = R.keys.as<uint64_t>(), *mk = R.mk.as<uint64_t>(); uint32_t *vals = R.vals.as<uint32_t>(), *ms = R.ms.as<uint32_t>();
	if (n_cands) reseed_copy_r1_kernel<<<rs_nblk(n_cands), 256, 0, st>>>(in.res_a, in.res_k, in.occ, in.occ_off, n_cands, keys, vals, mk, ms);
	reseed_set_kernel<<<1, 1, 0, st>>>(R.ctr.p + 4, (unsigned long long)n1);
	if (n_tasks)
		reseed_copy_out_kernel<<<rs_nblk(n_tasks), 256, 0, st>>>(R.out2.as<uint4>(), R.n2.as<uint32_t>(), nullptr, cap_a, n_tasks, R.tasks.as<rs_task_t>(), nullptr,
		                                                         R.ctr.p + 4, keys, vals, mk, ms);
	if (n_ovf)
		reseed_copy_out_kernel<<<rs_nblk(n_ovf), 256, 0, st>>>(R.out_b.as<uint4>(), R.n2b.as<uint32_t>(), nullptr, cap_b, n_ovf, R.tasks.as<rs_task_t>(), R.ovf.as<uint32_t>(),
		                                                       R.ctr.p + 4, keys, vals, mk, ms);
	if (r3)
		reseed_copy_out_kernel<<<rs_nblk(n_reads), 256, 0, st>>>(R.out3.as<uint4>(), R.n3.as<uint32_t>(), R.off3.as<uint64_t>(), 0u, (uint32_t)n_reads, nullptr, nullptr,
		                                                         R.ctr.p + 4, keys, vals, mk, ms);
	int end_bit = 33;
	while (end_bit < 64 && (n_reads >> (end_bit - 32)) != 0) ++end_bit;
	size_t ts = 0, tsc = 0, tsr = 0;
	HIPCK(rocprim::radix_sort_pairs(nullptr, ts, keys, R.keys2.as<uint64_t>(), vals, R.vals2.as<uint32_t>(), (size_t)n, 0, end_bit, st));
	HIPCK(rocprim::exclusive_scan(nullptr, tsc, R.rocc.as<uint32_t>(), R.roff.as<uint64_t>(), (uint64_t)0, (size_t)n + 1, rocprim::plus<uint64_t>(), st));
	HIPCK(rocprim::exclusive_scan(nullptr, tsr, in.n_ref_pos, in.prefix, 0u, (size_t)n_reads, rocprim::plus<uint32_t>(), st));
	if (tsc > ts) ts = tsc;
	if (tsr > ts) ts = tsr;
	RCK(R.tmp.need(ts));
	if (n) { tb = R.tmp.cap; HIPCK(rocprim::radix_sort_pairs(R.tmp.p, tb, keys, R.keys2.as<uint64_t>(), vals, R.vals2.as<uint32_t>(), (size_t)n, 0, end_bit, st)); }
	HIPCK(hipMemsetAsync(in.n_ref_pos, 0, 4 * n_reads, st));
	reseed_gather_kernel<<<rs_nblk(n + 1), 256, 0, st>>>(R.keys2.as<uint64_t>(), R.vals2.as<uint32_t>(), n, mk, ms, R.ra.as<res_t>(), R.rk.as<uint64_t>(), R.rocc.as<uint32_t>(), in.n_ref_pos);
	tb = R.tmp.cap;
	HIPCK(rocprim::exclusive_scan(R.tmp.p, tb, R.rocc.as<uint32_t>(), R.roff.as<uint64_t>(), (uint64_t)0, (size_t)n + 1, rocprim::plus<uint64_t>(), st));
	tb = R.tmp.cap;
	HIPCK(rocprim::exclusive_scan(R.tmp.p, tb, in.n_ref_pos, in.prefix, 0u, (size_t)n_reads, rocprim::plus<uint32_t>(), st));
	uint64_t tot = 0;
	HIPCK(hipMemcpyAsync(&tot, R.roff.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, st));
	HIPCK(hipStreamSynchronize(st));
	HIPCK(hipGetLastError());
	out->res_a = R.ra.as<res_t>(); out->res_k = R.rk.as<uint64_t>(); out->occ = R.rocc.as<uint32_t>(); out->occ_off = R.roff.as<uint64_t>();
	out->n = n; out->n_occ = tot;
	return BMH_OK;
}
