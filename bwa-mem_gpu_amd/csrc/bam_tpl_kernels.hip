// Whole-file templates by name on the device (BDP_TPL_FILE; csrc/bam_tpl_core.h has the rules), gfx950, wave64.
//
//   parts      per batch, behind bpo_check_fix: one lane per record writes the record's 32-byte part (btp_part: the two name hashes, the end word, the score, the
//              bits) and, with their options, its barcode word and its location.  Names and tags are unaligned: every read is by bytes or by words assembled from
//              bytes.  A lane touches nothing outside off [i] .. off [i + 1], which lie inside the batch; a record that is not whole inside them gives an empty part
//   grouping   once per file, over every record's part in file order: two stable rocprim radix passes (h0, then h1 through the first pass's permutation) with the
//              file index as the value; a set's head is a place whose key differs from its predecessor's, and its first record the index there (the sort is
//              stable); the firsts get a 1 at their place in file order and an exclusive scan over those numbers the templates
//   fold       one lane per sorted place, the lanes at set heads working: the lane walks its set's members (one to a few; a long set is a loop in one lane), folds
//              them (btp_fold), writes the entry at the set's ordinal with the first record's location and barcode word, and the ordinal to rec_tpl of every member.
//              The refusal word index << 3 | code is reduced in LDS and sent with one 64-bit atomicMin per block
//   counts     one lane per record: the secondary or supplementary records, the unmapped records and the templates, in total (__syncthreads_count, one atomicAdd
//              per block) and per library (a histogram in LDS, one atomicAdd per non-zero slot per block)
//
// The grouping asks for its memory at once and frees it before it returns: the decision allocates next.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <new>
#include <vector>
#include "bam_tpl.h"
#include "bam_post.h"
#include "devmem.h"

struct btp_dev_t {
	dev_buf<uint8_t> g_ids, g_off, g_lib, tmp, recs, off; uint32_t g_n = 0;
	dev_buf<btp_part_t> parts; dev_buf<bdp_loc_t> locs, tl; dev_buf<uint64_t> bcs, tb, key, key2; dev_buf<uint32_t> iota, idx, idx2, first, ord, rec_tpl; dev_buf<bdp_entry_t> E;
	dev_buf<unsigned long long> out;
	void drop_all() { tmp.drop(); parts.drop(); locs.drop(); tl.drop(); bcs.drop(); tb.drop(); key.drop(); key2.drop(); iota.drop(); idx.drop(); idx2.drop(); first.drop(); ord.drop(); rec_tpl.drop(); E.drop(); }
};

namespace {

unsigned blocks(uint64_t n) { return (unsigned)((n + 255) / 256); }

__global__ void __launch_bounds__(256) btp_parts(const uint8_t *__restrict__ recs, const uint64_t *__restrict__ off, uint32_t n, uint64_t total, bdp_groups_t G, bdp_bc_t bc, uint32_t hash_bits,
                                                 btp_part_t *__restrict__ parts, bdp_loc_t *__restrict__ locs, uint64_t *__restrict__ bcs, uint32_t *__restrict__ iota)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	iota[i] = i;
	const uint64_t a = off[i], b = off[i + 1];
	const uint64_t sz = a <= b && b <= total ? b - a : 0;
	btp_part_t p; p.h0 = p.h1 = 0; p.end = ~0ull; p.score = p.bits = 0;
	bdp_loc_t l; l.x = l.y = 0; l.tile = 0; l.rg = l.flags = 0;
	uint64_t w = 0;
	const uint8_t *rec = recs + a;
	if (sz >= BSR_FIXED && bsr_record_bytes(rec, sz) == sz && bdp_record_whole(rec, sz)) p = btp_part(rec, sz, G.n ? &G : nullptr, bc.mode != BDP_BC_OFF ? &bc : nullptr, &w, locs ? &l : nullptr, hash_bits);
	parts[i] = p;
	if (locs) locs[i] = l;
	if (bcs) bcs[i] = w;
}

// pass 0: key [i] = h0 of record i, idx [i] = i; pass 1: key [j] = h1 of the record at place j of the first pass's order
__global__ void __launch_bounds__(256) btp_keys(const btp_part_t *__restrict__ parts, uint32_t n, int pass, uint64_t *__restrict__ key, uint32_t *__restrict__ idx)
{
	const uint32_t j = blockIdx.x * 256 + threadIdx.x;
	if (j >= n) return;
	if (pass == 0) { key[j] = parts[j].h0; idx[j] = j; }
	else { const uint32_t i = idx[j]; key[j] = i < n ? parts[i].h1 : ~0ull; }
}

__device__ inline bool btp_head_at(const btp_part_t *__restrict__ parts, const uint32_t *__restrict__ idx, uint32_t n, uint32_t j)
{
	if (j == 0) return true;
	const uint32_t a = idx[j], b = idx[j - 1];
	return a >= n || b >= n || !btp_key_equal(parts[a], parts[b]);
}

// first [i] = 1 where record i is the first of its set (first is zeroed before)
__global__ void __launch_bounds__(256) btp_first(const btp_part_t *__restrict__ parts, const uint32_t *__restrict__ idx, uint32_t n, uint32_t *__restrict__ first)
{
	const uint32_t j = blockIdx.x * 256 + threadIdx.x;
	if (j < n && idx[j] < n && btp_head_at(parts, idx, n, j)) first[idx[j]] = 1u;
}

__global__ void __launch_bounds__(256) btp_fold_sets(const btp_part_t *__restrict__ parts, const bdp_loc_t *__restrict__ locs, const uint64_t *__restrict__ bcs, const uint32_t *__restrict__ idx,
                                                     uint32_t n, const uint32_t *__restrict__ ord, uint32_t T, int groups, int barcode, bdp_entry_t *__restrict__ E, bdp_loc_t *__restrict__ tl,
                                                     uint64_t *__restrict__ tb, uint32_t *__restrict__ rec_tpl, unsigned long long *word)
{
	__shared__ unsigned long long min_s;
	if (threadIdx.x == 0) min_s = BPO_NONE;
	__syncthreads();
	const uint32_t j = blockIdx.x * 256 + threadIdx.x;
	if (j < n && idx[j] < n && btp_head_at(parts, idx, n, j)) {
		const uint32_t f = idx[j];
		uint32_t m = 1;
		while (j + m < n && idx[j + m] < n && btp_key_equal(parts[idx[j + m]], parts[f])) ++m;
		const uint32_t t = ord[f];
		if (t < T) {
			bdp_entry_t e; uint32_t role = 0;
			const int st = btp_fold(parts, idx + j, m, groups != 0, barcode != 0, &e, &role);
			E[t] = e;
			if (tl) tl[t] = btp_location(locs[f], role, parts[f], groups != 0);
			if (tb) tb[t] = bcs[f];
			for (uint32_t q = 0; q < m; ++q) rec_tpl[idx[j + q]] = t;
			if (st != BDP_E_OK) atomicMin(&min_s, (unsigned long long)bpo_refusal(f, st));
		}
	}
	__syncthreads();
	if (threadIdx.x == 0 && min_s != BPO_NONE) atomicMin(word, min_s);
}

// out: [0] secondary or supplementary records [1] unmapped records [2] templates, then the same three per library [3 + 3 * lib]
__global__ void __launch_bounds__(256) btp_count(const btp_part_t *__restrict__ parts, const uint32_t *__restrict__ rec_tpl, const uint32_t *__restrict__ first, const bdp_entry_t *__restrict__ E,
                                                 uint32_t n, uint32_t T, uint32_t n_lib, unsigned long long *out)
{
	extern __shared__ uint32_t lib3_s[];
	for (uint32_t k = threadIdx.x; k < 3 * n_lib; k += 256) lib3_s[k] = 0;
	__syncthreads();
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	bool s = false, u = false, h = false;
	if (i < n) {
		const uint32_t b = parts[i].bits, t = rec_tpl[i];
		s = (b & BTP_SECSUP) != 0; u = (b & BTP_UNMAPPED) != 0; h = first[i] != 0;
		if (n_lib && t < T) {
			const uint32_t lib = bdp_lib_of(E[t]);
			if (lib < n_lib) {
				if (s) atomicAdd(lib3_s + 3 * lib, 1u);
				if (u) atomicAdd(lib3_s + 3 * lib + 1, 1u);
				if (h) atomicAdd(lib3_s + 3 * lib + 2, 1u);
			}
		}
	}
	const int c0 = __syncthreads_count(s), c1 = __syncthreads_count(u), c2 = __syncthreads_count(h);
	if (threadIdx.x == 0) {
		if (c0) atomicAdd(out + 0, (unsigned long long)c0);
		if (c1) atomicAdd(out + 1, (unsigned long long)c1);
		if (c2) atomicAdd(out + 2, (unsigned long long)c2);
	}
	for (uint32_t k = threadIdx.x; k < 3 * n_lib; k += 256) if (lib3_s[k]) atomicAdd(out + 3 + k, (unsigned long long)lib3_s[k]);
}

}   // namespace

btp_dev_t *btp_dev_create(void) { return new (std::nothrow) btp_dev_t(); }
void btp_dev_free(btp_dev_t *d) { delete d; }

int btp_dev_set_groups(btp_dev_t *d, const bdp_table_t *T, void *stream)
{
	hipStream_t st = (hipStream_t)stream;
	d->g_n = 0;
	if (!T || T->empty()) return BMH_OK;
	const size_t n = T->lib.size();
	RCK(d->g_ids.need(T->ids.size() + 1)); RCK(d->g_off.need(4 * (n + 1))); RCK(d->g_lib.need(n));
	HIPCK(hipMemcpyAsync(d->g_ids.p, T->ids.data(), T->ids.size(), hipMemcpyHostToDevice, st));
	HIPCK(hipMemcpyAsync(d->g_off.p, T->id_off.data(), 4 * (n + 1), hipMemcpyHostToDevice, st));
	HIPCK(hipMemcpyAsync(d->g_lib.p, T->lib.data(), n, hipMemcpyHostToDevice, st));
	HIPCK(hipStreamSynchronize(st));                                      // (the table may go before the kernels that read it have run)
	d->g_n = (uint32_t)n;
	return BMH_OK;
}

int btp_parts_device(btp_dev_t *d, const uint8_t *d_recs, const uint64_t *d_off, uint32_t n, uint64_t total, const bdp_plan_t &P, uint32_t hash_bits, void *stream, btp_parts_t &S,
                     const uint32_t **d_iota)
{
	hipStream_t st = (hipStream_t)stream;
	const bool optical = P.optical() != nullptr, barcode = P.barcode() != nullptr;
	RCK(d->parts.need((size_t)n + 1)); RCK(d->iota.need((size_t)n + 1));
	if (optical) RCK(d->locs.need((size_t)n + 1));
	if (barcode) RCK(d->bcs.need((size_t)n + 1));
	*d_iota = d->iota.p;
	if (!n) return BMH_OK;
	if ((P.groups() != nullptr) != (d->g_n != 0)) { bmh_set_error("duplicate marking: internal error: the read groups are not on the device"); return BMH_EINVAL; }
	const bdp_groups_t G = {(const char *)d->g_ids.p, (const uint32_t *)d->g_off.p, (const uint8_t *)d->g_lib.p, d->g_n};
	const bdp_bc_t bc = barcode ? *P.barcode() : bdp_bc_t{BDP_BC_OFF, 0, 0, 0};
	btp_parts<<<blocks(n), 256, 0, st>>>(d_recs, d_off, n, total, G, bc, hash_bits, d->parts.p, optical ? d->locs.p : nullptr, barcode ? d->bcs.p : nullptr, d->iota.p);
	HIPCK(hipGetLastError());
	const size_t at = S.parts.size();
	S.parts.resize(at + n);
	HIPCK(hipMemcpyAsync(S.parts.data() + at, d->parts.p, sizeof(btp_part_t) * (size_t)n, hipMemcpyDeviceToHost, st));
	if (optical) { S.locs.resize(at + n); HIPCK(hipMemcpyAsync(S.locs.data() + at, d->locs.p, sizeof(bdp_loc_t) * (size_t)n, hipMemcpyDeviceToHost, st)); }
	if (barcode) { S.bcs.resize(at + n); HIPCK(hipMemcpyAsync(S.bcs.data() + at, d->bcs.p, 8 * (size_t)n, hipMemcpyDeviceToHost, st)); }
	HIPCK(hipStreamSynchronize(st));
	return BMH_OK;
}

int btp_group_device(btp_dev_t *d, const btp_parts_t &S, const bdp_plan_t &P, void *stream, btp_result_t &R, const char *fn)
{
	hipStream_t st = (hipStream_t)stream;
	const bool groups = P.groups() != nullptr, optical = P.optical() != nullptr, barcode = P.barcode() != nullptr;
	const uint32_t n_lib = groups ? P.n_lib() : 0;
	const size_t N = S.parts.size();
	R = btp_result_t();
	if (N > 0xfffffff0ull) { bmh_set_error("%s: 2^32 records", fn); return BMH_EINVAL; }
	if (n_lib > BDP_MAX_LIBS) { bmh_set_error("%s: duplicate marking: %u libraries: a run holds at most %d", fn, n_lib, (int)BDP_MAX_LIBS); return BMH_EINVAL; }
	if (groups) R.lib3.assign(3 * (size_t)n_lib, 0);
	if (!N) return BMH_OK;
	if ((optical && S.locs.size() != N) || (barcode && S.bcs.size() != N)) { bmh_set_error("%s: internal error: the parts' side arrays do not match the records", fn); return BMH_EINVAL; }
	const uint32_t n = (uint32_t)N;
	d->drop_all();
	// per record: the part 32, the keys 2 x 8, the indices 2 x 4, first, ord and the map 3 x 4; per template (at most one per record): the entry 24; the side arrays twice
	size_t sb = sort_pairs_tmp_bytes<uint64_t, uint32_t>(N), tb = scan_tmp_bytes<uint32_t, uint32_t>(N + 1);
	const size_t tmpb = std::max(sb, tb);
	const size_t per = 32 + 16 + 8 + 12 + 24 + (optical ? 32 : 0) + (barcode ? 16 : 0), want = per * (N + 1) + tmpb + (64u << 20);
	size_t fr = 0, tot = 0;
	HIPCK(hipMemGetInfo(&fr, &tot));
	if (want > fr) {
		bmh_set_error("%s: duplicate marking: the templates of %zu records by name need %zu bytes of device memory (%zu per record and the sort's work space), %zu are free", fn, N, want, per, fr);
		return BMH_ENOMEM;
	}
	RCK(d->parts.resize(N + 1)); RCK(d->key.resize(N + 1)); RCK(d->key2.resize(N + 1)); RCK(d->idx.resize(N + 1)); RCK(d->idx2.resize(N + 1)); RCK(d->first.resize(N + 2)); RCK(d->ord.resize(N + 2));
	RCK(d->rec_tpl.resize(N + 1)); RCK(d->tmp.resize(tmpb)); RCK(d->out.need(4 + 3 * (size_t)BDP_MAX_LIBS));
	if (optical) RCK(d->locs.resize(N + 1));
	if (barcode) RCK(d->bcs.resize(N + 1));
	HIPCK(hipMemcpyAsync(d->parts.p, S.parts.data(), sizeof(btp_part_t) * N, hipMemcpyHostToDevice, st));
	if (optical) HIPCK(hipMemcpyAsync(d->locs.p, S.locs.data(), sizeof(bdp_loc_t) * N, hipMemcpyHostToDevice, st));
	if (barcode) HIPCK(hipMemcpyAsync(d->bcs.p, S.bcs.data(), 8 * N, hipMemcpyHostToDevice, st));
	btp_keys<<<blocks(n), 256, 0, st>>>(d->parts.p, n, 0, d->key.p, d->idx.p);
	HIPCK(rocprim::radix_sort_pairs(d->tmp.p, sb, d->key.p, d->key2.p, d->idx.p, d->idx2.p, N, 0, 64, st));
	btp_keys<<<blocks(n), 256, 0, st>>>(d->parts.p, n, 1, d->key.p, d->idx2.p);
	HIPCK(rocprim::radix_sort_pairs(d->tmp.p, sb, d->key.p, d->key2.p, d->idx2.p, d->idx.p, N, 0, 64, st));
	HIPCK(hipMemsetAsync(d->first.p, 0, 4 * (N + 1), st));
	btp_first<<<blocks(n), 256, 0, st>>>(d->parts.p, d->idx.p, n, d->first.p);
	HIPCK(rocprim::exclusive_scan(d->tmp.p, tb, d->first.p, d->ord.p, 0u, N + 1, rocprim::plus<uint32_t>(), st));
	uint32_t T = 0;
	HIPCK(hipMemcpyAsync(&T, d->ord.p + N, 4, hipMemcpyDeviceToHost, st));
	HIPCK(hipStreamSynchronize(st));
	HIPCK(hipGetLastError());
	if (T == 0 || T > n) { bmh_set_error("%s: internal error: %u templates among %u records", fn, T, n); return BMH_EINVAL; }
	if (T >= 1u << 31) { bmh_set_error("%s: duplicate marking: 2^31 templates", fn); return BMH_EINVAL; }
	RCK(d->E.resize((size_t)T + 1));
	if (optical) RCK(d->tl.resize((size_t)T + 1));
	if (barcode) RCK(d->tb.resize((size_t)T + 1));
	std::vector<unsigned long long> out(4 + 3 * (size_t)n_lib, 0);
	out[0] = BPO_NONE;
	HIPCK(hipMemcpyAsync(d->out.p, out.data(), 8 * out.size(), hipMemcpyHostToDevice, st));
	HIPCK(hipMemsetAsync(d->rec_tpl.p, 0, 4 * N, st));
	btp_fold_sets<<<blocks(n), 256, 0, st>>>(d->parts.p, optical ? d->locs.p : nullptr, barcode ? d->bcs.p : nullptr, d->idx.p, n, d->ord.p, T, groups, barcode, d->E.p, optical ? d->tl.p : nullptr,
	                                         barcode ? d->tb.p : nullptr, d->rec_tpl.p, d->out.p);
	btp_count<<<blocks(n), 256, 4 * 3 * n_lib, st>>>(d->parts.p, d->rec_tpl.p, d->first.p, d->E.p, n, T, n_lib, d->out.p + 1);
	HIPCK(hipGetLastError());
	R.rec_tpl.resize(N); R.E.resize(T);
	HIPCK(hipMemcpyAsync(out.data(), d->out.p, 8 * out.size(), hipMemcpyDeviceToHost, st));
	HIPCK(hipMemcpyAsync(R.rec_tpl.data(), d->rec_tpl.p, 4 * N, hipMemcpyDeviceToHost, st));
	HIPCK(hipMemcpyAsync(R.E.data(), d->E.p, sizeof(bdp_entry_t) * (size_t)T, hipMemcpyDeviceToHost, st));
	if (optical) { R.locs.resize(T); HIPCK(hipMemcpyAsync(R.locs.data(), d->tl.p, sizeof(bdp_loc_t) * (size_t)T, hipMemcpyDeviceToHost, st)); }
	if (barcode) { R.bcs.resize(T); HIPCK(hipMemcpyAsync(R.bcs.data(), d->tb.p, 8 * (size_t)T, hipMemcpyDeviceToHost, st)); }
	HIPCK(hipStreamSynchronize(st));
	d->drop_all();
	R.word = out[0];
	if (R.word != BPO_NONE) return BMH_OK;
	if (out[3] != T) { bmh_set_error("%s: internal error: %llu set heads counted for %u templates", fn, out[3], T); return BMH_EINVAL; }
	R.info[0] = out[1]; R.info[1] = out[2];
	for (size_t k = 0; k < 3 * (size_t)n_lib; ++k) R.lib3[k] = out[4 + k];
	return BMH_OK;
}

namespace {
int templates_device(const char *fn, const uint8_t *records, uint64_t n_bytes, const bmh_markdup_opt_t *opt, int32_t hash_bits, void *stream, bmh_bam_templates_t *out)
{
	hipStream_t st = (hipStream_t)stream;
	bdp_plan_t P; std::vector<uint64_t> off;
	RCK(btp_templates_begin(records, n_bytes, opt, hash_bits, out, fn, P, off));
	struct own_t { btp_dev_t *p = nullptr; ~own_t() { if (p) btp_dev_free(p); } } D;
	if (!(D.p = btp_dev_create())) return BMH_ENOMEM;
	btp_dev_t *d = D.p;
	RCK(btp_dev_set_groups(d, P.groups(), st));
	const uint32_t n = (uint32_t)(off.size() - 1);
	btp_parts_t S; btp_result_t R; const uint32_t *d_iota = nullptr;
	RCK(d->recs.need((size_t)n_bytes + 16)); RCK(d->off.need(8 * off.size()));
	if (n_bytes) HIPCK(hipMemcpyAsync(d->recs.p, records, (size_t)n_bytes, hipMemcpyHostToDevice, st));
	HIPCK(hipMemcpyAsync(d->off.p, off.data(), 8 * off.size(), hipMemcpyHostToDevice, st));
	RCK(btp_parts_device(d, d->recs.p, (const uint64_t *)d->off.p, n, n_bytes, P, (uint32_t)hash_bits, st, S, &d_iota));
	RCK(btp_group_device(d, S, P, st, R, fn));
	if (R.word != BPO_NONE) return btp_refused(S, R.word, P, 0, fn);
	return btp_templates_export(R, P, out, fn);
}
}   // namespace

extern "C" int bmh_bam_templates_device(const uint8_t *records, uint64_t n_bytes, const bmh_markdup_opt_t *opt, int32_t hash_bits, void *stream, bmh_bam_templates_t *out)
{
	const char *fn = "bmh_bam_templates_device";
	try { return templates_device(fn, records, n_bytes, opt, hash_bits, stream, out); }
	catch (const std::bad_alloc &) { bmh_set_error("%s: out of memory", fn); return BMH_ENOMEM; }
}
