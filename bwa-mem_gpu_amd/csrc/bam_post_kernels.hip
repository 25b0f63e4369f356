// Sort, mark duplicates and index a BAM or SAM that any aligner wrote, on the device (csrc/bam_post_core.h has the rules).
//
//   check and fix   one lane per record of a batch, through the chain's offsets: the checks a foreign record needs (bpo_check: whole, references in range, and
//                   with marking a place and an end word that fits, with marking or coverage no long-CIGAR placeholder), then the bin recomputed and, with
//                   marking, 0x400 cleared -- byte stores, records are unaligned.  The smallest refused record of the batch goes through one 64-bit atomicMin per
//                   block on index << 3 | code (the block's own minimum first, through LDS); bins changed, flags cleared and template heads are counted per block
//   heads by name   one lane per record compares its name with its predecessor's (l_read_name, then 32-bit words assembled from bytes): the head flags that
//                   bdp_batch_device's scan numbers (BDP_TPL_NAME), and the two line counts the writer's rule leaves beside them
//   end words       the range check of the unclipped 5' end runs in the check kernel, before the entry kernel of csrc/bam_dup_kernels.hip computes the words it
//                   vouches for
//
// The driver takes the batches of csrc/bam_post.cpp's input: upload, check and fix, with marking the entries (bdp_batch_device under BDP_TPL_NAME, the per-library
// counts), the sorted run (bsr_sort_run_device, the template ordinals as the side word), the run store; at the end of the input the merge of
// csrc/bam_sort_kernels.hip with the plan and the coverage state -- the calls the aligner's output stage makes, without an aligner.
// With collate (BDP_TPL_FILE, csrc/bam_tpl_kernels.hip) a batch makes no entries: it leaves every record's part in the store and sorts with the identity as the side
// word; behind the last batch the grouping numbers the templates of the whole file, the runs' ordinals are rewritten, and the merge runs unchanged.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <new>
#include <vector>
#include "bam_post.h"
#include "bam_ws.h"
#include "bam_tpl.h"

namespace {

unsigned blocks(uint64_t n) { return (unsigned)((n + 255) / 256); }

// a record's bytes inside the buffer: off [i] .. off [i + 1], ascending and at most `total` (else 0: the lane takes no part)
__device__ inline uint64_t bpo_size_at(const uint64_t *__restrict__ off, uint32_t i, uint64_t total)
{
	const uint64_t a = off[i], b = off[i + 1];
	return a <= b && b <= total ? b - a : 0;
}

// word: the smallest index << 3 | code of the batch (BPO_NONE at first); cnt: [0] bins changed [1] 0x400 cleared [2] template heads
__global__ void __launch_bounds__(256) bpo_check_fix(uint8_t *__restrict__ recs, const uint64_t *__restrict__ off, uint32_t n, uint64_t total, int32_t n_ref, uint32_t mode,
                                                     unsigned long long *word, unsigned long long *cnt)
{
	__shared__ unsigned long long min_s;
	if (threadIdx.x == 0) min_s = BPO_NONE;
	__syncthreads();
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	uint32_t changed = 0; bool head = false;
	if (i < n) {
		const uint64_t sz = bpo_size_at(off, i, total);
		int st = sz ? bpo_fix(recs + off[i], sz, n_ref, mode, &changed) : (int)BPO_E_CUT;
		if (st != BPO_OK) atomicMin(&min_s, (unsigned long long)bpo_refusal(i, st));
		// (the fix writes bytes 14, 15 and 19 only; the neighbour's name compare reads byte 12 and the bytes from 36 on)
		else head = i == 0 || !(bpo_size_at(off, i - 1, total) && bpo_name_equal(recs + off[i], sz, recs + off[i - 1], off[i] - off[i - 1]));
	}
	const int c0 = __syncthreads_count(changed & 1u), c1 = __syncthreads_count(changed & 2u), c2 = __syncthreads_count(head);
	if (threadIdx.x == 0) {
		if (min_s != BPO_NONE) atomicMin(word, min_s);
		if (c0) atomicAdd(cnt + 0, (unsigned long long)c0);
		if (c1) atomicAdd(cnt + 1, (unsigned long long)c1);
		if (c2) atomicAdd(cnt + 2, (unsigned long long)c2);
	}
}

// BDP_TPL_NAME: head [i] = 1 where record i begins a template; info [2], [3] += the secondary or supplementary and the unmapped records (bdp_heads' counts).  The
// first record always heads a template, so info [1] is never set to 0 here
__global__ void __launch_bounds__(256) bpo_heads(const uint8_t *__restrict__ recs, const uint64_t *__restrict__ off, uint32_t n, uint64_t total, uint32_t *__restrict__ head, uint32_t *info)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	uint32_t fl = 0; bool valid = false;
	if (i < n) {
		const uint64_t sz = bpo_size_at(off, i, total);
		valid = sz >= BSR_FIXED;
		if (valid) fl = bsr_flag(recs + off[i]);
		const bool same = i > 0 && valid && bpo_size_at(off, i - 1, total) && bpo_name_equal(recs + off[i], sz, recs + off[i - 1], off[i] - off[i - 1]);
		head[i] = same ? 0u : 1u;
	}
	const int c0 = __syncthreads_count(valid && (fl & 0x900u)), c1 = __syncthreads_count(valid && (fl & 4u));
	if (threadIdx.x == 0) { if (c0) atomicAdd(info + 2, (uint32_t)c0); if (c1) atomicAdd(info + 3, (uint32_t)c1); }
}

}   // namespace

int bpo_heads_device(const uint8_t *d_recs, const uint64_t *d_off, uint32_t n, uint64_t total, uint32_t *d_head, uint32_t *d_info, void *stream)
{
	if (!n) return BMH_OK;
	bpo_heads<<<blocks(n), 256, 0, (hipStream_t)stream>>>(d_recs, d_off, n, total, d_head, d_info);
	HIPCK(hipGetLastError());
	return BMH_OK;
}

// ---------------------------------------------------------------------------------------------------------------- the device form

namespace {

struct dev_state_t {
	hipStream_t st = nullptr;
	dev_buf<uint8_t> recs, off, word; dev_buf<char> text;
	bsr_dev_t *bsr = nullptr; bdp_dev_t *bdp = nullptr; bmh_bam_ws_t *ws = nullptr, *sam_ws = nullptr; btp_dev_t *btp = nullptr;
	dev_buf<char> ctg_names; dev_buf<uint32_t> ctg_noff; bool ctg_up = false;
	bsr_store_t store;
	std::vector<uint8_t> sorted; std::vector<uint64_t> keys, soff, bcs; std::vector<uint32_t> stpl, lib3; std::vector<bdp_entry_t> E; std::vector<bdp_loc_t> locs;
	~dev_state_t() { if (bsr) bsr_dev_free(bsr); if (bdp) bdp_dev_free(bdp); if (ws) bmh_bam_ws_free(ws); if (sam_ws) bmh_bam_ws_free(sam_ws); if (btp) btp_dev_free(btp); }
};

// SAM lines through the device's converter; the records come back to the host, where the chain and the batches are made as for a BAM
int convert_device(dev_state_t &D, const char *text, size_t n, int n_contigs, const std::string &blob, const std::vector<uint32_t> &noff, std::vector<uint8_t> &recs, uint32_t *bad, uint32_t *status)
{
	if (!D.sam_ws && !(D.sam_ws = bmh_bam_ws_create())) return BMH_ENOMEM;
	if (!D.ctg_up) {
		RCK(D.ctg_names.need(blob.size() + 1)); RCK(D.ctg_noff.need(noff.size()));
		HIPCK(hipMemcpyAsync(D.ctg_names.p, blob.data(), blob.size(), hipMemcpyHostToDevice, D.st));
		HIPCK(hipMemcpyAsync(D.ctg_noff.p, noff.data(), 4 * noff.size(), hipMemcpyHostToDevice, D.st));
		D.ctg_up = true;
	}
	RCK(D.text.need(n + 1));
	HIPCK(hipMemcpyAsync(D.text.p, text, n, hipMemcpyHostToDevice, D.st));
	bmh_bam_out_t bo;
	RCK(bmh_sam_to_bam_device(D.sam_ws, D.text.p, n, n_contigs, D.ctg_names.p, D.ctg_noff.p, D.st, &bo));
	*bad = ~0u;
	if (bo.n_refused) { *bad = bo.first_refused; *status = bo.first_status; return BMH_OK; }
	recs.resize((size_t)bo.bam_bytes);
	if (bo.bam_bytes) HIPCK(hipMemcpyAsync(recs.data(), bo.d_bam, (size_t)bo.bam_bytes, hipMemcpyDeviceToHost, D.st));
	HIPCK(hipStreamSynchronize(D.st));
	return BMH_OK;
}

// the templates of the batch's first n records on the device; the verdict's message names file indices
int entries_device(bpo_run_t &R, dev_state_t &D, uint32_t n, uint64_t total, const uint32_t **d_tpl, const bdp_entry_t **d_e, const bdp_loc_t **d_l, const uint64_t **d_b, uint32_t info[BDP_INFO_WORDS_PACK],
                   const uint32_t **d_lib3)
{
	const bdp_bc_t *bc = R.J.P.barcode(); const bool optical = R.J.P.optical() != nullptr, barcode = bc != nullptr, groups = R.J.P.groups() != nullptr;
	const uint32_t *d_info = nullptr;
	RCK(bdp_batch_device(D.bdp, D.recs.p, (const uint64_t *)D.off.p, n, total, D.st, d_tpl, d_e, &d_info, optical ? d_l : nullptr, bc, barcode ? d_b : nullptr, BDP_TPL_NAME));
	if (groups && d_lib3) RCK(bdp_batch_lib_counts_device(D.bdp, D.recs.p, (const uint64_t *)D.off.p, n, total, R.J.P.table.n_lib, D.st, d_lib3));
	HIPCK(hipMemcpyAsync(info, d_info, 4 * bdp_info_words(bc), hipMemcpyDeviceToHost, D.st));
	HIPCK(hipStreamSynchronize(D.st));
	uint32_t bad = 0;
	const int st = bdp_batch_verdict(n, info, groups, barcode, barcode && bc->pack, &bad);
	if (st == BDP_E_OK) {
		if (info[0] == 0 || info[0] > n) { bmh_set_error("%s: internal error: %u templates among %u records", R.fn, info[0], n); return BMH_EINVAL; }
		return BMH_OK;
	}
	const uint64_t at = R.in.base + bad - 1;
	return st == BDP_E_TEMPLATE ? bdp_name_refused(at, R.fn) : st >= BDP_E_BC_TYPE ? bdp_barcode_refused((uint32_t)at, st, R.fn) : bdp_group_refused((uint32_t)at, st, R.fn);
}

int device_batch(bpo_run_t &R, dev_state_t &D)
{
	const bpo_input_t &in = R.in;
	const uint32_t n = in.n; const uint64_t total = in.off[n];
	const int n_ref = (int)in.names.size();
	RCK(D.recs.need((size_t)total + 16)); RCK(D.off.need(8 * ((size_t)n + 1))); RCK(D.word.need(32));
	HIPCK(hipMemcpyAsync(D.recs.p, in.buf.data(), (size_t)total, hipMemcpyHostToDevice, D.st));
	HIPCK(hipMemcpyAsync(D.off.p, in.off.data(), 8 * ((size_t)n + 1), hipMemcpyHostToDevice, D.st));
	unsigned long long w[4] = {BPO_NONE, 0, 0, 0};
	HIPCK(hipMemcpyAsync(D.word.p, w, 32, hipMemcpyHostToDevice, D.st));
	bpo_check_fix<<<blocks(n), 256, 0, D.st>>>(D.recs.p, (const uint64_t *)D.off.p, n, total, n_ref, R.mode, (unsigned long long *)D.word.p, (unsigned long long *)D.word.p + 1);
	HIPCK(hipGetLastError());
	HIPCK(hipMemcpyAsync(w, D.word.p, 32, hipMemcpyDeviceToHost, D.st));
	HIPCK(hipStreamSynchronize(D.st));
	const uint32_t *d_tpl = nullptr, *d_stpl = nullptr, *d_lib3 = nullptr; const bdp_entry_t *d_e = nullptr; const bdp_loc_t *d_l = nullptr; const uint64_t *d_b = nullptr;
	uint32_t info[BDP_INFO_WORDS_PACK] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
	if (R.collate && !D.btp) { if (!(D.btp = btp_dev_create())) return BMH_ENOMEM; RCK(btp_dev_set_groups(D.btp, R.J.P.groups(), D.st)); }
	if (R.J.markdup && !R.collate && !D.bdp) { if (!(D.bdp = bdp_dev_create())) return BMH_ENOMEM; RCK(bdp_dev_set_groups(D.bdp, R.J.P.groups(), D.st)); }
	if (w[0] != BPO_NONE) {
		// a refused record: the templates before the one that holds it are whole, and a refusal among them comes first
		const uint32_t bad = (uint32_t)(w[0] >> 3); const int code = (int)(w[0] & 7u);
		if (bad >= n) { bmh_set_error("%s: internal error: record %u of %u refused", R.fn, bad, n); return BMH_EINVAL; }
		const uint32_t n_ok = R.collate ? 0 : bpo_template_start(in.buf.data(), in.off.data(), bad);
		if (R.J.markdup && n_ok) RCK(entries_device(R, D, n_ok, in.off[n_ok], &d_tpl, &d_e, &d_l, &d_b, info, nullptr));
		return bpo_refused(R.fn, in.base + bad, code, in.buf.data() + in.off[bad], in.off[bad + 1] - in.off[bad], n_ref);
	}
	R.counts.bins_changed += w[1]; R.counts.dup_flags_cleared += w[2]; R.counts.templates += w[3];
	const bool optical = R.J.P.optical() != nullptr, barcode = R.J.P.barcode() != nullptr, groups = R.J.P.groups() != nullptr;
	if (R.collate) RCK(btp_parts_device(D.btp, D.recs.p, (const uint64_t *)D.off.p, n, total, R.J.P, 128, D.st, D.store.tpl_parts, &d_tpl));
	else if (R.J.markdup) RCK(entries_device(R, D, n, total, &d_tpl, &d_e, &d_l, &d_b, info, &d_lib3));
	const uint8_t *ds = nullptr; const uint64_t *dk = nullptr, *dso = nullptr;
	RCK(bsr_sort_run_device(D.bsr, D.recs.p, (const uint64_t *)D.off.p, n, total, D.st, &ds, &dk, &dso, d_tpl, &d_stpl));
	D.sorted.resize((size_t)total + 1); D.keys.resize((size_t)n + 1); D.soff.resize((size_t)n + 2);
	HIPCK(hipMemcpyAsync(D.sorted.data(), ds, (size_t)total, hipMemcpyDeviceToHost, D.st));
	HIPCK(hipMemcpyAsync(D.keys.data(), dk, 8 * (size_t)n, hipMemcpyDeviceToHost, D.st));
	HIPCK(hipMemcpyAsync(D.soff.data(), dso, 8 * ((size_t)n + 1), hipMemcpyDeviceToHost, D.st));
	const uint32_t nt = R.J.markdup ? info[0] : 0;
	if (R.collate) { D.stpl.resize(n); D.E.clear(); HIPCK(hipMemcpyAsync(D.stpl.data(), d_stpl, 4 * (size_t)n, hipMemcpyDeviceToHost, D.st)); }
	else if (R.J.markdup) {
		D.stpl.resize(n); D.E.resize(nt);
		HIPCK(hipMemcpyAsync(D.stpl.data(), d_stpl, 4 * (size_t)n, hipMemcpyDeviceToHost, D.st));
		HIPCK(hipMemcpyAsync(D.E.data(), d_e, sizeof(bdp_entry_t) * (size_t)nt, hipMemcpyDeviceToHost, D.st));
		if (optical) { D.locs.resize(nt); HIPCK(hipMemcpyAsync(D.locs.data(), d_l, sizeof(bdp_loc_t) * (size_t)nt, hipMemcpyDeviceToHost, D.st)); }
		if (barcode) { D.bcs.resize(nt); HIPCK(hipMemcpyAsync(D.bcs.data(), d_b, 8 * (size_t)nt, hipMemcpyDeviceToHost, D.st)); }
		if (groups) { D.lib3.resize(3 * (size_t)R.J.P.table.n_lib); HIPCK(hipMemcpyAsync(D.lib3.data(), d_lib3, 12 * (size_t)R.J.P.table.n_lib, hipMemcpyDeviceToHost, D.st)); }
	}
	HIPCK(hipStreamSynchronize(D.st));
	if (D.soff[n] != total) { bmh_set_error("%s: internal error: the sorted run holds %llu bytes, the batch's records %llu", R.fn, (unsigned long long)D.soff[n], (unsigned long long)total); return BMH_EINVAL; }
	bsr_dup_t bd = {D.stpl.data(), D.E.data(), nt, info[2], info[3]};
	if (groups && !R.collate) { bd.lib3 = D.lib3.data(); bd.n_lib3 = R.J.P.table.n_lib; }
	if (optical && !R.collate) bd.locs = D.locs.data();
	if (barcode && !R.collate) bd.bcs = D.bcs.data();
	RCK(D.store.append(D.sorted.data(), total, D.keys.data(), D.soff.data(), n, R.J.markdup ? &bd : nullptr));
	if (R.collate) D.store.runs.back().tbase = in.base;                // (tpl holds batch indices: the file index of a record is tbase + tpl [i])
	R.counts.records += n; ++R.counts.batches;
	return BMH_OK;
}

// every batch checked and kept as a sorted run, the templates grouped, the runs merged: everything of the device form before bpo_run_t::end
int post_device(bpo_run_t &R, dev_state_t &D, bmh_sam_sink_t sink, void *user, uint64_t *base)
{
	const char *fn = R.fn;
	if (!(D.bsr = bsr_dev_create()) || !(D.ws = bmh_bam_ws_create())) return BMH_ENOMEM;
	if (R.o.sorted.sort_mem) D.store.mem_bytes = R.o.sorted.sort_mem;
	if (R.o.sorted.tmp_dir) D.store.tmp_dir = R.o.sorted.tmp_dir;
	int rc;
	const bool trace = getenv("BMH_ALIGNER_TRACE") != nullptr;
	auto now_ms = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
	const double t_begin = now_ms();
	while ((rc = R.in.next(R.o.batch_bytes, fn)) == 1) RCK(device_batch(R, D));
	if (rc < 0) return rc;
	const double t_batches = now_ms();
	if (R.collate) {                                                   // the templates of the whole file by name: the grouping, then the runs' ordinals rewritten
		if (!D.btp && !(D.btp = btp_dev_create())) return BMH_ENOMEM;
		btp_result_t G;
		RCK(btp_group_device(D.btp, D.store.tpl_parts, R.J.P, D.st, G, fn));
		if (G.word != BPO_NONE) return btp_refused(D.store.tpl_parts, G.word, R.J.P, R.sam_line0(), fn);
		if (G.rec_tpl.size() != R.counts.records) { bmh_set_error("%s: internal error: %zu ordinals for %llu records", fn, G.rec_tpl.size(), (unsigned long long)R.counts.records); return BMH_EINVAL; }
		D.store.retemplate(G.rec_tpl);
		D.store.entries.swap(G.E); D.store.locs.swap(G.locs); D.store.bcs.swap(G.bcs); D.store.lib_info.swap(G.lib3);
		D.store.dup_info[0] = G.info[0]; D.store.dup_info[1] = G.info[1];
		D.store.tpl_parts = btp_parts_t();                             // (their memory goes back before the merge takes its own)
		R.counts.templates = D.store.entries.size();
		btp_dev_free(D.btp); D.btp = nullptr;
	}
	const double t_grouped = now_ms();
	std::string members;
	RCK(R.header_members(members));
	if (sink(user, members.data(), members.size()) != 0) { bmh_set_error("the sink refused the text"); return BMH_EINVAL; }
	*base = members.size();
	R.counts.spilled_runs = D.store.spilled;
	RCK(bsr_write_device(D.bsr, D.ws, D.store, R.J, D.st, sink, user, fn));
	if (trace)
		fprintf(stderr, "[bam post] %llu records in %llu batches: read, checked and sorted in %.1f ms, templates by name over the file in %.1f ms, merged in %.1f ms\n",
		        (unsigned long long)R.counts.records, (unsigned long long)R.counts.batches, t_batches - t_begin, t_grouped - t_batches, now_ms() - t_grouped);
	return BMH_OK;
}

}   // namespace

extern "C" int bmh_bam_post_file_device(const char *path, const bmh_bam_post_opt_t *opt, void *stream, bmh_sam_sink_t sink, void *user, bmh_bam_post_result_t *out, bmh_sorted_results_t *res)
{
	const char *fn = "bmh_bam_post_file_device";
	dev_state_t D; D.st = (hipStream_t)stream;
	bpo_run_t R; uint64_t base = 0;
	int rc;
	try {
		rc = R.begin(path, opt, sink, out, res, fn, [&D](const char *text, size_t n, int nc, const std::string &blob, const std::vector<uint32_t> &noff, std::vector<uint8_t> &recs, uint32_t *bad,
		                                                uint32_t *status) { return convert_device(D, text, n, nc, blob, noff, recs, bad, status); });
		if (rc == BMH_OK) rc = post_device(R, D, sink, user, &base);
	} catch (const std::bad_alloc &) { bmh_set_error("%s: out of memory", fn); rc = BMH_ENOMEM; }
	return R.end(rc, base, sink, user, out, res);
}
