// Reads in host memory -> SAM text, driven from C threads (the host side of the gase_aln run around the
// device path; what worker1 / worker2 + kt_pipeline do in the reference, src/bwamem.c:2042-2340, src/fastmap.c:59-120).
//
// The stages exist already as C-ABI entry points (seeding, chaining, extension, merge, the region tail, CIGARs, the formatter); until
// round 4 a Python loop called them batch after batch and was three to ten times slower than the device path it drove.  Here:
//   * `n_lanes` worker threads take the batches of the read set in turn; a worker owns a stream, its workspaces and pinned staging and
//     takes its batch through H2D -> seeding -> chaining -> extension -> merge -> region tail -> CIGARs -> D2H;
//   * one writer thread formats the finished batches IN ORDER (bmh_format_sam is itself multi-threaded) and hands the text to the
//     caller's sink while the workers are on the next batches.
// Single-end batches finish their region tail on the device (bmh_finalize_regs_device); a batch it refuses (BMH_ECAPACITY), an index
// with ALT contigs and interleaved pairs (bmh_finalize_pairs_dev) take the host forms -- the same choices bwamem_hip/aligner.py makes,
// the same text.  Reads of up to BMH_EXT_LONG_MAX bases: the device job builder chains those beyond 700 bases in wide records, and the
// extension takes query sides up to the aligner's cap (bmh_aligner_set_max_qlen, 768 by default; a batch with a longer one fails the run).
#include <hip/hip_runtime.h>
#include <sched.h>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <sys/mman.h>
#include <sys/stat.h>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#define BMH_CK_PREFIX "bmh_aligner_run: "
#include "bmh_internal.h"
#include "devmem.h"
#include "pair_kernels.h"
#include "bam_ws.h"
#include "bam_sort.h"
#include "bam_dup.h"
#include "bam_cov.h"
#include "bam_stats.h"
#include "batch_queue.h"

namespace {

struct aligner_t {
	const bmh_index_t *idx;
	const uint8_t *pac; int64_t l_pac;
	int n_contigs;
	std::vector<std::string> names; std::vector<const char *> name_ptr;
	std::vector<int64_t> off; std::vector<int32_t> len; std::vector<uint8_t> alt; bool has_alt;
	bmh_chain_opt_t co; bmh_ext_params_t ep; bmh_post_opt_t po; bmh_pe_opt_t pe;
	std::string rg_id;             // the aligner's own copy of popt->rg_id (po.rg_id points into it): the caller's string need not outlive the call that created the aligner
	uint32_t max_qlen = 768;       // the extension cap of the chain workspaces (bmh_aligner_set_max_qlen)
	bmh_reseed_opt_t rs = {0, 1.5f, 10, 20};   // the seeding rounds (bmh_aligner_set_reseed; enable 0: the first round only)
	// what the sorted runs that follow are made under, checked (bmh_aligner_set_sorted_output; csrc/bam_sort.h): the level, the window, the index of a file without
	// records, and the plans of marking, coverage and statistics -- all off unless out_fmt is BMH_OUT_BAM_SORTED.  next.P's table is the run's read groups (below),
	// marked or not; where the counts go is decided when a run begins
	bsr_out_t next;
	int out_fmt = BMH_OUT_SAM, out_level = 1;  // what the sink receives (bmh_aligner_set_output): the records' text, or BGZF members of BAM records
	std::vector<char> ctg_blob; std::vector<uint32_t> ctg_noff;      // the contig table as the BAM converter takes it
	// a run over read groups (bmh_aligner_run_groups), while it lasts: every group's ID (a batch's records carry its group's) and the table duplicate marking reads;
	// the serial changes whenever the table does, so a lane knows whether its copy on the device is the run's
	std::vector<std::string> group_ids; uint64_t groups_serial = 0;
	const char *rg_of(int group) const { return group >= 0 && (size_t)group < group_ids.size() ? group_ids[(size_t)group].c_str() : po.rg_id; }
	// a run that keeps its input's read groups (bmh_aligner_set_keep_rg), while it lasts: the same table holds the header's @RG lines, but the group is a property of
	// a read (rs.groups), not of a batch -- a batch's group stays -1 and its records take their IDs from the table by the read's index
	bool per_read = false;
	bmh_read_groups_t read_groups(const uint32_t *read_group) const { return {read_group, next.P.table.ids.data(), next.P.table.id_off.data(), (uint32_t)next.P.table.lib.size()}; }
};

}   // namespace

// the CPUs this process may actually use: its affinity mask, capped by the cgroup's CPU quota (a container that shows 256 hardware threads
// may be granted 16: two hundred threads on sixteen CPUs spend their time switching)
extern "C" int bmh_effective_cpus(void)
{
	int n = (int)std::thread::hardware_concurrency();
	cpu_set_t set;
	if (sched_getaffinity(0, sizeof(set), &set) == 0) { const int c = CPU_COUNT(&set); if (c > 0 && (n < 1 || c < n)) n = c; }
	FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r");
	if (f) {
		char q[64]; long long per = 0;
		if (fscanf(f, "%63s %lld", q, &per) == 2 && strcmp(q, "max") != 0 && per > 0) { const long long c = (atoll(q) + per - 1) / per; if (c > 0 && c < n) n = (int)c; }
		fclose(f);
	} else if ((f = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) != nullptr) {
		long long quota = -1, per = 0;
		if (fscanf(f, "%lld", &quota) != 1) quota = -1;
		fclose(f);
		FILE *g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r");
		if (g) { if (fscanf(g, "%lld", &per) != 1) per = 0; fclose(g); }
		if (quota > 0 && per > 0) { const long long c = (quota + per - 1) / per; if (c > 0 && c < n) n = (int)c; }
	}
	return n < 1 ? 1 : n;
}

namespace {

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// device (dbuf_t) / pinned host (hbuf_t) buffers that only ever grow (csrc/devmem.h)
template <class T> using dbuf_t = dev_buf<T>;
template <class T> using hbuf_t = pin_buf<T>;

// What the writer needs of a finished batch.  The large arrays are PINNED buffers the device copies straight into; a result goes back
// to a pool when its text is written, so the buffers are allocated a few times per run, not per batch (a million reads leave 70 MB
// of records and 190 MB of CIGAR / MD arrays: every extra pass over them on one thread costs what a device stage costs).
struct result_t {
	uint32_t b0 = 0, n = 0; uint64_t m = 0, n_sel = 0;
	int group = -1;                                                     // the read group of the batch (a run over groups), -1: the aligner's -R or none
	const bmh_read_set_t *rs = nullptr; int64_t id0 = 0; void *token = nullptr;      // the read set the batch [b0, b0 + n) lies in, the index of its first read in the run, the source's handle
	hbuf_t<int32_t> fin, aln, slot32; hbuf_t<uint32_t> opr, off, packed;
	hbuf_t<char> text; uint64_t text_len = 0; bool has_text = false;     // the text written on the device (no formatting on the host)
	hbuf_t<uint64_t> skeys, soff; uint32_t n_rec = 0;                   // sorted BAM: text holds the batch's records in order; their keys and offsets [n_rec + 1]
	hbuf_t<uint32_t> lib3;                                             // ... of a batch that mixes libraries (aligner_t::per_read): its counts per library [3 * libraries]
	hbuf_t<uint64_t> dup_b;                                           // ... when barcodes are compared: the templates' barcode words
	hbuf_t<bdp_loc_t> dup_l;                                          // ... when optical duplicates are counted: the templates' locations
	hbuf_t<uint32_t> stpl; hbuf_t<bdp_entry_t> dup_e; uint32_t dup_info[BDP_INFO_WORDS_PACK] = {0, 0, 0, 0, 0, 0, 0, 0, 0}; uint64_t dup_d2h = 0;      // duplicate marking: the records' template ordinals in that order, the templates' entries, bdp_batch_device's info
	std::vector<int64_t> slot;                   // (host selection only; empty: slot32)
	std::vector<int32_t> h_rec, unflag;          // pairs
	std::vector<uint32_t> dev_index;             // record -> its place in the lane's d_fin when that is not the record's own index (ALT indexes); empty: identity
};

struct lane_t {
	hipStream_t st = nullptr, st2 = nullptr;     // st2: copies to the host beside the kernels of st
	hipStream_t st_hi = nullptr;                 // highest priority: takes st's place for what follows the extension (region tail, selection, CIGARs, text) -- run_batch
	bmh_seed_ws_t *sws = nullptr; uint32_t sws_reads = 0; uint64_t sws_bases = 0;
	bmh_chain_ws_t *cws = nullptr; uint32_t cws_reads = 0; uint64_t cws_seeds = 0; uint64_t regs_guess = 0;
	dbuf_t<uint8_t> d_reads, d_work; dbuf_t<uint32_t> d_offs, d_lens, d_sel, d_opr, d_cigar, d_off, d_packed, d_over, d_sel2; dbuf_t<int32_t> d_out3, d_regs, d_fin, d_aln, d_slot, d_hrec, d_unflag; dbuf_t<char> d_md;
	dbuf_t<int32_t> d_dedup, d_fin2, d_hrec2, d_unflag2, d_rslot, d_hh, d_ufh, d_finh; dbuf_t<uint32_t> d_roff, d_roff2, d_opr2, d_todo_pairs, d_oprh, d_offh; dbuf_t<uint8_t> d_todo, d_scan;   // pairs on the device
	hbuf_t<uint8_t> h_todo; std::vector<uint32_t> todo_pairs, offh; void *pair_scratch = nullptr;
	dbuf_t<uint32_t> d_alt_ids, d_alt_off; dbuf_t<int32_t> d_alt_sub;         // ALT contigs: the reads the host redid, on their way into d_fin
	dbuf_t<uint32_t> d_cg2; dbuf_t<int32_t> d_aln2; dbuf_t<char> d_md2; uint32_t max_read_len = 0;      // the redo of the alignments that overflow the fixed slots
	dbuf_t<char> d_names, d_text, d_ctg_names; dbuf_t<uint64_t> d_name_off, d_text_off; dbuf_t<uint32_t> d_ctg_name_off; dbuf_t<int64_t> d_ctg_off; bool ctg_up = false;
	hbuf_t<uint32_t> h_offs, h_sel, h_rpr; hbuf_t<int32_t> h_regs; hbuf_t<float> h_fr; hbuf_t<uint8_t> h_need, h_reads; hbuf_t<char> h_names; hbuf_t<uint64_t> h_name_off;
	// a FASTQ batch: its qualities (at the letters' offsets) and, with -C, its comments -- staged and sent only when the read set carries them
	dbuf_t<uint8_t> d_quals; dbuf_t<char> d_comments; dbuf_t<uint64_t> d_comment_off; hbuf_t<uint8_t> h_quals; hbuf_t<char> h_comments; hbuf_t<uint64_t> h_comment_off;
	bool has_quals = false, has_comments = false;
	// a run that keeps its input's read groups: every read's group beside the lengths, and the table of IDs (sent when the run's serial changes)
	dbuf_t<uint32_t> d_rgrp, d_rg_off; dbuf_t<char> d_rg_ids; uint64_t rg_serial = 0; bool has_rgrp = false;
	double t[8] = {0, 0, 0, 0, 0, 0, 0, 0};      // h2d, seed, chain+extend+merge, tail, select, cigar + d2h, wait at the gate
	// the copies themselves, timed by events on the lane's stream (what t[0] and t[5] are NOT: those are host clocks around the whole stage -- the staging of the
	// letters, offsets and names on host threads / the CIGAR and text kernels the host waits for): [0] reads, offsets, names H2D  [1] SAM text D2H
	hipEvent_t ev_c[4] = {nullptr, nullptr, nullptr, nullptr}; double copy_ms[2] = {0, 0}; uint64_t copy_bytes[2] = {0, 0}; bool d2h_marked = false;
	uint32_t host_tail = 0;                      // batches of the run whose region tail the device refused (BMH_ECAPACITY): the host forms took them
	bmh_bam_ws_t *bam = nullptr;                 // BAM output: the converter's and the compressor's buffers
	bsr_dev_t *bsr = nullptr;                    // sorted BAM output: the sort's, the gather's and the index pass's buffers
	bdp_dev_t *bdp = nullptr;                    // duplicate marking: the batch's heads, ordinals and entries
	uint64_t groups_serial = 0;                  // ... the read groups it holds are those of the run with this serial (aligner_t)
	~lane_t()
	{
		if (bam) bmh_bam_ws_free(bam);
		if (bsr) bsr_dev_free(bsr);
		if (bdp) bdp_dev_free(bdp);
		for (hipEvent_t e : ev_c) if (e) (void)hipEventDestroy(e);
		if (sws) bmh_seed_ws_free(sws);
		if (cws) bmh_chain_ws_free(cws);
		if (st) { bmh_extend_release(st); (void)hipStreamDestroy(st); }
		if (st2) (void)hipStreamDestroy(st2);
		if (st_hi) { bmh_extend_release(st_hi); (void)hipStreamDestroy(st_hi); }
		if (pair_scratch) bmh_pairs_scratch_free(pair_scratch);
	}
};

// pageable -> pinned on a few threads (one thread copies 15 GB/s: the letters of a million reads were 10 ms of a lane's batch)
void par_memcpy(void *dst, const void *src, size_t n, int n_threads)
{
	const int T = n < (8u << 20) ? 1 : (n_threads < 4 ? (n_threads < 1 ? 1 : n_threads) : 4);
	if (T == 1) { memcpy(dst, src, n); return; }
	std::vector<std::thread> th;
	for (int t = 0; t < T; ++t) {
		const size_t a = (n * (size_t)t / T) & ~(size_t)63, b = t == T - 1 ? n : (n * (size_t)(t + 1) / T) & ~(size_t)63;
		th.emplace_back([=] { memcpy((uint8_t *)dst + a, (const uint8_t *)src + a, b - a); });
	}
	for (auto &x : th) x.join();
}

// CIGAR / NM / MD of the n_sel records listed in Ln.d_sel, packed on the device (bmh_cigar_pack: an alignment's operations and MD string are a dozen
// bytes, its fixed slots 160); the few alignments that overflow the fixed slots (flag 1: more operations, flag 8: a longer MD) are redone with
// large ones and put in place there too.  to_host: the alignments, their offsets and the packed words go to R (the host formatter's inputs).
int cigars(const aligner_t &A, lane_t &Ln, const int32_t *d_fin, uint64_t n_sel, result_t &R, bool to_host, uint64_t *words_out)
{
	// fixed slots: 16 operations; an MD string of 96 bytes for reads up to 192 bases, half a read's length beyond (a 300 bp read with a dozen mismatches
	// writes 60-100 characters: with 96 every tenth alignment went the way of the overflowed ones)
	// The slots of the redone alignments cannot overflow: an alignment of a read of L bases has at most 2 L + 1 operations (every operation but a
	// deletion consumes a base of the read, a deletion stands between two others) and an MD string of at most two characters per reference base it
	// spans (L + the band at most) -- so one pathological read no longer ends a run of millions
	const int max_cigar = 16, md_cap = Ln.max_read_len <= 192 ? 96 : (int)((Ln.max_read_len / 2 + 31) & ~31u);
	const int MC = std::max(64, 2 * (int)Ln.max_read_len + 2), MD = std::max(1024, (int)((4 * Ln.max_read_len + 2 * (uint32_t)std::max(A.co.w, 0) + 64 + 31) & ~31u));
	R.n_sel = n_sel;
	*words_out = 0;
	if (to_host) { RCK(R.aln.need(8 * (n_sel + 1))); RCK(R.off.need(n_sel + 2)); }
	RCK(Ln.d_aln.need(8 * (n_sel + 1))); RCK(Ln.d_off.need(n_sel + 2)); RCK(Ln.d_packed.need(1));
	if (n_sel == 0) return BMH_OK;
	RCK(Ln.d_cigar.need((size_t)max_cigar * n_sel)); RCK(Ln.d_md.need((size_t)md_cap * n_sel)); RCK(Ln.d_over.need(n_sel + 8)); RCK(Ln.d_sel2.need(n_sel));
	RCK(bmh_cigar_batch(A.idx, Ln.d_reads.p, Ln.d_offs.p, Ln.d_lens.p, d_fin, 16, Ln.d_sel.p, (uint32_t)n_sel, &A.ep, A.co.w, max_cigar, Ln.d_cigar.p, Ln.d_aln.p, md_cap, Ln.d_md.p, Ln.st));
	const size_t wb = bmh_cigar_pack_work((uint32_t)n_sel);
	RCK(Ln.d_work.need(wb));
	// (the counter of the overflowed alignments: the last word of d_over's spare room)
	const int64_t n_over = bmh_cigar_overflowed(Ln.d_aln.p, (uint32_t)n_sel, Ln.d_sel.p, Ln.d_over.p, Ln.d_sel2.p, Ln.d_over.p + n_sel + 4, Ln.st);
	if (n_over < 0) return (int)n_over;
	int64_t words = bmh_cigar_pack_sizes(Ln.d_aln.p, (uint32_t)n_sel, 1, Ln.d_off.p, Ln.d_work.p, Ln.d_work.cap, Ln.st);
	if (words < 0) return (int)words;
	RCK(Ln.d_packed.need((size_t)words + (size_t)n_over * (MC + MD / 4) + 1));
	RCK(bmh_cigar_pack(Ln.d_aln.p, Ln.d_cigar.p, max_cigar, Ln.d_md.p, md_cap, (uint32_t)n_sel, Ln.d_off.p, Ln.d_packed.p, Ln.st));
	if (n_over) {
		const size_t no = (size_t)n_over;
		RCK(Ln.d_cg2.need((size_t)MC * no)); RCK(Ln.d_aln2.need(8 * no)); RCK(Ln.d_md2.need((size_t)MD * no)); RCK(Ln.d_work.need(bmh_cigar_patch_work((uint32_t)no)));
		RCK(bmh_cigar_batch(A.idx, Ln.d_reads.p, Ln.d_offs.p, Ln.d_lens.p, d_fin, 16, Ln.d_sel2.p, (uint32_t)no, &A.ep, A.co.w, MC, Ln.d_cg2.p, Ln.d_aln2.p, MD, Ln.d_md2.p, Ln.st));
		words = bmh_cigar_patch(Ln.d_aln.p, Ln.d_off.p, Ln.d_packed.p, (uint64_t)words, Ln.d_over.p, (uint32_t)no, Ln.d_aln2.p, Ln.d_cg2.p, MC, Ln.d_md2.p, MD, Ln.d_work.p, Ln.d_work.cap, Ln.st);
		if (words < 0) return (int)words;
		if (getenv("BMH_ALIGNER_TRACE")) fprintf(stderr, "[aligner] %zu of %llu alignments redone with large CIGAR / MD slots\n", no, (unsigned long long)n_sel);
	}
	*words_out = (uint64_t)words;
	if (!to_host) return BMH_OK;
	RCK(R.packed.need((size_t)words + 1));
	HIPCK(hipMemcpyAsync(R.aln.p, Ln.d_aln.p, 32 * n_sel, hipMemcpyDeviceToHost, Ln.st));
	HIPCK(hipMemcpyAsync(R.off.p, Ln.d_off.p, 4 * (n_sel + 1), hipMemcpyDeviceToHost, Ln.st));
	if (words) HIPCK(hipMemcpyAsync(R.packed.p, Ln.d_packed.p, 4 * (size_t)words, hipMemcpyDeviceToHost, Ln.st));
	HIPCK(hipStreamSynchronize(Ln.st));
	for (uint64_t k = 0; k < n_sel; ++k)
		if (R.aln.p[8 * k + 7] & ~2) { bmh_set_error("bmh_aligner_run: bmh_cigar_batch flagged an alignment (CIGAR or MD longer than the buffers)"); return BMH_ECAPACITY; }
	return BMH_OK;
}

// a record BAM cannot hold fails the run: the one message of the device's converter (text_on_device) and the host's (out_stage_t)
int bam_refused(const std::string &read_name, uint32_t status)
{
	bmh_set_error("BAM output: read '%s': its SAM record cannot be written as BAM: %s", read_name.c_str(), bmh_bam_status_name(status));
	return BMH_EINVAL;
}

// the batch's SAM text written on the device (bmh_sam_text_sizes / _write) and copied into R.text
int text_on_device(const aligner_t &A, lane_t &Ln, const bmh_post_opt_t &po, const int32_t *d_fin, uint32_t n, bool paired, result_t &R)
{
	if (!Ln.ctg_up) {                                              // the sequences' names and offsets, once per lane
		RCK(Ln.d_ctg_names.need(A.ctg_blob.size())); RCK(Ln.d_ctg_name_off.need(A.ctg_noff.size())); RCK(Ln.d_ctg_off.need(A.off.size()));
		HIPCK(hipMemcpy(Ln.d_ctg_names.p, A.ctg_blob.data(), A.ctg_blob.size(), hipMemcpyHostToDevice));
		HIPCK(hipMemcpy(Ln.d_ctg_name_off.p, A.ctg_noff.data(), 4 * A.ctg_noff.size(), hipMemcpyHostToDevice));
		HIPCK(hipMemcpy(Ln.d_ctg_off.p, A.off.data(), 8 * A.off.size(), hipMemcpyHostToDevice));
		Ln.ctg_up = true;
	}
	bmh_sam_dev_t d;
	memset(&d, 0, sizeof(d));
	d.n_reads = n; d.d_names = Ln.d_names.p; d.d_name_off = Ln.d_name_off.p; d.d_reads = Ln.d_reads.p; d.d_offs = Ln.d_offs.p; d.d_lens = Ln.d_lens.p;
	d.n_contigs = A.n_contigs; d.d_contig_names = Ln.d_ctg_names.p; d.d_contig_name_off = Ln.d_ctg_name_off.p; d.d_contig_offset = Ln.d_ctg_off.p;
	d.d_fin = d_fin; d.d_fin_per_read = Ln.d_opr.p; d.d_slot = Ln.d_slot.p; d.d_aln = Ln.d_aln.p; d.d_cig_off = Ln.d_off.p; d.d_packed = Ln.d_packed.p;
	d.d_h_rec = paired ? Ln.d_hrec.p : nullptr; d.d_unflag = paired ? Ln.d_unflag.p : nullptr;
	if (Ln.has_quals) d.d_quals = Ln.d_quals.p;
	if (Ln.has_comments) { d.d_comments = Ln.d_comments.p; d.d_comment_off = Ln.d_comment_off.p; }
	if (Ln.has_rgrp) { d.d_read_group = Ln.d_rgrp.p; d.d_rg_ids = Ln.d_rg_ids.p; d.d_rg_id_off = Ln.d_rg_off.p; d.n_rg = (uint32_t)A.next.P.table.lib.size(); }
	const size_t wb = bmh_sam_text_work(n);
	RCK(Ln.d_work.need(wb)); RCK(Ln.d_text_off.need((size_t)n + 2));
	const int64_t total = bmh_sam_text_sizes(&po, &d, Ln.d_text_off.p, Ln.d_work.p, Ln.d_work.cap, Ln.st);
	if (total < 0) return (int)total;
	RCK(Ln.d_text.need((size_t)total + 1)); RCK(R.text.need((size_t)total + 1));
	RCK(bmh_sam_text_write(&po, &d, Ln.d_text_off.p, Ln.d_text.p, Ln.d_work.p, Ln.d_work.cap, Ln.st));
	if (A.out_fmt == BMH_OUT_BAM || A.out_fmt == BMH_OUT_BAM_SORTED) {
		// BAM output: the text stays on the device -- text -> records -> members on the lane's stream; only the members cross to the host.  The batch's
		// last member is short, so the batches stay independent and the file is their concatenation
		RCK(bmh_sam_text_check(Ln.d_work.p, n, Ln.st));
		R.text_len = 0; R.has_text = true; R.n_rec = 0;
		if (!total) return BMH_OK;
		if (!Ln.bam && !(Ln.bam = bmh_bam_ws_create())) return BMH_ENOMEM;
		bmh_bam_out_t bo;
		RCK(bmh_sam_to_bam_device(Ln.bam, Ln.d_text.p, (uint64_t)total, A.n_contigs, Ln.d_ctg_names.p, Ln.d_ctg_name_off.p, Ln.st, &bo));
		if (bo.n_refused) return bam_refused(bmh_bam_record_name_device(Ln.bam, Ln.d_text.p, (uint64_t)total, bo.first_refused), bo.first_status);
		if (A.out_fmt == BMH_OUT_BAM_SORTED) {
			// sorted output: records -> keys -> sort -> gather on the lane's stream; the run (records, keys, offsets) crosses uncompressed, the writer stores it
			if (!Ln.bsr && !(Ln.bsr = bsr_dev_create())) return BMH_ENOMEM;
			const uint8_t *ds = nullptr; const uint64_t *dk = nullptr, *dso = nullptr;
			const uint32_t nrec = bo.n_records;
			// duplicate marking: on the records in the writer's order, before the sort -- heads, their scan, one entry per template; the ordinals follow the records
			const uint32_t *d_tpl = nullptr, *d_info = nullptr, *d_stpl = nullptr, *d_lib3 = nullptr; const bdp_entry_t *d_e = nullptr; const bdp_loc_t *d_l = nullptr; const uint64_t *d_b = nullptr;
			const bdp_bc_t *bc = A.next.P.barcode(); const bool optical = A.next.P.optical() != nullptr, barcode = bc != nullptr;
			const uint32_t tmax = paired ? n / 2 : n;                   // the batch's templates: every read or pair leaves at least one record, so no more entries than this come down
			if (A.next.markdup) {
				if (!Ln.bdp && !(Ln.bdp = bdp_dev_create())) return BMH_ENOMEM;
				if (Ln.groups_serial != A.groups_serial) { RCK(bdp_dev_set_groups(Ln.bdp, &A.next.P.table, Ln.st)); Ln.groups_serial = A.groups_serial; }
				RCK(bdp_batch_device(Ln.bdp, bo.d_bam, (const uint64_t *)Ln.bam->off.p, nrec, bo.bam_bytes, Ln.st, &d_tpl, &d_e, &d_info, optical ? &d_l : nullptr, bc, barcode ? &d_b : nullptr));
				RCK(R.stpl.need((size_t)nrec + 1)); RCK(R.dup_e.need((size_t)std::min(nrec, tmax) + 1));
				if (optical) RCK(R.dup_l.need((size_t)std::min(nrec, tmax) + 1));
				if (barcode) RCK(R.dup_b.need((size_t)std::min(nrec, tmax) + 1));
				if (A.per_read) {                                     // a batch of several libraries: its counts per library, from the entries' library bytes
					RCK(bdp_batch_lib_counts_device(Ln.bdp, bo.d_bam, (const uint64_t *)Ln.bam->off.p, nrec, bo.bam_bytes, A.next.P.table.n_lib, Ln.st, &d_lib3));
					RCK(R.lib3.need(3 * (size_t)A.next.P.table.n_lib));
				}
			}
			RCK(bsr_sort_run_device(Ln.bsr, bo.d_bam, (const uint64_t *)Ln.bam->off.p, nrec, bo.bam_bytes, Ln.st, &ds, &dk, &dso, d_tpl, &d_stpl));
			RCK(R.text.need((size_t)bo.bam_bytes + 1)); RCK(R.skeys.need((size_t)nrec + 1)); RCK(R.soff.need((size_t)nrec + 2));
			HIPCK(hipEventRecord(Ln.ev_c[2], Ln.st));
			if (bo.bam_bytes) HIPCK(hipMemcpyAsync(R.text.p, ds, (size_t)bo.bam_bytes, hipMemcpyDeviceToHost, Ln.st));
			if (nrec) HIPCK(hipMemcpyAsync(R.skeys.p, dk, 8 * (size_t)nrec, hipMemcpyDeviceToHost, Ln.st));
			HIPCK(hipMemcpyAsync(R.soff.p, dso, 8 * ((size_t)nrec + 1), hipMemcpyDeviceToHost, Ln.st));
			R.dup_d2h = 0;
			if (A.next.markdup) {                                          // (the count comes down with them and is checked below)
				const size_t ne = std::min(nrec, tmax);
				if (nrec) HIPCK(hipMemcpyAsync(R.stpl.p, d_stpl, 4 * (size_t)nrec, hipMemcpyDeviceToHost, Ln.st));
				if (ne) HIPCK(hipMemcpyAsync(R.dup_e.p, d_e, sizeof(bdp_entry_t) * ne, hipMemcpyDeviceToHost, Ln.st));
				if (ne && optical) HIPCK(hipMemcpyAsync(R.dup_l.p, d_l, sizeof(bdp_loc_t) * ne, hipMemcpyDeviceToHost, Ln.st));
				if (ne && barcode) HIPCK(hipMemcpyAsync(R.dup_b.p, d_b, 8 * ne, hipMemcpyDeviceToHost, Ln.st));
				const size_t ni = A.next.P.table.empty() && !barcode ? 16 : 4 * bdp_info_words(bc);      // (with read groups: the words of a template without a known group; with barcodes: of one whose tags are refused)
				HIPCK(hipMemcpyAsync(R.dup_info, d_info, ni, hipMemcpyDeviceToHost, Ln.st));
				if (d_lib3) HIPCK(hipMemcpyAsync(R.lib3.p, d_lib3, 12 * (size_t)A.next.P.table.n_lib, hipMemcpyDeviceToHost, Ln.st));
				R.dup_d2h = 4ull * nrec + sizeof(bdp_entry_t) * ne + ni + (d_lib3 ? 12ull * A.next.P.table.n_lib : 0) + (optical ? sizeof(bdp_loc_t) * ne : 0) + (barcode ? 8ull * ne : 0);
				Ln.copy_bytes[1] += R.dup_d2h;
			}
			HIPCK(hipEventRecord(Ln.ev_c[3], Ln.st));
			Ln.copy_bytes[1] += bo.bam_bytes + 16ull * nrec; Ln.d2h_marked = true;
			HIPCK(hipStreamSynchronize(Ln.st));
			if (A.next.markdup && nrec) {
				RCK(bdp_batch_check(nrec, R.dup_info, !A.next.P.table.empty(), "sorted BAM", barcode, barcode && bc->pack));
				if (R.dup_info[0] == 0 || R.dup_info[0] > std::min(nrec, tmax)) { bmh_set_error("sorted BAM: internal error: %u templates among %u records", R.dup_info[0], nrec); return BMH_EINVAL; }
			}
			if (R.soff.p[nrec] != bo.bam_bytes) {                 // (the gather skips a record whose offsets lie outside the buffers: the scan of the sizes shows it)
				bmh_set_error("sorted BAM: internal error: the sorted run holds %llu bytes, the batch's records %llu", (unsigned long long)R.soff.p[nrec], (unsigned long long)bo.bam_bytes);
				return BMH_EINVAL;
			}
			R.text_len = bo.bam_bytes; R.n_rec = nrec;
			return BMH_OK;
		}
		const uint8_t *d_members = nullptr; uint64_t mb = 0;
		RCK(bmh_bgzf_deflate_device(Ln.bam, bo.d_bam, bo.bam_bytes, A.out_level, Ln.st, &d_members, &mb));
		RCK(R.text.need((size_t)mb + 1));
		if (mb) {
			HIPCK(hipEventRecord(Ln.ev_c[2], Ln.st));
			HIPCK(hipMemcpyAsync(R.text.p, d_members, (size_t)mb, hipMemcpyDeviceToHost, Ln.st));
			HIPCK(hipEventRecord(Ln.ev_c[3], Ln.st));
			Ln.copy_bytes[1] += mb; Ln.d2h_marked = true;
		}
		HIPCK(hipStreamSynchronize(Ln.st));
		R.text_len = mb;
		return BMH_OK;
	}
	if (total) {
		HIPCK(hipEventRecord(Ln.ev_c[2], Ln.st));
		HIPCK(hipMemcpyAsync(R.text.p, Ln.d_text.p, (size_t)total, hipMemcpyDeviceToHost, Ln.st));
		HIPCK(hipEventRecord(Ln.ev_c[3], Ln.st));
		Ln.copy_bytes[1] += (uint64_t)total; Ln.d2h_marked = true;
	}
	RCK(bmh_sam_text_check(Ln.d_work.p, n, Ln.st));
	R.text_len = (uint64_t)total; R.has_text = true;
	return BMH_OK;
}

// An index with ALT contigs, single-end: the device tail has run as if there were none.  A read WITHOUT a hit on an ALT contig comes out of
// mem_mark_primary_se exactly as without the table (n_pri == n: one marking round, secondary_all = secondary, src/bwamem.c:714-760), so only the
// reads that have one are redone on the host, from their regions, with the table -- same number of records (mem_sort_dedup_patch does not look at
// is_alt), written over the device's; their copies for the CIGAR stage are appended behind the m records of d_fin (dev_index).
int patch_alt_reads(const aligner_t &A, lane_t &Ln, const bmh_dev_jobs_t &dj, const bmh_post_opt_t &po, const uint8_t *codes, const uint64_t *offs64,
                    uint32_t n, uint64_t nr, uint64_t m, int n_threads, result_t &R)
{
	const bool tr = getenv("BMH_ALIGNER_TRACE") != nullptr;
	const double ta = now_s();
	RCK(Ln.h_regs.need(8 * (nr + 1))); RCK(Ln.h_rpr.need(n + 1)); RCK(Ln.h_fr.need(n + 1));
	if (nr) HIPCK(hipMemcpyAsync(Ln.h_regs.p, Ln.d_regs.p, 32 * (size_t)nr, hipMemcpyDeviceToHost, Ln.st));
	HIPCK(hipMemcpyAsync(Ln.h_rpr.p, dj.d_regs_per_read, 4 * (size_t)n, hipMemcpyDeviceToHost, Ln.st));
	HIPCK(hipMemcpyAsync(Ln.h_fr.p, dj.d_frac_rep, 4 * (size_t)n, hipMemcpyDeviceToHost, Ln.st));
	HIPCK(hipStreamSynchronize(Ln.st));
	const double tb = now_s();
	std::vector<uint64_t> rec_off((size_t)n + 1, 0), reg_off((size_t)n + 1, 0);
	for (uint32_t r = 0; r < n; ++r) { rec_off[r + 1] = rec_off[r] + R.opr.p[r]; reg_off[r + 1] = reg_off[r] + Ln.h_rpr.p[r]; }
	if (rec_off[n] != m || reg_off[n] != nr) { bmh_set_error("bmh_aligner_run: internal error: record / region counts do not add up"); return BMH_EINVAL; }
	auto on_alt = [&](const int32_t *q) {
		const int64_t rb = (int64_t)(uint32_t)q[4] | (int64_t)q[5] << 32, re = (int64_t)(uint32_t)q[6] | (int64_t)q[7] << 32;
		const int64_t pos = rb < A.l_pac ? rb : (A.l_pac << 1) - 1 - (re - 1);
		int lo = 0, hi = A.n_contigs;
		while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (A.off[(size_t)mid] <= pos) lo = mid; else hi = mid; }
		return A.alt[(size_t)lo] != 0;
	};
	const int T = n >= 65536 ? (n_threads < 8 ? n_threads : 8) : 1;
	std::vector<std::vector<uint32_t>> part((size_t)T);
	auto scan = [&](int t) {
		const uint32_t r0 = (uint32_t)((uint64_t)n * t / T), r1 = (uint32_t)((uint64_t)n * (t + 1) / T);
		for (uint32_t r = r0; r < r1; ++r) {
			bool any = false;
			for (uint64_t k = rec_off[r]; k < rec_off[r + 1] && !any; ++k) any = on_alt(R.fin.p + 16 * k);
			if (any) part[(size_t)t].push_back(r);
			else for (uint64_t k = rec_off[r]; k < rec_off[r + 1]; ++k) R.fin.p[16 * k + 11] = R.fin.p[16 * k + 12];      // the ALT-mode record: [11] = secondary_all (= secondary here)
		}
	};
	if (T == 1) scan(0);
	else { std::vector<std::thread> th; for (int t = 0; t < T; ++t) th.emplace_back(scan, t); for (auto &x : th) x.join(); }
	std::vector<uint32_t> ids;
	for (const auto &v : part) ids.insert(ids.end(), v.begin(), v.end());
	R.dev_index.clear();
	if (ids.empty()) return bmh_alt_records_device(Ln.d_fin.p, m, nullptr, nullptr, nullptr, nullptr, 0, Ln.st);
	const uint32_t ns = (uint32_t)ids.size();
	const double tc = now_s();
	if (tr) fprintf(stderr, "[aligner] ALT contigs: %u of %u reads have a hit on one and are redone on the host; regions to the host %.1f ms, records looked through %.1f ms\n", ns, n, (tb - ta) * 1e3, (tc - tb) * 1e3);
	std::vector<uint32_t> sub_rpr(ns); std::vector<float> sub_fr(ns); std::vector<uint64_t> sub_offs(ns);
	uint64_t n_sub_regs = 0, n_sub_recs = 0;
	for (uint32_t j = 0; j < ns; ++j) { const uint32_t r = ids[j]; sub_rpr[j] = Ln.h_rpr.p[r]; sub_fr[j] = Ln.h_fr.p[r]; sub_offs[j] = offs64[r]; n_sub_regs += sub_rpr[j]; n_sub_recs += R.opr.p[r]; }
	std::vector<int32_t> sub_regs(8 * (size_t)(n_sub_regs + 1)), sub_out(16 * (size_t)(n_sub_regs + 1));
	std::vector<uint32_t> sub_opr(ns);
	{
		uint64_t w = 0;
		for (uint32_t j = 0; j < ns; ++j) { const uint32_t r = ids[j]; memcpy(&sub_regs[8 * w], Ln.h_regs.p + 8 * reg_off[r], 32 * (size_t)sub_rpr[j]); w += sub_rpr[j]; }
	}
	const int64_t ms = bmh_finalize_regs_ids(&A.co, &A.ep, &po, A.l_pac, A.pac, ns, codes, sub_offs.data(), sub_regs.data(), sub_rpr.data(), sub_fr.data(), A.n_contigs,
	                                         A.n_contigs > 1 ? A.off.data() : nullptr, sub_out.data(), sub_opr.data(), n_threads, ids.data());
	if (ms < 0) return (int)ms;
	if ((uint64_t)ms != n_sub_recs) { bmh_set_error("bmh_aligner_run: internal error: the host tail left %lld records where the device tail left %llu", (long long)ms, (unsigned long long)n_sub_recs); return BMH_EINVAL; }
	std::vector<uint32_t> sub_off((size_t)ns + 1, 0);
	uint64_t w = 0;
	for (uint32_t j = 0; j < ns; ++j) {
		const uint32_t r = ids[j];
		if (sub_opr[j] != R.opr.p[r]) { bmh_set_error("bmh_aligner_run: internal error: read %u has %u records on the host, %u on the device", r, sub_opr[j], R.opr.p[r]); return BMH_EINVAL; }
		memcpy(R.fin.p + 16 * rec_off[r], &sub_out[16 * w], 64 * (size_t)sub_opr[j]);
		sub_off[j] = (uint32_t)w;
		w += sub_opr[j];
	}
	sub_off[ns] = (uint32_t)w;
	// the redone records take their places in the device's array too (a read keeps its number of records: mem_sort_dedup_patch does not look at the table), after every
	// record of the batch has become an ALT-mode record ([11] = secondary_all)
	RCK(Ln.d_alt_ids.need(ns)); RCK(Ln.d_alt_off.need((size_t)ns + 1)); RCK(Ln.d_alt_sub.need(16 * ((size_t)ms + 1)));
	HIPCK(hipMemcpyAsync(Ln.d_alt_ids.p, ids.data(), 4 * (size_t)ns, hipMemcpyHostToDevice, Ln.st));
	HIPCK(hipMemcpyAsync(Ln.d_alt_off.p, sub_off.data(), 4 * ((size_t)ns + 1), hipMemcpyHostToDevice, Ln.st));
	if (ms) HIPCK(hipMemcpyAsync(Ln.d_alt_sub.p, sub_out.data(), 64 * (size_t)ms, hipMemcpyHostToDevice, Ln.st));
	RCK(bmh_alt_records_device(Ln.d_fin.p, m, Ln.d_roff.p, Ln.d_alt_ids.p, Ln.d_alt_off.p, Ln.d_alt_sub.p, ns, Ln.st));
	HIPCK(hipStreamSynchronize(Ln.st));                              // (ids, sub_off, sub_out are locals)
	if (tr) fprintf(stderr, "[aligner] ALT contigs: host tail of those reads and their way back %.1f ms\n", (now_s() - tc) * 1e3);
	return BMH_OK;
}

// The single-end tail of a batch of interleaved pairs in the form the pairing kernel reads (regs_core.h: alt_keep_sub_n), with the regions behind mem_sort_dedup_patch
// (d_dedup) and the first record of every read (d_roff) beside the records; *ex: the tail's logarithm table and contig offsets for bmh_pair_device
int64_t pair_tail_device(const bmh_index_t *idx, const bmh_chain_opt_t *co, const bmh_ext_params_t *ep, const bmh_post_opt_t *po, const uint8_t *d_reads, const uint32_t *d_offs, uint32_t n,
                         const int32_t *d_regs, uint64_t nr, const uint32_t *d_rpr, const float *d_frac_rep, int n_contigs, const int64_t *ctg_off, int32_t *d_fin, int32_t *d_dedup,
                         uint32_t *d_opr, uint32_t *d_roff, void *st, bmh_fin_extra_t *ex)
{
	memset(ex, 0, sizeof(*ex));
	ex->d_dedup_out = d_dedup; ex->d_out_off = d_roff; ex->alt_keep_sub_n = 1;
	return bmh_finalize_regs_device_ex(idx, co, ep, po, d_reads, d_offs, n, d_regs, nr, d_rpr, d_frac_rep, n_contigs, n_contigs > 1 ? ctg_off : nullptr, d_fin, d_opr, st, ex);
}

// Interleaved pairs with mem_pair / mem_sam_pe's choices on the device (csrc/pair_dev.hip) for the pairs the mate rescue does not touch: the single-end tail
// for every read (mem_sort_dedup_patch, mem_mark_primary_se, mem_reg2sam's selection) with a copy of the regions behind mem_sort_dedup_patch for the host;
// the host computes the insert-size statistics and finds the pairs the rescue touches (bmh_finalize_pairs_split), the device pairs the others meanwhile;
// the host walks the pairs that are left -- the rescued ones, the ones the device hands back -- and their records take their places on the device.
// On return *d_fin_out / Ln.d_opr / Ln.d_hrec / Ln.d_unflag hold the batch's records as bmh_finalize_pairs would have left them; R.m their number.
struct pd_user_t { const aligner_t *A; lane_t *Ln; const bmh_dev_jobs_t *dj; const bmh_post_opt_t *po; bmh_fin_extra_t *ex; uint32_t n; };
int pd_after_pestat(void *u_, const double *pes)
{
	pd_user_t &u = *(pd_user_t *)u_;
	lane_t &Ln = *u.Ln; const aligner_t &A = *u.A;
	RCK(bmh_pair_device(&A.co, &A.ep, u.po, &A.pe, pes, A.l_pac, A.n_contigs, u.ex->d_ctg_off, u.ex->d_logtab, u.ex->n_log, Ln.d_fin.p, Ln.d_opr.p, Ln.d_roff.p,
	                    u.dj->d_frac_rep, u.n, Ln.d_hrec.p, Ln.d_unflag.p, Ln.d_todo.p, Ln.st));
	HIPCK(hipMemcpyAsync(Ln.h_todo.p, Ln.d_todo.p, u.n / 2, hipMemcpyDeviceToHost, Ln.st));
	return BMH_OK;
}
int pd_before_final(void *u_, const uint8_t **extra)
{
	pd_user_t &u = *(pd_user_t *)u_;
	HIPCK(hipStreamSynchronize(u.Ln->st));
	*extra = u.Ln->h_todo.p;
	return BMH_OK;
}
int pairs_on_device(const aligner_t &A, lane_t &Ln, const bmh_read_set_t &rs, const bmh_dev_jobs_t &dj, const bmh_post_opt_t &po, const uint8_t *codes, const uint64_t *offs64,
                    uint32_t b0, uint32_t n, uint64_t nr, int n_threads, result_t &R, const int32_t **d_fin_out)
{
	const bool prof = getenv("BMH_PAIR_PROFILE") != nullptr;
	const double t0 = now_s();
	RCK(Ln.d_fin.need(16 * (nr + 1))); RCK(Ln.d_opr.need(n + 1)); RCK(Ln.d_dedup.need(16 * (nr + 1))); RCK(Ln.d_roff.need(n + 1));
	RCK(Ln.d_hrec.need(n + 1)); RCK(Ln.d_unflag.need(n + 1)); RCK(Ln.d_todo.need(n / 2 + 1)); RCK(Ln.h_todo.need(n / 2 + 1));
	bmh_fin_extra_t ex;
	const int64_t m1 = pair_tail_device(A.idx, &A.co, &A.ep, &po, Ln.d_reads.p, Ln.d_offs.p, n, Ln.d_regs.p, nr, dj.d_regs_per_read, dj.d_frac_rep, A.n_contigs, A.off.data(),
	                                    Ln.d_fin.p, Ln.d_dedup.p, Ln.d_opr.p, Ln.d_roff.p, Ln.st, &ex);
	if (m1 < 0) return (int)m1;
	RCK(Ln.h_regs.need(16 * ((size_t)m1 + 1))); RCK(Ln.h_rpr.need(n + 1)); RCK(Ln.h_fr.need(n + 1));
	if (m1) HIPCK(hipMemcpyAsync(Ln.h_regs.p, Ln.d_dedup.p, 64 * (size_t)m1, hipMemcpyDeviceToHost, Ln.st));
	HIPCK(hipMemcpyAsync(Ln.h_rpr.p, Ln.d_opr.p, 4 * (size_t)n, hipMemcpyDeviceToHost, Ln.st));
	HIPCK(hipMemcpyAsync(Ln.h_fr.p, dj.d_frac_rep, 4 * (size_t)n, hipMemcpyDeviceToHost, Ln.st));
	HIPCK(hipStreamSynchronize(Ln.st));
	const double t1 = now_s();
	// the host: statistics, the rescue's windows (aligned on the device), the pairs that are the host's
	pd_user_t u = {&A, &Ln, &dj, &po, &ex, n};
	Ln.todo_pairs.resize(n / 2 + 1);
	bmh_pairs_split_t split; memset(&split, 0, sizeof(split));
	split.after_pestat = pd_after_pestat; split.before_final = pd_before_final; split.user = &u; split.todo_pairs = Ln.todo_pairs.data(); split.scratch_slot = &Ln.pair_scratch;
	// knob ALIGNER_RESCUE_DEV=1: the rescue's windows found by a kernel on the regions the device keeps (pair_kernels.hip: rescue_jobs_kernel) instead of the host's
	// first walk -- the same records (tests/test_gpu_parity.py).  Off by default: measured beside each other on one box (profiles/r06_rescue_ab.txt) the host's walk
	// is the faster one by 3 %: the device is the bound of paired reads -> SAM, the walk's 9 ms a batch overlap the other lanes' kernels, the two passes (1 ms each) do not
	const bmh_rescue_in_t rin = {Ln.d_dedup.p, Ln.d_opr.p, Ln.d_roff.p, Ln.d_lens.p, ex.d_ctg_off, A.n_contigs};
	if (bmh_tune("ALIGNER_RESCUE_DEV", 0) != 0) split.rescue_in = &rin;
	uint64_t cap = (uint64_t)m1 + 2ull * n + 4096;                  // (room for every pair: the pairs the device hands back are the ones with the most records)
	int64_t mh = BMH_ECAPACITY;
	RCK(R.opr.need(n + 1)); R.h_rec.resize(n); R.unflag.resize(n);
	for (int attempt = 0; attempt < 4 && mh == BMH_ECAPACITY; ++attempt, cap *= 4) {
		// (a second attempt repeats the device's pair kernel on records it has changed already: they are restored first)
		if (attempt) { bmh_fin_extra_t ex2; const int64_t m2 = pair_tail_device(A.idx, &A.co, &A.ep, &po, Ln.d_reads.p, Ln.d_offs.p, n, Ln.d_regs.p, nr, dj.d_regs_per_read, dj.d_frac_rep, A.n_contigs, A.off.data(),
		                                                                        Ln.d_fin.p, Ln.d_dedup.p, Ln.d_opr.p, Ln.d_roff.p, Ln.st, &ex2); if (m2 != m1) return m2 < 0 ? (int)m2 : BMH_EINVAL; }
		RCK(R.fin.need(16 * (size_t)cap));
		mh = bmh_finalize_pairs_split(A.idx, Ln.d_reads.p, Ln.d_offs.p, Ln.st, &A.co, &A.ep, &po, &A.pe, A.l_pac, A.pac, n, codes, offs64, rs.lens + b0,
		                              Ln.h_regs.p, Ln.h_rpr.p, Ln.h_fr.p, A.n_contigs, A.n_contigs > 1 ? A.off.data() : nullptr, A.n_contigs > 1 ? A.len.data() : nullptr,
		                              R.fin.p, cap, R.opr.p, R.h_rec.data(), R.unflag.data(), n_threads, &split);
	}
	if (mh < 0) return (int)mh;
	const double t2 = now_s();
	// the host's records take their places
	const uint32_t nt = (uint32_t)split.n_todo;
	Ln.offh.resize(2 * (size_t)nt + 1);
	{ uint32_t o = 0; for (uint32_t k = 0; k < 2 * nt; ++k) { Ln.offh[k] = o; o += R.opr.p[k]; } if ((int64_t)o != mh) { bmh_set_error("bmh_aligner_run: internal error: the host's pairs left %lld records, their counts add up to %u", (long long)mh, o); return BMH_EINVAL; } }
	RCK(Ln.d_todo_pairs.need(nt + 1)); RCK(Ln.d_oprh.need(2 * (size_t)nt + 1)); RCK(Ln.d_offh.need(2 * (size_t)nt + 1)); RCK(Ln.d_hh.need(2 * (size_t)nt + 1)); RCK(Ln.d_ufh.need(2 * (size_t)nt + 1));
	RCK(Ln.d_finh.need(16 * ((size_t)mh + 1))); RCK(Ln.d_rslot.need(n + 1)); RCK(Ln.d_opr2.need(n + 1)); RCK(Ln.d_hrec2.need(n + 1)); RCK(Ln.d_unflag2.need(n + 1)); RCK(Ln.d_roff2.need(n + 1));
	if (nt) {
		HIPCK(hipMemcpyAsync(Ln.d_todo_pairs.p, Ln.todo_pairs.data(), 4 * (size_t)nt, hipMemcpyHostToDevice, Ln.st));
		HIPCK(hipMemcpyAsync(Ln.d_oprh.p, R.opr.p, 8 * (size_t)nt, hipMemcpyHostToDevice, Ln.st));
		HIPCK(hipMemcpyAsync(Ln.d_offh.p, Ln.offh.data(), 8 * (size_t)nt, hipMemcpyHostToDevice, Ln.st));
		HIPCK(hipMemcpyAsync(Ln.d_hh.p, R.h_rec.data(), 8 * (size_t)nt, hipMemcpyHostToDevice, Ln.st));
		HIPCK(hipMemcpyAsync(Ln.d_ufh.p, R.unflag.data(), 8 * (size_t)nt, hipMemcpyHostToDevice, Ln.st));
		if (mh) HIPCK(hipMemcpyAsync(Ln.d_finh.p, R.fin.p, 64 * (size_t)mh, hipMemcpyHostToDevice, Ln.st));
	}
	RCK(bmh_pair_merge_counts(n, Ln.d_todo_pairs.p, nt, Ln.d_rslot.p, Ln.d_opr.p, Ln.d_hrec.p, Ln.d_unflag.p, Ln.d_oprh.p, Ln.d_hh.p, Ln.d_ufh.p, Ln.d_opr2.p, Ln.d_hrec2.p, Ln.d_unflag2.p, Ln.st));
	const size_t sb = bmh_pair_scan_bytes(n);
	RCK(Ln.d_scan.need(sb));
	RCK(bmh_pair_scan(Ln.d_opr2.p, Ln.d_roff2.p, n, Ln.d_scan.p, Ln.d_scan.cap, Ln.st));
	uint32_t last[2] = {0, 0};
	HIPCK(hipMemcpyAsync(&last[0], Ln.d_roff2.p + (n - 1), 4, hipMemcpyDeviceToHost, Ln.st));
	HIPCK(hipMemcpyAsync(&last[1], Ln.d_opr2.p + (n - 1), 4, hipMemcpyDeviceToHost, Ln.st));
	HIPCK(hipStreamSynchronize(Ln.st));
	const uint64_t m = (uint64_t)last[0] + last[1];
	RCK(Ln.d_fin2.need(16 * (m + 1)));
	RCK(bmh_pair_merge_records(n, Ln.d_rslot.p, Ln.d_fin.p, Ln.d_roff.p, Ln.d_finh.p, Ln.d_offh.p, Ln.d_opr2.p, Ln.d_roff2.p, Ln.d_fin2.p, Ln.st));
	Ln.d_opr.swap(Ln.d_opr2); Ln.d_hrec.swap(Ln.d_hrec2); Ln.d_unflag.swap(Ln.d_unflag2);
	*d_fin_out = Ln.d_fin2.p;
	R.m = m;
	if (prof) {
		uint32_t n1 = 0, n2 = 0;                                      // (the kernel writes 0, 1 or 2: a pair with a hit on an ALT contig is not handed back)
		for (uint32_t q = 0; q < n / 2; ++q) { n1 += Ln.h_todo.p[q] == 1; n2 += Ln.h_todo.p[q] == 2; }
		fprintf(stderr, "[pairs] handed back by the device: %u pairs with a score too close to an integer, %u beyond %d hits\n", n1, n2, bmh_pair_limit());
	}
	if (prof) fprintf(stderr, "[pairs] on the device: single-end tail + regions to the host %.1f ms, host (statistics, rescue, %u of %u pairs walked) %.1f ms, merge %.1f ms\n",
	                  (t1 - t0) * 1e3, nt, n / 2, (t2 - t1) * 1e3, (now_s() - t2) * 1e3);
	return BMH_OK;
}

// one batch [b0, b1) of the read set on lane Ln -> R
// id0: index of the batch's first read in the run (the tie-break hash of mem_mark_primary_se takes it); src_pinned: rs.ascii is pinned host memory (no staging copy)
// How many lanes may be in the path's device stages (seeding .. regions) at once: knob ALIGNER_GPU_SLOTS, 0 = as many as there are.  Lanes that start together
// stay in step -- all of them seeding, then all of them in the host's walks with the device idle --; with fewer slots than lanes they fall out of step for good.
// (one gate per run -- run_core owns it --, so that two runs in one process with different lane counts do not share a count under different caps)
struct gate_t { std::mutex mu; std::condition_variable cv; int in = 0; int cap = 0; };
struct gate_hold_t {
	gate_t &g; bool held = false;
	explicit gate_hold_t(gate_t &g_) : g(g_)
	{
		if (g.cap <= 0) return;
		std::unique_lock<std::mutex> lk(g.mu);
		g.cv.wait(lk, [&] { return g.in < g.cap; });
		++g.in; held = true;
	}
	void release() { if (!held) return; { std::lock_guard<std::mutex> lk(g.mu); --g.in; } g.cv.notify_all(); held = false; }
	~gate_hold_t() { release(); }
};

int run_batch(const aligner_t &A, lane_t &Ln, const bmh_read_set_t &rs, uint32_t b0, uint32_t b1, int64_t id0, int group, bool src_pinned, bool paired, int n_threads, gate_t &gpu_gate, result_t &R)
{
	const uint32_t n = b1 - b0;
	R.b0 = b0; R.n = n; R.rs = &rs; R.id0 = id0; R.group = group;
	R.dev_index.clear();
	const uint64_t a0 = rs.offs[b0], a1 = rs.offs[b1 - 1] + rs.lens[b1 - 1], nb = a1 - a0;
	if (nb >> 31) { bmh_set_error("bmh_aligner_run: a batch holds 2^31 bases or more (offsets inside a batch are 32-bit)"); return BMH_EINVAL; }
	double t0 = now_s();
	// ---- reads to the device
	RCK(Ln.d_reads.need(nb + 16)); RCK(Ln.d_offs.need(n + 1)); RCK(Ln.d_lens.need(n + 1)); RCK(Ln.h_offs.need(n + 1));
	Ln.max_read_len = 0;
	for (uint32_t r = 0; r < n; ++r) { Ln.h_offs.p[r] = (uint32_t)(rs.offs[b0 + r] - a0); if (rs.lens[b0 + r] > Ln.max_read_len) Ln.max_read_len = rs.lens[b0 + r]; }
	for (hipEvent_t &e : Ln.ev_c) if (!e) HIPCK(hipEventCreate(&e));
	Ln.d2h_marked = false;
	uint64_t h2d_bytes = nb + 8 * (uint64_t)n;
	if (!src_pinned) RCK(Ln.h_reads.need(nb + 16));
	if (!src_pinned) par_memcpy(Ln.h_reads.p, rs.ascii + a0, nb, n_threads);       // (pageable -> pinned by this lane's threads, then one DMA: the lanes stage side by side)
	HIPCK(hipEventRecord(Ln.ev_c[0], Ln.st));
	if (src_pinned) HIPCK(hipMemcpyAsync(Ln.d_reads.p, rs.ascii + a0, nb, hipMemcpyHostToDevice, Ln.st));       // (pinned or registered host memory -- a batch of a read file filled by the loader, a caller's registered buffer: no staging copy)
	else HIPCK(hipMemcpyAsync(Ln.d_reads.p, Ln.h_reads.p, nb, hipMemcpyHostToDevice, Ln.st));
	HIPCK(hipMemcpyAsync(Ln.d_offs.p, Ln.h_offs.p, 4 * (size_t)n, hipMemcpyHostToDevice, Ln.st));
	HIPCK(hipMemcpyAsync(Ln.d_lens.p, rs.lens + b0, 4 * (size_t)n, hipMemcpyHostToDevice, Ln.st));
	// the text is written on the device (bmh_sam_text_*): the names go along
	const bool host_format = getenv("BMH_ALIGNER_HOST_FORMAT") != nullptr;          // (A/B and cross-check: records to the host, text by bmh_format_sam)
	const bool host_select = getenv("BMH_ALIGNER_HOST_SELECT") != nullptr;          // (A/B and cross-check: the host's selection for every batch; implies the host's text)
	const bool text_dev = !host_format && !host_select;
	R.has_text = false; R.text_len = 0;
	// a blob with its offsets (the names; -C: the comments): the batch's part, its offsets from 0, through pinned memory
	auto send_blob = [&](const void *blob, const uint64_t *off, uint64_t n_bytes, hbuf_t<char> &hb, hbuf_t<uint64_t> &ho, dbuf_t<char> &db, dbuf_t<uint64_t> &dof) -> int {
		const uint64_t c0 = off[b0], c1 = b1 < rs.n_reads ? off[b1] : n_bytes;
		RCK(hb.need(c1 - c0 + 1)); RCK(ho.need(n + 2)); RCK(db.need(c1 - c0 + 1)); RCK(dof.need(n + 2));
		memcpy(hb.p, (const char *)blob + c0, c1 - c0);
		for (uint32_t r = 0; r < n; ++r) ho.p[r] = off[b0 + r] - c0;
		ho.p[n] = c1 - c0;
		HIPCK(hipMemcpyAsync(db.p, hb.p, c1 - c0, hipMemcpyHostToDevice, Ln.st));
		HIPCK(hipMemcpyAsync(dof.p, ho.p, 8 * ((size_t)n + 1), hipMemcpyHostToDevice, Ln.st));
		h2d_bytes += (c1 - c0) + 8 * ((uint64_t)n + 1);
		return BMH_OK;
	};
	if (text_dev) RCK(send_blob(rs.names, rs.name_offs, rs.n_name_bytes, Ln.h_names, Ln.h_name_off, Ln.d_names, Ln.d_name_off));
	// FASTQ: the qualities go beside the letters (same offsets); -C: the comments beside the names.  A read set without them takes none of this
	Ln.has_quals = text_dev && rs.quals != nullptr;
	Ln.has_comments = text_dev && A.po.copy_comment && rs.comments != nullptr && rs.comment_offs != nullptr;
	if (Ln.has_quals) {
		RCK(Ln.d_quals.need(nb + 16));
		if (src_pinned) HIPCK(hipMemcpyAsync(Ln.d_quals.p, rs.quals + a0, nb, hipMemcpyHostToDevice, Ln.st));
		else {
			RCK(Ln.h_quals.need(nb + 16));
			par_memcpy(Ln.h_quals.p, rs.quals + a0, nb, n_threads);
			HIPCK(hipMemcpyAsync(Ln.d_quals.p, Ln.h_quals.p, nb, hipMemcpyHostToDevice, Ln.st));
		}
		h2d_bytes += nb;
	}
	if (Ln.has_comments) RCK(send_blob(rs.comments, rs.comment_offs, rs.n_comment_bytes, Ln.h_comments, Ln.h_comment_off, Ln.d_comments, Ln.d_comment_off));
	// a run that keeps its input's read groups: every read's group goes up with the batch, like the comment offsets; the table of IDs once per run and lane
	Ln.has_rgrp = false;
	if (A.per_read) {
		if (!rs.groups) { bmh_set_error("bmh_aligner_run: internal error: a run that keeps read groups met a batch without them"); return BMH_EINVAL; }
		if (text_dev) {
			if (Ln.rg_serial != A.groups_serial) {
				RCK(Ln.d_rg_ids.need(A.next.P.table.ids.size() + 1)); RCK(Ln.d_rg_off.need(A.next.P.table.id_off.size()));
				HIPCK(hipMemcpyAsync(Ln.d_rg_ids.p, A.next.P.table.ids.data(), A.next.P.table.ids.size(), hipMemcpyHostToDevice, Ln.st));
				HIPCK(hipMemcpyAsync(Ln.d_rg_off.p, A.next.P.table.id_off.data(), 4 * A.next.P.table.id_off.size(), hipMemcpyHostToDevice, Ln.st));
				Ln.rg_serial = A.groups_serial;                       // (the aligner's table outlives the run's batches: the copy reads it in its own time)
			}
			RCK(Ln.d_rgrp.need(n + 1));
			HIPCK(hipMemcpyAsync(Ln.d_rgrp.p, rs.groups + b0, 4 * (size_t)n, hipMemcpyHostToDevice, Ln.st));
			h2d_bytes += 4 * (uint64_t)n;
			Ln.has_rgrp = true;
		}
	}
	HIPCK(hipEventRecord(Ln.ev_c[1], Ln.st));
	Ln.copy_bytes[0] += h2d_bytes;
	// ---- seeding
	if (!Ln.sws || n > Ln.sws_reads || nb > Ln.sws_bases) {
		if (Ln.sws) bmh_seed_ws_free(Ln.sws);
		Ln.sws_reads = n + n / 4; Ln.sws_bases = nb + nb / 4;
		// (64 occurrences per read of 150 bases: a batch of long reads gets that per 150 of its bases)
		const uint64_t per = std::max<uint64_t>(Ln.sws_reads, Ln.sws_bases / 150);
		const uint64_t occ = 64ull * per > (1ull << 16) ? 64ull * per : (1ull << 16);
		Ln.sws = bmh_seed_ws_create(Ln.sws_reads, Ln.sws_bases, Ln.sws_bases, occ);          // one candidate per base bounds the candidates; the workspace adds what its chunked appends lose
		if (!Ln.sws) return BMH_ENOMEM;
	}
	const double tg = now_s(); Ln.t[0] += tg - t0;
	gate_hold_t gate(gpu_gate);
	double t1 = now_s(); Ln.t[6] += t1 - tg;                     // (the wait at the gate is its own entry, not part of the upload)
	bmh_seeds_t seeds;
	RCK(bmh_seed_ws_set_sample(Ln.sws, A.rs.enable ? 0u : (uint32_t)A.co.max_occ));      // only what the chaining below reads is located (re-seeding: everything)
	RCK(bmh_seed_batch_reseed(Ln.sws, A.idx, Ln.d_reads.p, Ln.d_offs.p, Ln.d_lens.p, n, A.co.min_seed_len, &A.rs, Ln.st, &seeds));
	double t2 = now_s(); Ln.t[1] += t2 - t1;
	// ---- chains, jobs, extension, regions
	const uint64_t ns = seeds.n_seeds ? seeds.n_seeds : 1;
	if (!Ln.cws || n > Ln.cws_reads || ns > Ln.cws_seeds) {
		if (Ln.cws) bmh_chain_ws_free(Ln.cws);
		Ln.cws_reads = n + n / 4; Ln.cws_seeds = ns + ns / 4 + 1024;
		Ln.cws = bmh_chain_ws_create(Ln.cws_reads, Ln.cws_seeds);
		if (!Ln.cws) return BMH_ENOMEM;
		RCK(bmh_chain_set_materialize(Ln.cws, 0));
		if (A.n_contigs > 1) {
			RCK(bmh_chain_set_contigs(Ln.cws, A.n_contigs, A.off.data(), A.len.data()));
			if (A.has_alt) RCK(bmh_chain_set_alt(Ln.cws, A.n_contigs, A.alt.data()));
		}
	}
	RCK(bmh_chain_ws_set_max_qlen(Ln.cws, A.max_qlen));
	bmh_dev_jobs_t dj;
	// the reference's GPU extension takes the deletion penalties for both gap kinds (src/fastmap.c:417-424)
	bmh_ext_params_t xp = A.ep; xp.o_ins = A.ep.o_del; xp.e_ins = A.ep.e_del;
	// one call for chaining, extension and merge: the seed-rich reads are chained beside the extension of the others (bmh_chain_extend_merge); the
	// regions' array is sized by a guess (the last batch's count, 6 per read to begin with) and the call repeated if the batch has more
	static const bool three_calls = getenv("BMH_ALIGNER_THREE_CALLS") != nullptr;       // (A/B: bmh_chain_batch -> bmh_chain_extend -> bmh_chain_merge)
	if (!three_calls) {
		uint64_t cap = Ln.regs_guess > 6ull * n ? Ln.regs_guess : 6ull * n;
		int rc = BMH_ECAPACITY;
		for (int attempt = 0; attempt < 4 && rc == BMH_ECAPACITY; ++attempt, cap *= 2) {
			RCK(Ln.d_regs.need(8 * (cap + 1)));
			rc = bmh_chain_extend_merge(Ln.cws, &A.co, A.idx, Ln.d_reads.p, Ln.d_offs.p, Ln.d_lens.p, n, &seeds, &xp, Ln.d_regs.p, cap, Ln.st, &dj);
		}
		if (rc != BMH_OK) return rc;
		Ln.regs_guess = dj.n_regs + dj.n_regs / 8;
	} else {
		RCK(bmh_chain_batch(Ln.cws, &A.co, A.idx, Ln.d_reads.p, Ln.d_offs.p, Ln.d_lens.p, n, &seeds, Ln.st, &dj));
		RCK(Ln.d_out3.need(3 * (dj.n_jobs + 1))); RCK(Ln.d_regs.need(8 * (dj.n_regs + 1)));
		RCK(bmh_chain_extend(Ln.cws, &xp, Ln.d_out3.p, nullptr, Ln.st));
		RCK(bmh_chain_merge(Ln.cws, Ln.d_out3.p, Ln.d_regs.p, Ln.st));
	}
	const uint64_t nr = dj.n_regs;
	// What follows the extension -- short kernels that wait on memory: the region tail, the selection, the CIGARs' traceback, the text -- goes to a stream of the
	// highest priority: beside the other lanes' extension kernels, whose waves fill the register files, these are the kernels that should get the slots that
	// become free.  The host waits for the lane's stream first (see bmh_seed_batch: no barrier packet waits in a high-priority queue).
	struct swap_back_t { lane_t &L; bool on; ~swap_back_t() { if (on) std::swap(L.st, L.st_hi); } } sb{Ln, false};
	if (Ln.st_hi) { HIPCK(hipStreamSynchronize(Ln.st)); std::swap(Ln.st, Ln.st_hi); sb.on = true; }
	else if (gate.held) HIPCK(hipStreamSynchronize(Ln.st));
	gate.release();
	double t3 = now_s(); Ln.t[2] += t3 - t2;
	bmh_post_opt_t po = A.po; po.id0 = id0; po.rg_id = A.rg_of(group);
	const uint8_t *codes = rs.codes + a0;
	std::vector<uint64_t> offs64;                                   // offsets relative to the batch, for the host forms
	auto host_offs = [&]() { if (offs64.empty()) { offs64.resize(n); for (uint32_t r = 0; r < n; ++r) offs64[r] = rs.offs[b0 + r] - a0; } return offs64.data(); };
	const int32_t *d_fin = nullptr;
	bool dev_select = true;                                         // the records that need a CIGAR are chosen on the device (bmh_sam_select_device)
	// ---- the region tail
	if (!paired) {
		int64_t m = -1;
		R.dev_index.clear();
		{
			// (ALT contigs: the table goes along; BMH_ALIGNER_ALT_HOST_PATCH: the device tail without it and the reads that touch an ALT contig redone on the host,
			// the form before the device's second marking round: the cross-check)
			const bool alt_patch = A.has_alt && getenv("BMH_ALIGNER_ALT_HOST_PATCH") != nullptr;
			bmh_post_opt_t po_dev = po; if (alt_patch) po_dev.contig_is_alt = nullptr;
			RCK(Ln.d_fin.need(16 * (nr + 1))); RCK(Ln.d_opr.need(n + 1));
			bmh_fin_extra_t ex; memset(&ex, 0, sizeof(ex));
			if (alt_patch) { RCK(Ln.d_roff.need(n + 1)); ex.d_out_off = Ln.d_roff.p; }      // (the first record of every read: where the host's redone reads go)
			m = bmh_finalize_regs_device_ex(A.idx, &A.co, &A.ep, &po_dev, Ln.d_reads.p, Ln.d_offs.p, n, Ln.d_regs.p, nr, dj.d_regs_per_read, dj.d_frac_rep,
			                                A.n_contigs, A.n_contigs > 1 ? A.off.data() : nullptr, Ln.d_fin.p, Ln.d_opr.p, Ln.st, &ex);
			if (m < 0 && m != BMH_ECAPACITY) return (int)m;
			if (m >= 0) {
				// (the stream is idle: the records go home on the second stream while the selection and the CIGAR kernels run on the first)
				if (!text_dev || alt_patch) {                        // (the host looks the records through for hits on ALT contigs)
					RCK(R.fin.need(16 * (size_t)m + 16)); RCK(R.opr.need(n + 1));
					if (m) HIPCK(hipMemcpyAsync(R.fin.p, Ln.d_fin.p, 64 * (size_t)m, hipMemcpyDeviceToHost, Ln.st2));
					HIPCK(hipMemcpyAsync(R.opr.p, Ln.d_opr.p, 4 * (size_t)n, hipMemcpyDeviceToHost, Ln.st2));
				}
				d_fin = Ln.d_fin.p;
				if (alt_patch) {
					HIPCK(hipStreamSynchronize(Ln.st2));
					RCK(patch_alt_reads(A, Ln, dj, po, codes, host_offs(), n, nr, (uint64_t)m, n_threads, R));
				}
			}
		}
		if (m < 0) {                                                // the host tail: a read beyond the device tail's fixed limits
			++Ln.host_tail;
			RCK(Ln.h_regs.need(8 * (nr + 1))); RCK(Ln.h_rpr.need(n + 1)); RCK(Ln.h_fr.need(n + 1));
			if (nr) HIPCK(hipMemcpyAsync(Ln.h_regs.p, Ln.d_regs.p, 32 * (size_t)nr, hipMemcpyDeviceToHost, Ln.st));
			HIPCK(hipMemcpyAsync(Ln.h_rpr.p, dj.d_regs_per_read, 4 * (size_t)n, hipMemcpyDeviceToHost, Ln.st));
			HIPCK(hipMemcpyAsync(Ln.h_fr.p, dj.d_frac_rep, 4 * (size_t)n, hipMemcpyDeviceToHost, Ln.st));
			HIPCK(hipStreamSynchronize(Ln.st));
			RCK(R.fin.need(16 * (size_t)(nr + 1))); RCK(R.opr.need(n + 1));
			m = bmh_finalize_regs(&A.co, &A.ep, &po, A.l_pac, A.pac, n, codes, host_offs(), Ln.h_regs.p, Ln.h_rpr.p, Ln.h_fr.p, A.n_contigs,
			                      A.n_contigs > 1 ? A.off.data() : nullptr, R.fin.p, R.opr.p, n_threads);
			if (m < 0) return (int)m;
			RCK(Ln.d_fin.need(16 * ((size_t)m + 1))); RCK(Ln.d_opr.need(n + 1));
			if (m) HIPCK(hipMemcpyAsync(Ln.d_fin.p, R.fin.p, 64 * (size_t)m, hipMemcpyHostToDevice, Ln.st));
			HIPCK(hipMemcpyAsync(Ln.d_opr.p, R.opr.p, 4 * (size_t)n, hipMemcpyHostToDevice, Ln.st));
			d_fin = Ln.d_fin.p;
		}
		R.m = (uint64_t)m;
	} else {
		bool pe_done = false;
		if (text_dev && !getenv("BMH_ALIGNER_PE_HOST") && !getenv("BMH_ALIGNER_PE_HOST_DEDUP")) {
			int rc_pd = pairs_on_device(A, Ln, rs, dj, po, codes, host_offs(), b0, n, nr, n_threads, R, &d_fin);
			if (rc_pd == BMH_OK) pe_done = true;
			else if (rc_pd != BMH_ECAPACITY) return rc_pd;              // (BMH_ECAPACITY: a read beyond the device tail's fixed limits: the host forms below)
		}
		if (!pe_done) {
			++Ln.host_tail;
		// mem_sort_dedup_patch of every read on the device (the first step of the single-end tail: bmh_dedup_regs_device), the rest of mem_sam_pe on host
		// threads from its records; a batch the device refuses (a read beyond its fixed limits), or BMH_ALIGNER_PE_HOST_DEDUP, takes the regions themselves
		int64_t md = BMH_ECAPACITY;
		if (!getenv("BMH_ALIGNER_PE_HOST_DEDUP")) {
			RCK(Ln.d_fin.need(16 * (nr + 1))); RCK(Ln.d_opr.need(n + 1));
			md = bmh_dedup_regs_device(A.idx, &A.co, &A.ep, &po, Ln.d_reads.p, Ln.d_offs.p, n, Ln.d_regs.p, nr, dj.d_regs_per_read, A.n_contigs, A.n_contigs > 1 ? A.off.data() : nullptr,
			                           Ln.d_fin.p, Ln.d_opr.p, Ln.st);
			if (md < 0 && md != BMH_ECAPACITY) return (int)md;
		}
		const bool deduped = md >= 0;
		const uint64_t n_in = deduped ? (uint64_t)md : nr;
		RCK(Ln.h_regs.need((deduped ? 16 : 8) * (n_in + 1))); RCK(Ln.h_rpr.need(n + 1)); RCK(Ln.h_fr.need(n + 1));
		if (n_in) HIPCK(hipMemcpyAsync(Ln.h_regs.p, deduped ? Ln.d_fin.p : Ln.d_regs.p, (deduped ? 64 : 32) * (size_t)n_in, hipMemcpyDeviceToHost, Ln.st));
		HIPCK(hipMemcpyAsync(Ln.h_rpr.p, deduped ? Ln.d_opr.p : dj.d_regs_per_read, 4 * (size_t)n, hipMemcpyDeviceToHost, Ln.st));
		HIPCK(hipMemcpyAsync(Ln.h_fr.p, dj.d_frac_rep, 4 * (size_t)n, hipMemcpyDeviceToHost, Ln.st));
		HIPCK(hipStreamSynchronize(Ln.st));
		if (getenv("BMH_PAIR_PROFILE")) fprintf(stderr, "[pairs] regions on the host after %.1f ms of the tail\n", (now_s() - t3) * 1e3);
		uint64_t cap = n_in + 2ull * n + 1024;                      // mate rescue adds a few regions per pair
		int64_t m = BMH_ECAPACITY;
		RCK(R.opr.need(n + 1)); R.h_rec.resize(n); R.unflag.resize(n);
		for (int attempt = 0; attempt < 3 && m == BMH_ECAPACITY; ++attempt, cap *= 2) {
			RCK(R.fin.need(16 * (size_t)cap));
			m = (deduped ? bmh_finalize_pairs_deduped : bmh_finalize_pairs_dev)(A.idx, Ln.d_reads.p, Ln.d_offs.p, Ln.st, &A.co, &A.ep, &po, &A.pe, A.l_pac, A.pac, n, codes, host_offs(), rs.lens + b0,
			                           Ln.h_regs.p, Ln.h_rpr.p, Ln.h_fr.p, A.n_contigs, A.n_contigs > 1 ? A.off.data() : nullptr, A.n_contigs > 1 ? A.len.data() : nullptr,
			                           R.fin.p, cap, R.opr.p, R.h_rec.data(), R.unflag.data(), nullptr, n_threads);
		}
		if (m < 0) return (int)m;
		if (getenv("BMH_PAIR_PROFILE")) fprintf(stderr, "[pairs] bmh_finalize_pairs_dev back after %.1f ms of the tail\n", (now_s() - t3) * 1e3);
		R.m = (uint64_t)m;
		RCK(Ln.d_fin.need(16 * ((size_t)m + 1))); RCK(Ln.d_opr.need(n + 1)); RCK(Ln.d_hrec.need(n + 1));
		if (m) HIPCK(hipMemcpyAsync(Ln.d_fin.p, R.fin.p, 64 * (size_t)m, hipMemcpyHostToDevice, Ln.st));
		HIPCK(hipMemcpyAsync(Ln.d_opr.p, R.opr.p, 4 * (size_t)n, hipMemcpyHostToDevice, Ln.st));
		HIPCK(hipMemcpyAsync(Ln.d_hrec.p, R.h_rec.data(), 4 * (size_t)n, hipMemcpyHostToDevice, Ln.st));
		if (text_dev) { RCK(Ln.d_unflag.need(n + 1)); HIPCK(hipMemcpyAsync(Ln.d_unflag.p, R.unflag.data(), 4 * (size_t)n, hipMemcpyHostToDevice, Ln.st)); }
		d_fin = Ln.d_fin.p;
		}
	}
	double t4 = now_s(); Ln.t[3] += t4 - t3;
	// ---- which records need a CIGAR
	const uint64_t m = R.m;
	uint64_t ns_sel = 0;
	RCK(Ln.d_sel.need(m + 1)); RCK(Ln.h_sel.need(m + 1));
	if (dev_select && !host_select) {
		R.slot.clear();
		RCK(Ln.d_slot.need(m + 1)); RCK(R.slot32.need(m + 1));
		const size_t wb = bmh_sam_select_work(n, m);
		RCK(Ln.d_work.need(wb));
		const int64_t k = bmh_sam_select_device(&po, d_fin, Ln.d_opr.p, paired ? Ln.d_hrec.p : nullptr, n, m, Ln.d_sel.p, Ln.d_slot.p, Ln.d_work.p, Ln.d_work.cap, Ln.st);
		if (k < 0) return (int)k;
		ns_sel = (uint64_t)k;
		if (m && !text_dev) HIPCK(hipMemcpyAsync(R.slot32.p, Ln.d_slot.p, 4 * (size_t)m, hipMemcpyDeviceToHost, Ln.st2));
	} else {
		HIPCK(hipStreamSynchronize(Ln.st2));                          // (the records)
		RCK(Ln.h_need.need(m + 1));
		// (reads are independent: ranges of them on host threads -- 3 M records of a million reads were 11 ms on one)
		std::vector<uint64_t> base((size_t)n + 1, 0);
		for (uint32_t r = 0; r < n; ++r) base[r + 1] = base[r] + R.opr.p[r];
		if (base[n] != m) { bmh_set_error("bmh_aligner_run: internal error: %llu records, the per-read counts add up to %llu", (unsigned long long)m, (unsigned long long)base[n]); return BMH_EINVAL; }
		const int T = n >= 65536 ? (n_threads < 8 ? n_threads : 8) : 1;
		std::vector<int64_t> part_rc((size_t)T, 0);
		auto part = [&](int t) {
			const uint32_t r0 = (uint32_t)((uint64_t)n * t / T) & ~1u, r1 = t == T - 1 ? n : (uint32_t)((uint64_t)n * (t + 1) / T) & ~1u;      // (even cuts: pairs stay together)
			if (r1 <= r0) return;
			part_rc[(size_t)t] = paired ? bmh_sam_need_cigar_pe(&po, R.fin.p + 16 * base[r0], R.opr.p + r0, R.h_rec.data() + r0, r1 - r0, Ln.h_need.p + base[r0])
			                            : bmh_sam_need_cigar(&po, R.fin.p + 16 * base[r0], R.opr.p + r0, r1 - r0, Ln.h_need.p + base[r0]);
		};
		if (T == 1) part(0);
		else { std::vector<std::thread> th; for (int t = 0; t < T; ++t) th.emplace_back(part, t); for (auto &x : th) x.join(); }
		for (int64_t v : part_rc) if (v < 0) return (int)v;
		R.slot.assign(m ? m : 1, -1);
		for (uint64_t k = 0; k < m; ++k) if (Ln.h_need.p[k]) { Ln.h_sel.p[ns_sel] = R.dev_index.empty() ? (uint32_t)k : R.dev_index[k]; R.slot[k] = (int64_t)ns_sel; ++ns_sel; }
		if (ns_sel) HIPCK(hipMemcpyAsync(Ln.d_sel.p, Ln.h_sel.p, 4 * ns_sel, hipMemcpyHostToDevice, Ln.st));
	}
	double t5 = now_s(); Ln.t[4] += t5 - t4;
	uint64_t words = 0;
	const bool dev_text_now = text_dev && dev_select;
	RCK(cigars(A, Ln, d_fin, ns_sel, R, !dev_text_now, &words));
	if (dev_text_now) RCK(text_on_device(A, Ln, po, d_fin, n, paired, R));
	HIPCK(hipStreamSynchronize(Ln.st2));
	if (sb.on) HIPCK(hipStreamSynchronize(Ln.st));                   // (the priority stream is idle before the lane's own takes its place again)
	{
		float ms = 0.f;
		if (hipEventSynchronize(Ln.ev_c[1]) == hipSuccess && hipEventElapsedTime(&ms, Ln.ev_c[0], Ln.ev_c[1]) == hipSuccess) Ln.copy_ms[0] += ms;
		if (Ln.d2h_marked && hipEventSynchronize(Ln.ev_c[3]) == hipSuccess && hipEventElapsedTime(&ms, Ln.ev_c[2], Ln.ev_c[3]) == hipSuccess) Ln.copy_ms[1] += ms;
	}
	Ln.t[5] += now_s() - t5;
	return BMH_OK;
}

// a batch of a read file in pinned host memory, filled by the loader thread (batch_queue.h) and read by a lane: the letters go to the device straight from here
struct fbatch_t {
	hbuf_t<uint8_t> ascii, codes, names; hbuf_t<uint64_t> offs, name_offs; hbuf_t<uint32_t> lens;
	hbuf_t<uint8_t> quals, comments; hbuf_t<uint64_t> comment_offs;        // a FASTQ file's qualities; -C: the comments
	hbuf_t<uint32_t> groups;                                               // a BAM whose read groups are kept: every read's
	bmh_read_set_t rs; uint32_t index = 0; int64_t id0 = 0; int group = -1;        // (id0: the first read's index in its file or group; group: of a run over read groups)
	// room for a batch of nr reads, nb bases, nn bytes of names (fq: with qualities; cm: with ncm bytes of comments), and o's pointers into it.  The nt4 codes always:
	// every host form reads them (pairs' walks, ALT reads, a batch the device tail refuses, the host formatter)
	int size(const char *fn, uint64_t nr, uint64_t nb, uint64_t nn, uint64_t ncm, bool fq, bool cm, bmh_read_set_t *o, bool rg = false)
	{
		if (nb >> 31) { bmh_set_error("%s: a batch holds 2^31 bases or more", fn); return BMH_EINVAL; }      // offsets inside a batch are 32-bit
		RCK(ascii.need(nb + 16)); RCK(codes.need(nb + 16)); RCK(names.need(nn + 16)); RCK(offs.need(nr + 2)); RCK(name_offs.need(nr + 2)); RCK(lens.need(nr + 2));
		if (fq) RCK(quals.need(nb + 16));
		if (cm) { RCK(comments.need(ncm + 16)); RCK(comment_offs.need(nr + 2)); }
		o->ascii = ascii.p; o->codes = codes.p; o->names = names.p; o->offs = offs.p; o->name_offs = name_offs.p; o->lens = lens.p;
		if (fq) o->quals = quals.p;
		if (cm) { o->comments = comments.p; o->comment_offs = comment_offs.p; }
		if (rg) { RCK(groups.need(nr + 2)); o->groups = groups.p; }
		return BMH_OK;
	}
};

}   // namespace

extern "C" {

// For the tests (csrc/bmh_internal.h): the device's part of pairs_on_device -- the tail, then the pairing kernel -- on the caller's arrays and statistics.
int64_t bmh_pairs_device_records(const bmh_index_t *idx, const bmh_chain_opt_t *copt, const bmh_ext_params_t *ep, const bmh_post_opt_t *popt, const bmh_pe_opt_t *pe,
                                 const double *pes, const uint8_t *d_reads, const uint32_t *d_offs, uint32_t n_reads, const int32_t *d_regs, uint64_t n_regs,
                                 const uint32_t *d_regs_per_read, const float *d_frac_rep, int n_contigs, const int64_t *contig_offset,
                                 int32_t *d_fin, int32_t *d_dedup, uint32_t *d_opr, uint32_t *d_off, int32_t *d_h_rec, int32_t *d_unflag, uint8_t *d_todo, void *stream)
{
	if (!idx || !copt || !ep || !popt || !pe || !pes || !d_fin || !d_dedup || !d_opr || !d_off || !d_h_rec || !d_unflag || !d_todo) { bmh_set_error("bmh_pairs_device_records: null argument"); return BMH_EINVAL; }
	if ((n_reads & 1) || (popt->id0 & 1)) { bmh_set_error("bmh_pairs_device_records: an odd number of reads or an odd id0 (pairs are interleaved)"); return BMH_EINVAL; }
	bmh_fin_extra_t ex;
	const int64_t m = pair_tail_device(idx, copt, ep, popt, d_reads, d_offs, n_reads, d_regs, n_regs, d_regs_per_read, d_frac_rep, n_contigs, contig_offset,
	                                   d_fin, d_dedup, d_opr, d_off, stream, &ex);
	if (m < 0) return m;
	RCK(bmh_pair_device(copt, ep, popt, pe, pes, (int64_t)idx->dev.l_pac, n_contigs, ex.d_ctg_off, ex.d_logtab, ex.n_log, d_fin, d_opr, d_off, d_frac_rep, n_reads, d_h_rec, d_unflag, d_todo, stream));
	HIPCK(hipStreamSynchronize((hipStream_t)stream));
	return m;
}

// (lanes and result objects stay with the aligner between runs: their workspaces and pinned buffers -- gigabytes for million-read batches
// -- cost more to allocate than a batch costs to align)
struct bmh_aligner {
	std::vector<std::unique_ptr<fbatch_t>> fbatches;      // batch buffers of bmh_aligner_run_fasta (pinned host memory), kept between runs
	aligner_t a;
	std::vector<std::unique_ptr<lane_t>> lanes;
	std::vector<std::unique_ptr<result_t>> pool; int n_results = 0;
	std::vector<std::string> parts;
	int dev = -1;
	uint64_t host_tail_batches = 0;                      // of the last run (bmh_aligner_host_tail_batches)
	uint64_t bam_pairs_bases = 0; int bam_pairs_lanes = 0;   // bmh_aligner_set_bam_pairs
	bool keep_rg = false; bmh_rg_header_fn rg_header = nullptr; void *rg_user = nullptr;      // bmh_aligner_set_keep_rg
	bool collate = false; uint64_t collate_mem = 0;                                            // bmh_aligner_set_collate
	bsr_store_t store;                                   // sorted BAM output: the runs of the run in progress
	// the last sorted run: what it was made under, its index and what it left (a.next as the run began, with its own places for the counts: the marking's record and
	// its libraries' rows); valid: its file was written whole.  What it holds is read off out's plans (bsr_out_t::parts)
	struct last_t { bsr_out_t out; bmh_markdup_counts_t counts = {}; std::vector<uint64_t> lib_counts, lib_opt; bool valid = false; } last;
};

bmh_aligner_t *bmh_aligner_create(const bmh_index_t *idx, const uint8_t *pac, int64_t l_pac, int n_contigs, const char *const *contig_names,
                                  const int32_t *contig_len, const uint8_t *contig_is_alt, const bmh_chain_opt_t *copt, const bmh_ext_params_t *ep,
                                  const bmh_post_opt_t *popt, const bmh_pe_opt_t *pe)
{
	if (!idx || !pac || !copt || !ep || !popt || n_contigs < 1 || !contig_names || !contig_len) { bmh_set_error("bmh_aligner_create: null argument"); return nullptr; }
	if (!idx->dev.pac || (int64_t)idx->dev.l_pac != l_pac) { bmh_set_error("bmh_aligner_create: the index must carry the 2-bit reference of l_pac bases"); return nullptr; }
	bmh_aligner *h = new bmh_aligner();
	aligner_t &A = h->a;
	A.idx = idx; A.pac = pac; A.l_pac = l_pac; A.n_contigs = n_contigs;
	int64_t o = 0;
	for (int c = 0; c < n_contigs; ++c) { A.names.emplace_back(contig_names[c]); A.off.push_back(o); A.len.push_back(contig_len[c]); o += contig_len[c]; A.alt.push_back(contig_is_alt ? contig_is_alt[c] : 0); }
	for (const std::string &s : A.names) A.name_ptr.push_back(s.c_str());
	if (o != l_pac) { bmh_set_error("bmh_aligner_create: the sequences' lengths add up to %lld, l_pac is %lld", (long long)o, (long long)l_pac); delete h; return nullptr; }
	A.has_alt = false;
	for (uint8_t v : A.alt) A.has_alt = A.has_alt || v != 0;
	A.co = *copt; A.ep = *ep; A.po = *popt;
	if (popt->rg_id) { A.rg_id = popt->rg_id; A.po.rg_id = A.rg_id.c_str(); }
	if (pe) A.pe = *pe; else bmh_pe_opt_default(&A.pe);
	A.co.contig_is_alt = A.has_alt ? A.alt.data() : nullptr; A.po.contig_is_alt = A.has_alt ? A.alt.data() : nullptr;
	for (const std::string &s : A.names) { A.ctg_noff.push_back((uint32_t)A.ctg_blob.size()); A.ctg_blob.insert(A.ctg_blob.end(), s.begin(), s.end()); A.ctg_blob.push_back(0); }
	A.ctg_noff.push_back((uint32_t)A.ctg_blob.size());
	return h;
}

// the one setter of sorted output: everything is checked (bsr_out_make's order) before anything changes
int bmh_aligner_set_sorted_output(bmh_aligner_t *h, const bmh_sorted_opt_t *opt)
{
	const char *fn = "bmh_aligner_set_sorted_output";
	if (!h) { bmh_set_error("%s: null aligner", fn); return BMH_EINVAL; }
	if (opt && opt->markdup && (opt->markdup->rg_ids || opt->markdup->rg_lib || opt->markdup->n_groups)) {
		bmh_set_error("%s: an aligner's read groups come from bmh_aligner_run_groups or bmh_aligner_set_keep_rg, not from the marking options (rg_ids stays NULL)", fn); return BMH_EINVAL;
	}
	bmh_markdup_counts_t mc; bmh_coverage_t cv; bmh_bam_stats_t st;      // (the records the check asks for: a run has its own)
	memset(&mc, 0, sizeof mc);
	bmh_sorted_results_t res; memset(&res, 0, sizeof res);
	bmh_recal_t rt;
	res.markdup = &mc; res.coverage = &cv; res.stats = &st; res.recal = &rt;
	// the recalibration table of a run reads the reference the index holds on the device: its bases and the contigs' places are the aligner's (the mask and the
	// group IDs stay the caller's until the run is over)
	bmh_sorted_opt_t with; bmh_recal_opt_t ro; std::vector<uint64_t> coff;
	if (opt && opt->recal && !opt->recal->pac) {
		with = *opt; memset(&ro, 0, sizeof ro); memcpy(&ro, opt->recal, offsetof(bmh_recal_opt_t, no_count));      // (no_count is read with apply only)
		if (ro.apply) ro.no_count = opt->recal->no_count;
		for (int64_t o : h->a.off) coff.push_back((uint64_t)o);
		ro.l_pac = (uint64_t)h->a.l_pac; ro.contig_offset = coff.data();
		with.recal = &ro; opt = &with;
	}
	bsr_out_t J;
	RCK(bsr_out_make(J, opt, h->a.n_contigs, h->a.len.data(), h->a.name_ptr.data(), &res, fn));
	J.timed = true; J.P.table = h->a.next.P.table;
	if (J.recal && !J.RU.pac) J.recal_d_pac = h->a.idx->dev.pac;
	h->a.next = J; h->a.out_fmt = BMH_OUT_BAM_SORTED; h->a.out_level = J.level;
	h->store.clear(); h->store.mem_bytes = opt && opt->sort_mem ? opt->sort_mem : 4ull << 30; h->store.tmp_dir = opt && opt->tmp_dir ? opt->tmp_dir : "";
	h->last = bmh_aligner::last_t(); h->last.out.ix = J.ix; h->last.valid = true;      // (until a run is made: the index of a file without records, and no results)
	return BMH_OK;
}

int bmh_aligner_set_output(bmh_aligner_t *h, int format, int level)
{
	if (!h) { bmh_set_error("bmh_aligner_set_output: null aligner"); return BMH_EINVAL; }
	if (format != BMH_OUT_SAM && format != BMH_OUT_BAM && format != BMH_OUT_BAM_SORTED) { bmh_set_error("bmh_aligner_set_output: format %d (BMH_OUT_SAM, BMH_OUT_BAM or BMH_OUT_BAM_SORTED)", format); return BMH_EINVAL; }
	if (format != BMH_OUT_SAM && level != 0 && level != 1) { bmh_set_error("bmh_aligner_set_output: level %d (0 or 1)", level); return BMH_EINVAL; }
	if (format == BMH_OUT_BAM_SORTED) { bmh_sorted_opt_t o; bmh_sorted_opt_default(&o); o.level = level; return bmh_aligner_set_sorted_output(h, &o); }
	bsr_out_t off; off.P.table = h->a.next.P.table;                      // (the options of sorted output go with the format)
	h->a.next = off; h->a.out_fmt = format; h->a.out_level = level;
	return BMH_OK;
}

int bmh_aligner_set_max_qlen(bmh_aligner_t *h, uint32_t cap)
{
	if (!h) { bmh_set_error("bmh_aligner_set_max_qlen: null aligner"); return BMH_EINVAL; }
	if (cap > BMH_EXT_LONG_MAX) { bmh_set_error("bmh_aligner_set_max_qlen: %u bases > BMH_EXT_LONG_MAX (%d)", cap, BMH_EXT_LONG_MAX); return BMH_EINVAL; }
	h->a.max_qlen = cap > 768 ? cap : 768;
	return BMH_OK;
}

int bmh_aligner_set_reseed(bmh_aligner_t *h, const bmh_reseed_opt_t *opt)
{
	if (!h) { bmh_set_error("bmh_aligner_set_reseed: null aligner"); return BMH_EINVAL; }
	if (opt) h->a.rs = *opt;
	else { bmh_reseed_opt_default(&h->a.rs); h->a.rs.enable = 0; }
	return BMH_OK;
}

int bmh_aligner_sorted_results(bmh_aligner_t *h, bmh_sorted_results_t *out, uint32_t need)
{
	const char *fn = "bmh_aligner_sorted_results";
	static const struct { uint32_t part; const char *did; } parts[] = {{BMH_SORTED_MARKDUP, "marked duplicates"}, {BMH_SORTED_OPTICAL, "counted optical duplicates"}, {BMH_SORTED_BARCODE, "compared barcodes"},
	                                                                   {BMH_SORTED_GROUPED, "grouped barcodes by edits"}, {BMH_SORTED_COVERAGE, "computed coverage"}, {BMH_SORTED_STATS, "computed statistics"},
	                                                                   {BMH_SORTED_RECAL, "counted or applied a recalibration table"}};
	if (!h || !out) { bmh_set_error("%s: null argument", fn); return BMH_EINVAL; }
	const bmh_aligner::last_t &T = h->last;
	const uint32_t have = T.valid ? T.out.parts() : 0;
	if (!(need & BMH_SORTED_RECAL)) out->recal = nullptr;              // (the results' last members are read only when the caller asks for the table by `need`)
	need |= (out->markdup ? BMH_SORTED_MARKDUP : 0u) | (out->coverage ? BMH_SORTED_COVERAGE : 0u) | (out->stats ? BMH_SORTED_STATS : 0u) | (out->recal ? BMH_SORTED_RECAL : 0u);
	for (const auto &p : parts)
		if (need & ~have & p.part) { bmh_set_error("%s: no run has %s (or the last one failed before its file was complete)", fn, p.did); return BMH_EINVAL; }
	bsr_out_t none;
	if (bmh_markdup_counts_t *c = out->markdup) {
		memcpy(c->counts, T.counts.counts, sizeof c->counts); memcpy(c->optical, T.counts.optical, sizeof c->optical); memcpy(c->grouped, T.counts.grouped, sizeof c->grouped);
		c->no_barcode = T.counts.no_barcode;
		if (c->lib_counts && !T.lib_counts.empty()) memcpy(c->lib_counts, T.lib_counts.data(), 8 * T.lib_counts.size());
		if (c->lib_optical && !T.lib_opt.empty()) memcpy(c->lib_optical, T.lib_opt.data(), 8 * T.lib_opt.size());
	}
	return bsr_out_export(T.valid ? T.out : none, out, fn);
}

int bmh_aligner_sort_index(bmh_aligner_t *h, uint64_t base_offset, uint8_t **bai, uint64_t *bai_bytes)
{
	if (!h || !bai || !bai_bytes) { bmh_set_error("bmh_aligner_sort_index: null argument"); return BMH_EINVAL; }
	*bai = nullptr; *bai_bytes = 0;
	if (h->last.out.ix.lin.empty()) { bmh_set_error("bmh_aligner_sort_index: no sorted run has been made (bmh_aligner_set_output with BMH_OUT_BAM_SORTED comes first)"); return BMH_EINVAL; }
	if (!h->last.valid) { bmh_set_error("bmh_aligner_sort_index: the last sorted run failed before its file was complete: there is no index of it"); return BMH_EINVAL; }
	std::string s;
	RCK(h->last.out.ix.bytes(base_offset, s));                    // (.bai or .csi: the format the run was made under)
	uint8_t *o = (uint8_t *)malloc(s.size() + 1);
	if (!o) { bmh_set_error("bmh_aligner_sort_index: out of memory"); return BMH_ENOMEM; }
	memcpy(o, s.data(), s.size());
	*bai = o; *bai_bytes = s.size();
	return BMH_OK;
}

uint64_t bmh_aligner_host_tail_batches(const bmh_aligner_t *h)
{
	return h ? h->host_tail_batches : 0;
}

void bmh_aligner_free(bmh_aligner_t *h)
{
	if (!h) return;
	int prev = 0;
	const bool sw = h->dev >= 0 && hipGetDevice(&prev) == hipSuccess && prev != h->dev && hipSetDevice(h->dev) == hipSuccess;
	h->lanes.clear(); h->pool.clear(); h->fbatches.clear();                 // (device and pinned buffers, streams: released on their device)
	if (sw) (void)hipSetDevice(prev);
	delete h;
}

// where the batches of a run come from: a read set in host memory cut at given places, or a read file cut and filled by a loader thread
struct batch_t { uint32_t index = 0; const bmh_read_set_t *rs = nullptr; uint32_t b0 = 0, b1 = 0; int64_t id0 = 0; bool pinned = false; void *token = nullptr; int group = -1; };
struct batch_src_t {
	std::function<int(batch_t &)> next;               // 1: a batch (in index order over the callers), 0: no more, < 0: an error (message set); thread-safe, may block
	std::function<void(void *)> release;              // the text of the batch with this token has been written
	std::function<void()> stop;                       // the run failed: stop producing, unblock next()
};

// ---- the output stage: what becomes of a finished batch's records.  One per run, its format the aligner's (h->a.out_fmt) when the run begins: SAM text and BAM members
// go to the sink batch by batch; the runs of a sorted BAM are kept (h->store) and merged into the file at the end of the input.  A batch comes as its lane left it --
// written on the device (R.text: text, members or a sorted run) -- or as the host formatter's parts of SAM text.  Not BMH_OK: the run fails, the message is set
struct out_stage_t {
	bmh_aligner *h; const int fmt; bmh_sam_sink_t sink; void *user; int n_threads; const char *fn;
	uint64_t n_bytes = 0;                                           // handed to the sink so far
	int lib_of(int group) const { return group >= 0 && (size_t)group < h->a.next.P.table.lib.size() ? (int)h->a.next.P.table.lib[(size_t)group] : -1; }
	int emit(const void *p, size_t n) { if (n && sink(user, (const char *)p, n) != 0) { bmh_set_error("the sink refused the text"); return BMH_EINVAL; } n_bytes += n; return BMH_OK; }
	// a sorted run begins: `last` becomes this run's -- the aligner's plan as it stands (the run's read groups are in it), an index without records, nothing valid --
	// and the places of its counts are its own
	int begin()
	{
		if (fmt != BMH_OUT_BAM_SORTED) return BMH_OK;
		h->store.clear();
		h->last = {h->a.next};
		bmh_aligner::last_t &T = h->last; bdp_plan_t &P = T.out.P;
		const uint32_t n_lib = T.out.markdup ? P.table.n_lib : 0;
		T.lib_counts.assign((size_t)BDP_N_COUNTS * n_lib, 0); T.lib_opt.assign(P.optical() ? (size_t)BDP_OPT_N * n_lib : 0, 0);
		T.out.dup_counts = T.counts.counts; P.lib_counts = n_lib ? T.lib_counts.data() : nullptr; P.no_barcode = &T.counts.no_barcode;
		P.opt.out = T.counts.optical; P.opt.lib_out = n_lib ? T.lib_opt.data() : nullptr; P.grp.out = T.counts.grouped; P.grp.lib_out = nullptr;
		return BMH_OK;
	}
	int device_batch(const result_t &R)
	{
		if (fmt != BMH_OUT_BAM_SORTED) return emit(R.text.p, (size_t)R.text_len);
		if (!R.n_rec) return BMH_OK;
		bsr_dup_t bd = {R.stpl.p, R.dup_e.p, R.dup_info[0], R.dup_info[2], R.dup_info[3], lib_of(R.group)};
		if (h->a.next.markdup && h->a.per_read) { bd.lib3 = R.lib3.p; bd.n_lib3 = h->a.next.P.table.n_lib; }
		if (h->a.next.P.optical()) bd.locs = R.dup_l.p;
		if (h->a.next.P.barcode()) bd.bcs = R.dup_b.p;
		if (h->a.next.markdup) h->last.out.dup_ms[2] += (double)R.dup_d2h;
		return h->store.append((const uint8_t *)R.text.p, R.text_len, R.skeys.p, R.soff.p, R.n_rec, h->a.next.markdup ? &bd : nullptr);      // a sorted run: kept until the end of the input
	}
	int host_batch(const std::vector<std::string> &parts, int group)
	{
		if (fmt == BMH_OUT_SAM) { for (const std::string &part : parts) RCK(emit(part.data(), part.size())); return BMH_OK; }
		// BAM: the text through the two host cores, the same records and members (sorted: the same run) as the device's
		const aligner_t &A = h->a;
		std::string all;
		for (const std::string &part : parts) all += part;
		uint8_t *bam = nullptr, *mem = nullptr; uint64_t bb = 0, mb = 0; uint32_t *st = nullptr, nrec = 0, r = 0;
		int rc = bmh_sam_to_bam_host(all.data(), all.size(), A.n_contigs, A.ctg_blob.data(), A.ctg_noff.data(), n_threads, &bam, &bb, &st, &nrec);
		while (rc == BMH_OK && r < nrec && !st[r]) ++r;
		if (rc == BMH_OK && r < nrec) {                              // the first refused record: line r of the text, its name the line's first field
			const char *a = all.data(), *const end = a + all.size();
			for (uint32_t k = 0; k < r; ++k) a = (const char *)memchr(a, '\n', (size_t)(end - a)) + 1;
			const char *e = a;
			while (e < end && e - a < 254 && *e != '\t' && *e != '\n') ++e;
			rc = bam_refused(std::string(a, e), st[r]);
		}
		if (rc == BMH_OK && fmt == BMH_OUT_BAM_SORTED) {
			std::vector<uint64_t> off, keys, soff(1, 0); std::vector<uint32_t> ord; std::vector<uint8_t> srt;
			rc = bsr_walk(bam, bb, A.n_contigs, off, fn);
			if (rc == BMH_OK) {
				bsr_sort_host(bam, off, keys, ord);
				srt.reserve((size_t)bb + 1);
				for (uint32_t i : ord) { srt.insert(srt.end(), bam + off[i], bam + off[i + 1]); soff.push_back(srt.size()); }
				std::vector<uint32_t> tpl, stpl; std::vector<bdp_entry_t> E; std::vector<bdp_loc_t> locs; std::vector<uint64_t> bcs; uint64_t info[2] = {0, 0};
				const bool optical = A.next.P.optical() != nullptr, barcode = A.next.P.barcode() != nullptr;
				if (A.next.markdup) {                                   // the host forms of the device's heads, ordinals and entries
					rc = bdp_entries_host(bam, off.data(), (uint32_t)ord.size(), tpl, E, info, fn, A.next.P, optical ? &locs : nullptr, barcode ? &bcs : nullptr);
					for (uint32_t i : ord) stpl.push_back(tpl[i]);
				}
				bsr_dup_t bd = {stpl.data(), E.data(), (uint32_t)E.size(), info[0], info[1], lib_of(group)};
				if (optical) bd.locs = locs.data();
				if (barcode) bd.bcs = bcs.data();
				std::vector<uint32_t> lib3;
				if (rc == BMH_OK && A.next.markdup && A.per_read) {        // the host form of bdp_batch_lib_counts_device
					std::vector<uint64_t> lc((size_t)BDP_N_COUNTS * A.next.P.table.n_lib, 0);
					bdp_lib_tally_host(bam, off.data(), (uint32_t)ord.size(), tpl.data(), E.data(), E.size(), A.next.P.table.n_lib, lc.data());
					for (uint32_t l = 0; l < A.next.P.table.n_lib; ++l) for (int k = 0; k < 3; ++k) lib3.push_back((uint32_t)lc[(size_t)BDP_N_COUNTS * l + BDP_SECSUP + k]);
					bd.lib3 = lib3.data(); bd.n_lib3 = A.next.P.table.n_lib;
				}
				if (rc == BMH_OK && !ord.empty()) rc = h->store.append(srt.data(), bb, keys.data(), soff.data(), ord.size(), A.next.markdup ? &bd : nullptr);
			}
		} else if (rc == BMH_OK) {
			rc = bmh_bgzf_deflate_host(bam, bb, A.out_level, n_threads, &mem, &mb);
			if (rc == BMH_OK) rc = emit(mem, (size_t)mb);
		}
		bmh_free(bam); bmh_free(st); bmh_free(mem);
		return rc;
	}
	// the end of the input.  Sorted: every run's keys sorted once more, the file written window by window (csrc/bam_sort_kernels.hip), on the first lane's stream
	static int forward(void *u, const char *b, size_t n) { out_stage_t *o = (out_stage_t *)u; o->n_bytes += n; return o->sink(o->user, b, n); }
	int end(bool trace)
	{
		if (fmt != BMH_OUT_BAM_SORTED) return BMH_OK;
		lane_t &L0 = *h->lanes[0]; bsr_out_t &J = h->last.out;
		int rc = BMH_OK;
		if (!L0.bam && !(L0.bam = bmh_bam_ws_create())) rc = BMH_ENOMEM;
		if (rc == BMH_OK && !L0.bsr && !(L0.bsr = bsr_dev_create())) rc = BMH_ENOMEM;
		const double tm0 = now_s();
		if (rc == BMH_OK) rc = bsr_write_device(L0.bsr, L0.bam, h->store, J, L0.st, forward, this, fn);
		if (trace && J.stats) fprintf(stderr, "[aligner] statistics: the kernels of %.0f windows took %.2f ms on the device, %.3f ms per window\n", J.stats_ms[1], J.stats_ms[0], J.stats_ms[0] / (J.stats_ms[1] > 0 ? J.stats_ms[1] : 1));
		if (trace && J.recal) fprintf(stderr, "[aligner] recalibration table: the kernels of %.0f windows took %.2f ms on the device, %.3f ms per window\n", J.recal_ms[1], J.recal_ms[0], J.recal_ms[0] / (J.recal_ms[1] > 0 ? J.recal_ms[1] : 1));
		if (trace && J.requal) fprintf(stderr, "[aligner] qualities recalibrated: the kernels of %.0f windows took %.2f ms on the device, %.3f ms per window\n", J.requal_ms[1], J.requal_ms[0], J.requal_ms[0] / (J.requal_ms[1] > 0 ? J.requal_ms[1] : 1));
		if (trace && J.coverage) fprintf(stderr, "[aligner] coverage: the depth steps of %.0f windows took %.2f ms on the device, %.3f ms per window (tile %llu, %llu bins)\n", J.cov_ms[1], J.cov_ms[0], J.cov_ms[0] / (J.cov_ms[1] > 0 ? J.cov_ms[1] : 1), (unsigned long long)J.CP.tile, (unsigned long long)J.CP.n_bins());
		if (trace && J.markdup) fprintf(stderr, "[aligner] duplicate marking: %.0f bytes of ordinals and entries came down with the batches\n", J.dup_ms[2]);
		if (trace) fprintf(stderr, "[aligner] sorted output: %zu runs (%llu spilled) merged in %.1f ms\n", h->store.runs.size(), (unsigned long long)h->store.spilled, (now_s() - tm0) * 1e3);
		h->store.clear();
		h->last.valid = rc == BMH_OK;                                 // (the index and the results are those of a whole file, or of none)
		return rc;
	}
};

// a batch whose text the device did not write (the A/B and cross-check forms of run_batch), through the host formatter: its text in `parts`
static bool format_on_host(const aligner_t &A, const result_t &R, bool paired, std::vector<std::string> &parts)
{
	const bmh_read_set_t *rs = R.rs;
	bmh_post_opt_t po = A.po; po.id0 = R.id0; po.rg_id = A.rg_of(R.group);
	const uint64_t a0 = rs->offs[R.b0];
	std::vector<uint64_t> offs64(R.n), noff(R.n);
	const uint64_t n0 = rs->name_offs[R.b0];
	for (uint32_t r = 0; r < R.n; ++r) { offs64[r] = rs->offs[R.b0 + r] - a0; noff[r] = rs->name_offs[R.b0 + r] - n0; }
	const bool cm = A.po.copy_comment && rs->comments && rs->comment_offs;
	std::vector<uint64_t> coff(cm ? R.n : 0);
	const uint64_t c0 = cm ? rs->comment_offs[R.b0] : 0;
	for (uint32_t r = 0; cm && r < R.n; ++r) coff[r] = rs->comment_offs[R.b0 + r] - c0;
	bmh_cigar_src_t cs;
	if (R.slot.empty()) cs.slot32 = R.slot32.p; else cs.slot64 = R.slot.data();
	cs.aln = R.aln.p; cs.packed = R.packed.p; cs.off = R.off.p;
	const bmh_read_groups_t rgs = A.read_groups(A.per_read ? rs->groups + R.b0 : nullptr);
	return bmh_format_sam_parts(&po, R.n, (const char *)rs->names + n0, noff.data(), rs->codes + a0, offs64.data(), rs->lens + R.b0, A.n_contigs,
	                            A.name_ptr.data(), A.off.data(), R.fin.p, R.opr.p, cs,
	                            paired ? R.h_rec.data() : nullptr, paired ? R.unflag.data() : nullptr, parts,
	                            rs->quals ? rs->quals + a0 : nullptr, cm ? (const char *)rs->comments + c0 : nullptr, cm ? coff.data() : nullptr, A.per_read ? &rgs : nullptr);
}

static int run_core(bmh_aligner_t *h, batch_src_t &src, const char *fn, int paired, int n_lanes, int n_threads, bmh_sam_sink_t sink, void *user, bmh_align_stats_t *stats)
{
	const aligner_t &A = h->a;
	if (n_lanes < 1) n_lanes = 1;
	if (n_threads < 1) n_threads = bmh_effective_cpus();
	// half of the lanes in the path's device stages, the others in their tails (gate_t): measured on 2 / 3 / 4 lanes, single-end and paired, never slower than all of them, +5-7 % with 2 and 4
	gate_t gpu_gate; gpu_gate.cap = bmh_tune("ALIGNER_GPU_SLOTS", n_lanes > 1 ? n_lanes / 2 : 0);
	int dev = 0;
	if (hipGetDevice(&dev) != hipSuccess) { bmh_set_error("%s: no HIP device", fn); return BMH_ENODEV; }
	const double t_start = now_s();
	const bool trace = getenv("BMH_ALIGNER_TRACE") != nullptr;        // per-batch timeline on stderr
	std::mutex mu; std::condition_variable cv;
	std::map<uint32_t, std::unique_ptr<result_t>> done;             // finished batches waiting for their turn at the writer
	std::vector<std::unique_ptr<result_t>> &pool = h->pool;         // result objects (pinned buffers) not in use: at most n_lanes + 2 exist
	int &n_results = h->n_results;
	uint32_t next_write = 0; int workers_alive = n_lanes;           // (guarded by mu)
	uint64_t n_reads_total = 0;
	int first_rc = BMH_OK; std::string first_err;
	auto fail = [&](int rc, const char *msg) { { std::lock_guard<std::mutex> lk(mu); if (first_rc == BMH_OK) { first_rc = rc; first_err = msg ? msg : ""; } cv.notify_all(); } if (src.stop) src.stop(); };
	std::vector<double> lane_t_sum(8, 0.0);
	double copy_sum[2] = {0, 0}; uint64_t copy_bytes_sum[2] = {0, 0};
	if (h->dev >= 0 && h->dev != dev) { bmh_set_error("%s: the aligner's lanes live on device %d, the current device is %d", fn, h->dev, dev); return BMH_EINVAL; }
	h->dev = dev;
	while ((int)h->lanes.size() < n_lanes) {
		std::unique_ptr<lane_t> ln(new lane_t());
		if (hipStreamCreateWithFlags(&ln->st, hipStreamNonBlocking) != hipSuccess || hipStreamCreateWithFlags(&ln->st2, hipStreamNonBlocking) != hipSuccess) {
			bmh_set_error("%s: hipStreamCreate: %s", fn, hipGetErrorString(hipGetLastError())); return BMH_ENODEV;
		}
		{
			const char *pe = getenv("BMH_ALIGNER_TAIL_PRIO");          // (BMH_ALIGNER_TAIL_PRIO=normal: A/B -- everything on the lane's own stream)
			int prio_lo = 0, prio_hi = 0;
			(void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
			if (!(pe && pe[0] == 'n') && hipStreamCreateWithPriority(&ln->st_hi, hipStreamNonBlocking, prio_hi) != hipSuccess) {
				bmh_set_error("%s: hipStreamCreateWithPriority: %s", fn, hipGetErrorString(hipGetLastError())); return BMH_ENODEV;
			}
		}
		h->lanes.push_back(std::move(ln));
	}
	for (auto &ln : h->lanes) { for (double &v : ln->t) v = 0.0; ln->copy_ms[0] = ln->copy_ms[1] = 0.0; ln->copy_bytes[0] = ln->copy_bytes[1] = 0; ln->host_tail = 0; }
	h->host_tail_batches = 0;
	out_stage_t out = {h, A.out_fmt, sink, user, n_threads, fn};
	RCK(out.begin());
	auto worker = [&](int lane_index) {
		if (hipSetDevice(dev) != hipSuccess) { fail(BMH_ENODEV, "hipSetDevice failed in a worker thread"); return; }
		lane_t &Ln = *h->lanes[(size_t)lane_index];
		for (;;) {
			batch_t bt;
			const int got = src.next(bt);
			if (got < 0) { fail(got, bmh_last_error()); break; }
			if (got == 0) break;
			const uint32_t b = bt.index;
			std::unique_ptr<result_t> R;
			{   // a result object from the pool: no more than n_lanes + 2 batches are ahead of the writer (their text is hundreds of megabytes each); the
				// batch the writer waits for always gets one
				std::unique_lock<std::mutex> lk(mu);
				n_reads_total += bt.b1 - bt.b0;
				cv.wait(lk, [&] { return first_rc != BMH_OK || !pool.empty() || n_results < n_lanes + 2 || b == next_write; });
				if (first_rc != BMH_OK) { if (src.release) src.release(bt.token); break; }
				if (!pool.empty()) { R = std::move(pool.back()); pool.pop_back(); }
				else { R.reset(new result_t()); ++n_results; }
			}
			R->token = bt.token;
			int rc = BMH_OK;
			const double tb0 = now_s();
			if (bt.b1 > bt.b0) rc = run_batch(A, Ln, *bt.rs, bt.b0, bt.b1, bt.id0, bt.group, bt.pinned, paired != 0, n_threads, gpu_gate, *R);
			else { R->b0 = bt.b0; R->n = 0; R->rs = bt.rs; R->id0 = bt.id0; R->group = bt.group; R->has_text = false; }
			if (trace) fprintf(stderr, "[aligner] lane %d batch %u: %.1f .. %.1f ms\n", lane_index, b, (tb0 - t_start) * 1e3, (now_s() - t_start) * 1e3);
			if (rc != BMH_OK) { if (src.release) src.release(bt.token); fail(rc, bmh_last_error()); break; }
			std::lock_guard<std::mutex> lk(mu);
			done[b] = std::move(R);
			cv.notify_all();
		}
		std::lock_guard<std::mutex> lk(mu);
		for (int k = 0; k < 8; ++k) lane_t_sum[(size_t)k] += Ln.t[k];
		for (int k = 0; k < 2; ++k) { copy_sum[k] += Ln.copy_ms[k]; copy_bytes_sum[k] += Ln.copy_bytes[k]; }
		--workers_alive;                                             // (the writer ends when every worker has: a batch that was taken is in `done` by then)
		cv.notify_all();
	};
	double t_format = 0.0; uint32_t n_written = 0;
	auto writer = [&]() {
		std::vector<std::string> &parts = h->parts;                  // (kept with the aligner: their capacity is the text of a batch)
		for (uint32_t b = 0;; ++b) {
			std::unique_ptr<result_t> R;
			{
				std::unique_lock<std::mutex> lk(mu);
				cv.wait(lk, [&] { return first_rc != BMH_OK || done.count(b) || workers_alive == 0; });
				if (first_rc != BMH_OK) return;
				if (!done.count(b)) return;                             // (every batch written)
				R = std::move(done[b]); done.erase(b);
			}
			if (R->n) {                                              // written on the device: nothing to format; else the host formatter first
				const double t0 = now_s();
				if (!R->has_text) {
					if (!format_on_host(A, *R, paired != 0, parts)) { fail(BMH_EINVAL, bmh_last_error()); return; }
					t_format += now_s() - t0;
				}
				const double ts0 = now_s();
				const int rc = R->has_text ? out.device_batch(*R) : out.host_batch(parts, R->group);
				if (rc != BMH_OK) { fail(rc, bmh_last_error()); return; }
				if (trace && R->has_text) fprintf(stderr, "[aligner] writer batch %u: text of the device, sink %.1f .. %.1f ms\n", b, (ts0 - t_start) * 1e3, (now_s() - t_start) * 1e3);
				else if (trace) fprintf(stderr, "[aligner] writer batch %u: format %.1f .. %.1f ms, sink .. %.1f\n", b, (t0 - t_start) * 1e3, (ts0 - t_start) * 1e3, (now_s() - t_start) * 1e3);
			}
			if (src.release) src.release(R->token);
			R->token = nullptr; R->rs = nullptr;
			std::lock_guard<std::mutex> lk(mu);
			next_write = b + 1; ++n_written;
			pool.push_back(std::move(R));
			cv.notify_all();
		}
	};
	{
		std::vector<std::thread> th;
		for (int k = 0; k < n_lanes; ++k) th.emplace_back(worker, k);
		std::thread wt(writer);
		for (auto &t : th) t.join();
		wt.join();
	}
	if (src.release) for (auto &kv : done) if (kv.second) src.release(kv.second->token);       // (a failed run: what was waiting for the writer)
	n_results = (int)pool.size();                                   // (after a failed run the results that were in flight are gone)
	for (auto &ln : h->lanes) h->host_tail_batches += ln->host_tail;
	if (first_rc != BMH_OK) { h->store.clear(); bmh_set_error("%s", first_err.c_str()); return first_rc; }
	const double te = now_s();
	RCK(out.end(trace));
	t_format += now_s() - te;
	if (stats) {
		stats->n_reads = n_reads_total; stats->n_bytes = out.n_bytes; stats->n_batches = n_written; stats->n_lanes = n_lanes;
		stats->seconds = now_s() - t_start; stats->format_seconds = t_format;
		stats->h2d_seconds = lane_t_sum[0]; stats->seed_seconds = lane_t_sum[1]; stats->chain_extend_seconds = lane_t_sum[2]; stats->tail_seconds = lane_t_sum[3];
		stats->select_seconds = lane_t_sum[4]; stats->cigar_seconds = lane_t_sum[5]; stats->gate_wait_seconds = lane_t_sum[6];
		stats->h2d_copy_seconds = copy_sum[0] * 1e-3; stats->d2h_copy_seconds = copy_sum[1] * 1e-3; stats->h2d_bytes = copy_bytes_sum[0]; stats->d2h_bytes = copy_bytes_sum[1];
	}
	return BMH_OK;
}

// page-locks (registers) a caller's host buffer so that the device copies straight out of it / releases it; what bmh_aligner_run does with a read set whose
// letters lie in such memory: no staging copy
int bmh_host_pin(void *p, size_t bytes)
{
	if (!p || !bytes) { bmh_set_error("bmh_host_pin: null argument"); return BMH_EINVAL; }
	const hipError_t e = hipHostRegister(p, bytes, hipHostRegisterDefault);
	if (e != hipSuccess) { bmh_set_error("bmh_host_pin: hipHostRegister of %zu bytes: %s", bytes, hipGetErrorString(e)); (void)hipGetLastError(); return BMH_ENODEV; }
	return BMH_OK;
}
int bmh_host_unpin(void *p)
{
	if (!p) return BMH_OK;
	const hipError_t e = hipHostUnregister(p);
	if (e != hipSuccess) { bmh_set_error("bmh_host_unpin: %s", hipGetErrorString(e)); (void)hipGetLastError(); return BMH_ENODEV; }
	return BMH_OK;
}

int bmh_aligner_run(bmh_aligner_t *h, const bmh_read_set_t *rs, const uint64_t *cuts, uint32_t n_batches, int paired, int n_lanes, int n_threads,
                    bmh_sam_sink_t sink, void *user, bmh_align_stats_t *stats)
{
	if (!h || !rs || !cuts || !sink) { bmh_set_error("bmh_aligner_run: null argument"); return BMH_EINVAL; }
	if (stats) memset(stats, 0, sizeof(*stats));
	if (h->keep_rg) { bmh_set_error("bmh_aligner_run: the input's read groups are kept (bmh_aligner_set_keep_rg): that takes a BAM file (bmh_aligner_run_files), not reads in memory"); return BMH_EINVAL; }
	if (n_batches == 0 || rs->n_reads == 0) return BMH_OK;
	// (the device path reads ascii / offs / lens only, but the host forms -- the pairs' walks, the host tail after BMH_ECAPACITY, the host formatter -- read every array)
	if (!rs->ascii || !rs->codes || !rs->offs || !rs->lens || !rs->names || !rs->name_offs) { bmh_set_error("bmh_aligner_run: the read set lacks one of ascii / codes / offs / lens / names / name_offs"); return BMH_EINVAL; }
	if (cuts[0] != 0 || cuts[n_batches] != rs->n_reads) { bmh_set_error("bmh_aligner_run: cuts[0] = 0 and cuts[n_batches] = n_reads are required"); return BMH_EINVAL; }
	for (uint32_t b = 0; b < n_batches; ++b)
		if (cuts[b + 1] < cuts[b] || (paired && ((cuts[b + 1] - cuts[b]) & 1)) || cuts[b + 1] - cuts[b] > 0xFFFFFFF0ull) { bmh_set_error("bmh_aligner_run: bad batch cuts"); return BMH_EINVAL; }
	for (uint64_t r = 0; r < rs->n_reads; ++r)
		if (rs->lens[r] > BMH_EXT_LONG_MAX) { bmh_set_error("bmh_aligner_run: read %llu has %u bases: the longest read the aligner takes has %d (BMH_EXT_LONG_MAX)", (unsigned long long)r, rs->lens[r], BMH_EXT_LONG_MAX); return BMH_EINVAL; }
	if ((uint32_t)n_lanes > n_batches) n_lanes = (int)n_batches;
	// the letters in pinned or registered host memory (hipHostMalloc, hipHostRegister / bmh_host_pin): the batches go to the device straight from there --
	// no staging copy into the lane's pinned buffer on host threads
	bool ascii_pinned = false;
	{
		hipPointerAttribute_t pa; memset(&pa, 0, sizeof(pa));
		const uint8_t *last = rs->ascii + (rs->n_bases ? rs->n_bases - 1 : 0);
		if (hipPointerGetAttributes(&pa, rs->ascii) == hipSuccess && pa.type == hipMemoryTypeHost) {
			hipPointerAttribute_t pb; memset(&pb, 0, sizeof(pb));
			ascii_pinned = hipPointerGetAttributes(&pb, last) == hipSuccess && pb.type == hipMemoryTypeHost;
		}
		(void)hipGetLastError();                                   // (an ordinary pointer: the query fails, and that is the answer)
	}
	std::atomic<uint32_t> next_batch{0};
	batch_src_t src;
	src.next = [&](batch_t &bt) {
		const uint32_t b = next_batch.fetch_add(1);
		if (b >= n_batches) return 0;
		bt.index = b; bt.rs = rs; bt.b0 = (uint32_t)cuts[b]; bt.b1 = (uint32_t)cuts[b + 1]; bt.id0 = (int64_t)cuts[b]; bt.pinned = ascii_pinned; bt.token = nullptr;
		return 1;
	};
	return run_core(h, src, "bmh_aligner_run", paired, n_lanes, n_threads, sink, user, stats);
}

// ---- the same from read FILES, batch by batch: a loader thread (batch_queue.h) fills every batch into pinned host memory (fbatch_t) while the lanes are on the batches
// before it; nothing of the file is held beyond the batches in flight (n_lanes + 3 of them).  A batch ends the way the reference's bseq_read ends one (reads are added
// until it holds at least batch_bases bases -- or exactly batch_reads reads if that is not 0 -- and, paired, an even number of reads; src/bwa.c:48-66).

// the arguments every such run checks, and the clamps of the batch's size
static int file_run_args(const char *fn, bmh_aligner_t *h, const char *path, bmh_sam_sink_t sink, bmh_align_stats_t *stats, uint64_t &batch_bases, uint64_t &batch_reads, int paired, int &n_lanes, int &n_threads)
{
	if (!h || !path || !sink) { bmh_set_error("%s: null argument", fn); return BMH_EINVAL; }
	if (stats) memset(stats, 0, sizeof(*stats));
	if (batch_bases == 0 && batch_reads == 0) { bmh_set_error("%s: batch_bases or batch_reads must be given", fn); return BMH_EINVAL; }
	if (batch_bases >= (1ull << 31) - 4096) batch_bases = (1ull << 31) - 4096;      // offsets inside a batch are 32-bit
	if (paired && (batch_reads & 1)) --batch_reads;
	if (n_lanes < 1) n_lanes = 1;
	if (n_threads < 1) n_threads = bmh_effective_cpus();
	return BMH_OK;
}

// what the loaders refuse of a batch: an odd number of reads in a paired file; once it is filled, a read longer than the aligner takes.  Else 1: the batch's place in the run
static int even_batch(const char *fn, int paired, uint64_t nr) { if (paired && (nr & 1)) { bmh_set_error("%s: an odd number of reads in a paired file", fn); return BMH_EINVAL; } return BMH_OK; }
static int accept_batch(const char *fn, int paired, fbatch_t &fb, int64_t &id0)
{
	const uint64_t nr = fb.rs.n_reads;
	RCK(even_batch(fn, paired, nr));
	for (uint64_t r = 0; r < nr; ++r)
		if (fb.lens.p[r] > BMH_EXT_LONG_MAX) { bmh_set_error("%s: read %lld has %u bases: the longest read the aligner takes has %d (BMH_EXT_LONG_MAX)", fn, (long long)(id0 + (int64_t)r), fb.lens.p[r], BMH_EXT_LONG_MAX); return BMH_EINVAL; }
	fb.id0 = id0; id0 += (int64_t)nr;
	return 1;
}

// the run: `fill` (1: fb holds the next batch, 0: the end, < 0: refused, the message set) on the loader thread, the lanes behind it.  after_release: a refusal fails
// the run only when the batches before it have been written (a file that ends before its mate file: the complete pairs first); else as soon as the lanes reach it
static int run_loaded(bmh_aligner_t *h, const char *fn, int dev, const std::function<int(fbatch_t &)> &fill, bool after_release, int paired, int n_lanes, int n_threads,
                      bmh_sam_sink_t sink, void *user, bmh_align_stats_t *stats)
{
	batch_queue_t<fbatch_t> q(h->fbatches, n_lanes + 3, after_release);
	batch_src_t src;
	src.next = [&](batch_t &bt) {
		fbatch_t *fb = nullptr; std::string err;
		const int got = q.next(&fb, err);
		if (got < 0) bmh_set_error("%s", err.c_str());
		if (got == 1) { bt.index = fb->index; bt.rs = &fb->rs; bt.b0 = 0; bt.b1 = (uint32_t)fb->rs.n_reads; bt.id0 = fb->id0; bt.pinned = true; bt.token = fb; bt.group = fb->group; }
		return got;
	};
	src.release = [&](void *tok) { q.release((fbatch_t *)tok); };
	src.stop = [&]() { q.stop(); };
	q.start([&](fbatch_t &fb, std::string &err) { const int rc = fill(fb); if (rc < 0) err = bmh_last_error(); return rc; },
	        [dev](std::string &err) { if (hipSetDevice(dev) == hipSuccess) return (int)BMH_OK; err = "hipSetDevice failed in the loader thread"; return (int)BMH_ENODEV; });
	const int rc = run_core(h, src, fn, paired, n_lanes, n_threads, sink, user, stats);
	q.join();
	return rc;
}

// one FASTA file (bmh_aligner_run_fasta) or, either: one FASTA or FASTQ file (bmh_aligner_run_file), one record per line group: the mapped file cut and filled on
// host threads (csrc/reads_io.cpp: bmh_fasta_cut / bmh_fasta_fill); fn: the entry point's name in messages
static int run_file(bmh_aligner_t *h, const char *path, uint64_t batch_bases, uint64_t batch_reads, int paired, int n_lanes, int n_threads,
                    bmh_sam_sink_t sink, void *user, bmh_align_stats_t *stats, bool either, const char *fn)
{
	RCK(file_run_args(fn, h, path, sink, stats, batch_bases, batch_reads, paired, n_lanes, n_threads));
	if (h->keep_rg) { bmh_set_error("%s: the input's read groups are kept (bmh_aligner_set_keep_rg): that takes a BAM file (bmh_aligner_run_files); text input carries none", fn); return BMH_EINVAL; }
	const uint8_t *buf = nullptr; size_t sz = 0;
	RCK(bmh_map_file(fn, path, &buf, &sz));
	if (sz == 0) return BMH_OK;
	bmh_reads_fmt_t fmt;
	fmt.either = either;
	fmt.fq = either && bmh_reads_detect(buf, sz);
	fmt.comments = either && h->a.po.copy_comment;        // (the comments are read only when the records carry them)
	int dev = 0;
	if (hipGetDevice(&dev) != hipSuccess) { (void)munmap((void *)buf, sz); bmh_set_error("%s: no HIP device", fn); return BMH_ENODEV; }
	const int load_threads = n_threads < 8 ? n_threads : 8;
	size_t p = 0, est = 0; int64_t id0 = 0;                 // where the next batch begins, the last one's size in the file, its first read's index in the run
	auto fill = [&](fbatch_t &fb) {
		while (p < sz) {
			size_t end = sz; uint64_t nr = 0, nb = 0, nn = 0, ncm = 0;
			RCK(bmh_fasta_cut(buf, sz, p, batch_bases, batch_reads, /* even counts, as bseq_read ends its batches */ batch_reads == 0, load_threads, est, &end, &nr, &nb, &nn, fmt, &ncm));
			if (nr == 0) { p = end; continue; }
			RCK(even_batch(fn, paired, nr));                        // (before anything is allocated for it)
			memset(&fb.rs, 0, sizeof(fb.rs));
			RCK(fb.size(fn, nr, nb, nn, ncm, fmt.fq, fmt.comments, &fb.rs));
			RCK(bmh_fasta_fill(buf, p, end, nr, nb, nn, load_threads, &fb.rs, fmt, ncm));
			est = end - p; p = end;
			fb.group = -1;
			return accept_batch(fn, paired, fb, id0);
		}
		return 0;
	};
	const int rc = run_loaded(h, fn, dev, fill, false, paired, n_lanes, n_threads, sink, user, stats);
	(void)munmap((void *)buf, sz);
	return rc;
}

}   // extern "C"

// one or two read files of any shape (multi-line, gzip / BGZF, R1 + R2): the loader drives the pump of csrc/reads_parse.hip -- text windows in pinned memory, records
// cut on the device (or walked by the host where the device hands a window back)
int bmh_aligner_run_files(bmh_aligner_t *h, const char *path1, const char *path2, uint64_t batch_bases, uint64_t batch_reads, int paired, int n_lanes, int n_threads,
                          bmh_sam_sink_t sink, void *user, bmh_align_stats_t *stats)
{
	const char *fn = "bmh_aligner_run_files";
	if (path2) paired = 1;
	RCK(file_run_args(fn, h, path1, sink, stats, batch_bases, batch_reads, paired, n_lanes, n_threads));
	int dev = 0;
	if (hipGetDevice(&dev) != hipSuccess) { bmh_set_error("%s: no HIP device", fn); return BMH_ENODEV; }
	const bool cm = h->a.po.copy_comment != 0;
	const bool keep = h->keep_rg;
	if (keep) {                                                        // refused before the file is opened
		if (path2) { bmh_set_error("%s: the input's read groups are kept (bmh_aligner_set_keep_rg) and a mates file was given: such a run takes one BAM file", fn); return BMH_EINVAL; }
		if (h->a.po.rg_id && h->a.po.rg_id[0]) { bmh_set_error("%s: the input's read groups are kept (bmh_aligner_set_keep_rg) and the aligner has a read group of its own ('%s', -R): one or the other", fn, h->a.po.rg_id); return BMH_EINVAL; }
		if (h->a.next.markdup && h->a.n_contigs > (int)BDP_MAX_REF) { bmh_set_error("%s: %d reference sequences: with read groups duplicate marking takes at most 2^24 (the library is the top byte of its key)", fn, h->a.n_contigs); return BMH_EINVAL; }
	}
	// (BMH_READS_HOST=1: the pump's host forms cut every window -- the A/B and cross-check switch of the device parser and the BAM decoder kernels)
	bmh_reads_pump_t *P = bmh_pump_open(path1, path2, n_threads, cm, bmh_tune("READS_HOST", 0) != 0, (size_t)std::max(0, bmh_tune("READS_CHUNK_BYTES", 0)) /* (the tests' small windows; 0: sized by the batch) */, keep, keep && h->a.next.markdup, h->collate, h->collate_mem);
	if (!P) return BMH_EINVAL;
	if (h->collate && bmh_pump_bam_paired(P) < 0) {                    // refused before a batch is read
		bmh_pump_close(P);
		bmh_set_error("reads file: %s: mates are collated by name (--collate) in BAM input only: text input is taken in the order of its records", path1);
		return BMH_EINVAL;
	}
	aligner_t &A = h->a;
	// the run's table is the aligner's until the run is over, whichever way it ends
	struct table_guard_t { aligner_t &A; bool on; ~table_guard_t() { if (on) { A.group_ids.clear(); A.next.P.table = bdp_table_t(); A.per_read = false; ++A.groups_serial; } } } guard{A, false};
	if (keep) {
		// the header was read whole when the pump opened the file: its @RG lines are the run's read groups, and the caller hears of them before the first record
		const bmh_rg_table_t *T = bmh_pump_read_groups(P);
		bdp_table_t G;
		G.id_off.assign(1, 0u);
		for (size_t g = 0; g < T->ids.size(); ++g) { G.ids += T->ids[g]; G.id_off.push_back((uint32_t)G.ids.size()); G.lib.push_back((uint8_t)T->lib[g]); }      // (beyond 255 libraries the byte is not read: no duplicate marking)
		G.n_lib = (uint32_t)T->lib_names.size();
		A.group_ids.assign(T->ids.begin(), T->ids.end()); A.next.P.table = G; A.per_read = true; ++A.groups_serial; guard.on = true;
		if (h->rg_header) {
			std::string lines;
			for (const std::string &l : T->lines) { lines += l; lines += '\n'; }
			if (h->rg_header(h->rg_user, lines.data(), lines.size(), (int)T->lib.size(), T->lib.data()) != 0) { bmh_pump_close(P); bmh_set_error("%s: the caller refused the input's read groups", fn); return BMH_EINVAL; }
		}
	}
	// a BAM file says itself whether it holds pairs (flag 0x1 of its first record kept, known since the file was opened): the run's lanes start with that
	const int bam_pairs = bmh_pump_bam_paired(P);
	if (bam_pairs == 0 && paired) { bmh_pump_close(P); bmh_set_error("reads file: %s: paired reads were asked for and the BAM's records do not carry flag 0x1", path1); return BMH_EINVAL; }
	if (bam_pairs == 1 && !paired) {
		paired = 1;
		if (batch_reads & 1) --batch_reads;
		if (h->bam_pairs_bases && batch_reads == 0) batch_bases = std::min<uint64_t>(h->bam_pairs_bases, (1ull << 31) - 4096);
		if (h->bam_pairs_lanes > 0) n_lanes = h->bam_pairs_lanes;
	}
	int64_t id0 = 0;
	auto fill = [&](fbatch_t &fb) {
		const bmh_batch_alloc_t alloc = [&](uint64_t nr, uint64_t nb, uint64_t nn, uint64_t ncm, bool fq, bmh_read_set_t *rs) { return fb.size(fn, nr, nb, nn, ncm, fq, cm, rs, keep); };
		const int rc = bmh_pump_next(P, batch_bases, batch_reads, /* even counts, as bseq_read ends its batches */ batch_reads == 0, false, alloc, &fb.rs);
		fb.group = -1;                                                 // (the buffers are kept between runs: one of a run over groups still names its group)
		return rc == 1 ? accept_batch(fn, paired, fb, id0) : rc;
	};
	const int rc = run_loaded(h, fn, dev, fill, true, paired, n_lanes, n_threads, sink, user, stats);
	uint64_t cnt[4]; bmh_pump_counts(P, cnt); bmh_reads_note_counts(cnt);
	uint64_t icnt[2]; bmh_pump_inflate_counts(P, icnt); bmh_reads_note_inflate_counts(icnt);
	uint64_t bcnt[2]; bmh_pump_bam_counts(P, bcnt); bmh_reads_note_bam_counts(bcnt);
	uint64_t ccnt[5]; bmh_pump_collate_counts(P, ccnt); bmh_reads_note_collate_counts(ccnt);
	bmh_pump_close(P);
	return rc;
}

// several read groups in one run: the loader opens group g + 1's pump when group g's is at its end and goes on filling the same queue -- the lanes see one
// stream of batches, each with its group (the records' RG:Z, the batch's library), its reads indexed from 0 within the group
int bmh_aligner_run_groups(bmh_aligner_t *h, const bmh_read_group_t *groups, int n_groups, uint64_t batch_bases, uint64_t batch_reads, int paired, int n_lanes, int n_threads,
                           bmh_sam_sink_t sink, void *user, bmh_align_stats_t *stats)
{
	const char *fn = "bmh_aligner_run_groups";
	if (!h || !sink) { bmh_set_error("%s: null argument", fn); return BMH_EINVAL; }
	if (stats) memset(stats, 0, sizeof(*stats));
	if (n_groups < 1 || !groups) { bmh_set_error("%s: no read groups were given", fn); return BMH_EINVAL; }
	if (h->a.po.rg_id && h->a.po.rg_id[0]) { bmh_set_error("%s: the aligner has a read group of its own ('%s', -R): a run over read groups takes them from its groups alone", fn, h->a.po.rg_id); return BMH_EINVAL; }
	if (h->keep_rg) { bmh_set_error("%s: the input's read groups are kept (bmh_aligner_set_keep_rg): that and a run over read groups do not combine", fn); return BMH_EINVAL; }
	std::vector<const char *> ids; std::vector<int32_t> libs;
	int stated = paired ? 1 : 0;                                       // pairs by what the caller says: `paired`, or a group with two files
	for (int g = 0; g < n_groups; ++g) {
		if (!groups[g].id || !groups[g].path1) { bmh_set_error("%s: read group %d lacks its ID or its reads file", fn, g); return BMH_EINVAL; }
		if (strlen(groups[g].id) > 255) { bmh_set_error("%s: read group %d: its ID is longer than 255 characters", fn, g); return BMH_EINVAL; }
		ids.push_back(groups[g].id); libs.push_back(groups[g].library);
		if (groups[g].path2) stated = 1;
	}
	bdp_table_t T;
	RCK(bdp_table_make(T, ids.data(), libs.data(), n_groups, fn));
	if (h->a.next.markdup && h->a.n_contigs > (int)BDP_MAX_REF) { bmh_set_error("%s: %d reference sequences: with read groups duplicate marking takes at most 2^24 (the library is the top byte of its key)", fn, h->a.n_contigs); return BMH_EINVAL; }
	if (h->a.next.P.optical() && n_groups > (int)BDP_OPT_MAX_GROUPS) { bmh_set_error("%s: %d read groups: with an optical distance a run takes at most %d (a location holds its group's row in 16 bits)", fn, n_groups, (int)BDP_OPT_MAX_GROUPS); return BMH_EINVAL; }
	for (int g = 0; g < n_groups; ++g)
		for (const char *path : {groups[g].path1, groups[g].path2}) {
			struct stat sb;
			if (path && stat(path, &sb) != 0) { bmh_set_error("read group '%s': reads file: %s: %s", groups[g].id, path, strerror(errno)); return BMH_EINVAL; }
		}
	RCK(file_run_args(fn, h, groups[0].path1, sink, stats, batch_bases, batch_reads, stated, n_lanes, n_threads));
	int dev = 0;
	if (hipGetDevice(&dev) != hipSuccess) { bmh_set_error("%s: no HIP device", fn); return BMH_ENODEV; }
	const bool cm = h->a.po.copy_comment != 0;
	// the state of the loader: the group being read, its pump, the index of its next read; what the pumps counted
	struct loader_t { bmh_reads_pump_t *P = nullptr; int g = 0; int64_t id0 = 0; uint64_t cnt[4] = {0, 0, 0, 0}, icnt[2] = {0, 0}, bcnt[2] = {0, 0}, ccnt[5] = {0, 0, 0, 0, 0}; } ld;
	auto named = [&](int g) { const std::string m = bmh_last_error(); bmh_set_error("read group '%s': %s", groups[g].id, m.c_str()); return (int)BMH_EINVAL; };
	auto close_pump = [&]() {
		if (!ld.P) return;
		uint64_t c[4], ic[2], bc[2];
		bmh_pump_counts(ld.P, c); bmh_pump_inflate_counts(ld.P, ic); bmh_pump_bam_counts(ld.P, bc);
		for (int k = 0; k < 4; ++k) ld.cnt[k] += c[k];
		for (int k = 0; k < 2; ++k) { ld.icnt[k] += ic[k]; ld.bcnt[k] += bc[k]; }
		uint64_t cc[5]; bmh_pump_collate_counts(ld.P, cc);             // (counts add up over the groups, peaks are the largest)
		ld.ccnt[0] += cc[0]; ld.ccnt[1] += cc[1]; ld.ccnt[2] = std::max(ld.ccnt[2], cc[2]); ld.ccnt[3] = std::max(ld.ccnt[3], cc[3]); ld.ccnt[4] += cc[4];
		bmh_pump_close(ld.P); ld.P = nullptr;
	};
	// group g's pump; *pairs: does the group hold pairs (two files, a BAM with flag 0x1, else what `paired` says)
	auto open_pump = [&](int g, int *pairs) -> int {
		ld.P = bmh_pump_open(groups[g].path1, groups[g].path2, n_threads, cm, false, (size_t)std::max(0, bmh_tune("READS_CHUNK_BYTES", 0)), false, false, h->collate && !groups[g].path2, h->collate_mem);     // (a group of text files is taken as ever)
		if (!ld.P) return named(g);
		const int bam_pairs = bmh_pump_bam_paired(ld.P);
		if (bam_pairs == 0 && paired) { bmh_set_error("read group '%s': reads file: %s: paired reads were asked for and the BAM's records do not carry flag 0x1", groups[g].id, groups[g].path1); return BMH_EINVAL; }
		*pairs = groups[g].path2 || bam_pairs == 1 || (bam_pairs < 0 && paired) ? 1 : 0;
		ld.g = g; ld.id0 = 0;
		return BMH_OK;
	};
	int run_pairs = 0;
	int rc = open_pump(0, &run_pairs);
	if (rc != BMH_OK) { close_pump(); return rc; }
	if (run_pairs && !stated) {                                        // (the first group is a BAM that holds pairs: bmh_aligner_run_files' choices for that case)
		if (batch_reads & 1) --batch_reads;
		if (h->bam_pairs_bases && batch_reads == 0) batch_bases = std::min<uint64_t>(h->bam_pairs_bases, (1ull << 31) - 4096);
		if (h->bam_pairs_lanes > 0) n_lanes = h->bam_pairs_lanes;
	}
	auto fill = [&](fbatch_t &fb) -> int {
		for (;;) {
			if (!ld.P) {
				if (ld.g + 1 >= n_groups) return 0;
				int pairs = 0;
				RCK(open_pump(ld.g + 1, &pairs));
				if (pairs != run_pairs) {
					bmh_set_error("read group '%s': reads file: %s: the group holds %s and the groups before it %s (all groups of a run hold pairs, or none does)", groups[ld.g].id, groups[ld.g].path1,
					              pairs ? "pairs" : "single-end reads", run_pairs ? "pairs" : "single-end reads");
					return BMH_EINVAL;
				}
			}
			const bmh_batch_alloc_t alloc = [&](uint64_t nr, uint64_t nb, uint64_t nn, uint64_t ncm, bool fq, bmh_read_set_t *rs) { return fb.size(fn, nr, nb, nn, ncm, fq, cm, rs); };
			int got = bmh_pump_next(ld.P, batch_bases, batch_reads, /* even counts, as bseq_read ends its batches */ batch_reads == 0, false, alloc, &fb.rs);
			if (got == 1) { fb.group = ld.g; got = accept_batch(fn, run_pairs, fb, ld.id0); }
			if (got < 0) return named(ld.g);
			if (got == 1) return 1;
			close_pump();                                              // the group's end: the next group's first batch follows in the same queue
		}
	};
	aligner_t &A = h->a;
	A.group_ids.assign(ids.begin(), ids.end()); A.next.P.table = T; ++A.groups_serial;
	rc = run_loaded(h, fn, dev, fill, true, run_pairs, n_lanes, n_threads, sink, user, stats);
	A.group_ids.clear(); A.next.P.table = bdp_table_t(); ++A.groups_serial;
	close_pump();
	bmh_reads_note_counts(ld.cnt); bmh_reads_note_inflate_counts(ld.icnt); bmh_reads_note_bam_counts(ld.bcnt); bmh_reads_note_collate_counts(ld.ccnt);
	return rc;
}

int bmh_aligner_set_keep_rg(bmh_aligner_t *h, int on, bmh_rg_header_fn header, void *user)
{
	if (!h) { bmh_set_error("bmh_aligner_set_keep_rg: null aligner"); return BMH_EINVAL; }
	h->keep_rg = on != 0; h->rg_header = on ? header : nullptr; h->rg_user = on ? user : nullptr;
	return BMH_OK;
}

int bmh_aligner_set_collate(bmh_aligner_t *h, int on, uint64_t mem_bytes)
{
	if (!h) { bmh_set_error("bmh_aligner_set_collate: null aligner"); return BMH_EINVAL; }
	if (!on && mem_bytes) { bmh_set_error("bmh_aligner_set_collate: a cap of %llu bytes (--collate-mem) without --collate: the cap is that of the collation's open records", (unsigned long long)mem_bytes); return BMH_EINVAL; }
	h->collate = on != 0; h->collate_mem = mem_bytes;
	return BMH_OK;
}

int bmh_aligner_set_bam_pairs(bmh_aligner_t *h, uint64_t batch_bases, int n_lanes)
{
	if (!h) { bmh_set_error("bmh_aligner_set_bam_pairs: null aligner"); return BMH_EINVAL; }
	h->bam_pairs_bases = batch_bases; h->bam_pairs_lanes = n_lanes;
	return BMH_OK;
}

int bmh_aligner_run_fasta(bmh_aligner_t *h, const char *path, uint64_t batch_bases, uint64_t batch_reads, int paired, int n_lanes, int n_threads,
                          bmh_sam_sink_t sink, void *user, bmh_align_stats_t *stats)
{ return run_file(h, path, batch_bases, batch_reads, paired, n_lanes, n_threads, sink, user, stats, false, "bmh_aligner_run_fasta"); }

int bmh_aligner_run_file(bmh_aligner_t *h, const char *path, uint64_t batch_bases, uint64_t batch_reads, int paired, int n_lanes, int n_threads,
                         bmh_sam_sink_t sink, void *user, bmh_align_stats_t *stats)
{ return run_file(h, path, batch_bases, batch_reads, paired, n_lanes, n_threads, sink, user, stats, true, "bmh_aligner_run_file"); }
