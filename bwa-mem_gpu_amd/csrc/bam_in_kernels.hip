// BAM records cut into reads on the device (bmh_reads_load_files, bmh_aligner_run_files on a BAM file; bmh_bam_reads_device): the pump's third kind.
//
// A window of inflated BAM records starts at a record.  A record names its own length, so the record starts are one dependent chain: the host walks it over the
// window it has just inflated (bmh_bam_chain, one 4-byte read per record) and the table of 32-bit starts goes up with the window.  That is why BAM always takes
// the host inflate, also with BMH_INFLATE_DEVICE=1; a chain walk on the device is not done.  Everything else is here, per window:
//   1 per record  bi_check (csrc/bam_in_core.h): the record's own fields bounded by its extent, every tag's type and extent; kept or skipped from the flag
//                 (0x100 / 0x800: no read); a kept record's qualities looked through (none, or none above 93), its comment sized           (bin_validate)
//   2             exclusive scan of "kept" -> the kept records in order                                                                       (rocPRIM, bin_compact)
//   3 per kept    its read: kept record j is read j, or with pairs (flag 0x1 on the file's first kept record) the 0x40 record of kept records 2i, 2i+1 is read
//                 2i and the 0x80 record read 2i+1; the two names equal, one of each, 0x1 on all or none                                       (bin_place)
//   4 per read    exclusive scans of the lengths -> offs, name_offs, comment_offs                                                              (rocPRIM)
//   5 per base    one wave per read: nibble -> letter and nt4 code, quality + 33; mirrored (and the base complemented) for flag 0x10            (bin_scatter)
//   6 per read    its name, and its tags as the comment text                                                                                   (bin_names)
// A run that keeps the input's read groups gives the kernels the table of IDs (bi_groups_t, in global memory: a few hundred bytes that every lane reads row by row,
// so the rows come from the scalar and L2 caches; staging them in LDS would add a barrier to a kernel that has none): step 1 finds each kept record's RG:Z
// (bi_read_group) and its index, step 3 checks that a pair's two records agree and writes one index per read beside the lengths.  Without a table (RG = false) the
// kernels are what they were.
// A record that fails a check raises the window's flag (a plain store to a status word); so do a window whose records disagree about having qualities and, at
// the file's end, a record without its partner or bytes that are no whole record.  A flagged window is decoded by the host form (csrc/reads_io.cpp:
// bmh_bam_host_run), which delivers what comes before the damage and words the refusal with the record's index -- the fallback rule that exists for text.
// No lane reads outside its record [start, next start), which the host's walk has put inside the window, and none writes outside the spans the scans gave it.
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#define BMH_CK_PREFIX "BAM reads: "
#include "bmh_internal.h"
#include "devmem.h"
#include "bam_in_core.h"

namespace {

struct bin_ctl_t { uint32_t flag, n_qual, n_noqual, pad; };
struct bin_to64 { __host__ __device__ uint64_t operator()(uint32_t v) const { return v; } };

// per record: kept, and for a kept one its flag, lengths and where its bases start
struct bin_rec_t { uint32_t *kept, *flag, *lseq, *lname, *seqoff, *clen, *left_out, *grp; };

template <bool RG>
__global__ void __launch_bounds__(256) bin_validate(const uint8_t *__restrict__ b, const uint32_t *__restrict__ starts, uint32_t nrec, int comments, bin_rec_t M, bin_ctl_t *ctl, bi_groups_t G)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= nrec) return;
	const uint32_t s = starts[i];
	const uint8_t *r = b + s;
	bi_rec_t R;
	uint32_t kept = 0;
	bool bad = bi_check(r, starts[i + 1] - s, &R) != BI_OK;
	if (!bad && bi_role(R.flag) != 0) {
		uint32_t hq = 0;
		uint32_t g = 0;
		if (bi_check_kept(r, R, &hq) != BI_OK) bad = true;
		else if (RG && bi_read_group(r, R, G, &g) != BI_OK) bad = true;
		else {
			kept = 1;
			if (RG) M.grp[i] = g;
			uint32_t lo = 0;
			const uint32_t cl = bi_comment(r, R, nullptr, 0, &lo);
			M.flag[i] = R.flag; M.lseq[i] = R.l_seq; M.lname[i] = R.l_name; M.seqoff[i] = R.seq_off; M.clen[i] = comments ? cl + 1 : 0u; M.left_out[i] = lo;
			atomicAdd(hq ? &ctl->n_qual : &ctl->n_noqual, 1u);
		}
	}
	M.kept[i] = kept;
	if (bad) ctl->flag = 1;
}

// kidx: exclusive scan of kept
__global__ void __launch_bounds__(256) bin_compact(uint32_t nrec, const uint32_t *__restrict__ kept, const uint32_t *__restrict__ kidx, uint32_t *__restrict__ krec)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < nrec && kept[i]) krec[kidx[i]] = i;
}

// kept record j < nuse -> its read (nuse is even with pairs): lengths, the record it comes from, where the records taken with it end
template <bool RG>
__global__ void __launch_bounds__(256) bin_place(const uint8_t *__restrict__ b, const uint32_t *__restrict__ starts, uint32_t nuse, int paired, bin_rec_t M, const uint32_t *__restrict__ krec,
                                                 uint32_t *__restrict__ lens, uint32_t *__restrict__ nlen, uint32_t *__restrict__ clen, uint32_t *__restrict__ rrec, uint32_t *__restrict__ left_out,
                                                 uint32_t *__restrict__ rend, bin_ctl_t *ctl, uint32_t *__restrict__ rgrp)
{
	const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= nuse) return;
	const uint32_t i = krec[j], flag = M.flag[i], role = bi_role(flag);
	bool bad = (int)(flag & 1u) != paired;
	uint32_t r = j;
	if (paired) {
		if (role == 3) bad = true;
		r = (j & ~1u) + (role == 2 ? 1u : 0u);
		if (!(j & 1u)) {                                       // the pair's first record looks at its partner
			const uint32_t i2 = krec[j + 1], ln = M.lname[i];
			if (bi_role(M.flag[i2]) + role != 3 || M.lname[i2] != ln) bad = true;
			else if (RG && M.grp[i2] != M.grp[i]) bad = true;       // a pair of two read groups
			else {
				const uint8_t *n1 = b + starts[i] + BI_NAME_OFF, *n2 = b + starts[i2] + BI_NAME_OFF;
				for (uint32_t k = 0; k < ln; ++k) if (n1[k] != n2[k]) { bad = true; break; }
			}
		}
	}
	rend[j] = starts[i + 1];
	if (bad) { ctl->flag = 1; return; }                        // (two records of one role would write one read twice: the window is the host's anyway)
	lens[r] = M.lseq[i]; nlen[r] = M.lname[i]; clen[r] = M.clen[i]; rrec[r] = i; left_out[r] = M.left_out[i];
	if (RG) rgrp[r] = M.grp[i];
}

// one wave per read
__global__ void __launch_bounds__(256) bin_scatter(const uint8_t *__restrict__ b, const uint32_t *__restrict__ starts, uint32_t k, bin_rec_t M, const uint32_t *__restrict__ rrec,
                                                   const uint64_t *__restrict__ offs, uint8_t *__restrict__ ascii, uint8_t *__restrict__ codes, uint8_t *__restrict__ quals)
{
	const uint32_t r = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64, lane = threadIdx.x & 63u;
	if (r >= k) return;
	const uint32_t i = rrec[r];
	const uint8_t *rec = b + starts[i];
	bi_rec_t R;
	R.flag = M.flag[i]; R.l_seq = M.lseq[i]; R.seq_off = M.seqoff[i]; R.qual_off = R.seq_off + (R.l_seq + 1) / 2;
	const uint64_t d = offs[r];
	for (uint32_t t = lane; t < R.l_seq; t += 64) {
		const uint8_t c = bi_base(rec, R, t);
		ascii[d + t] = c; codes[d + t] = bi_nt4(c);
		if (quals) quals[d + t] = bi_qual(rec, R, t);
	}
}

__global__ void __launch_bounds__(256) bin_names(const uint8_t *__restrict__ b, const uint32_t *__restrict__ starts, uint32_t k, int comments, bin_rec_t M, const uint32_t *__restrict__ rrec,
                                                 const uint32_t *__restrict__ clen, const uint64_t *__restrict__ noffs, const uint64_t *__restrict__ coffs, uint8_t *__restrict__ names, uint8_t *__restrict__ cm)
{
	const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
	if (r >= k) return;
	const uint32_t i = rrec[r], s = starts[i];
	const uint8_t *rec = b + s;
	const uint32_t ln = M.lname[i];
	uint8_t *d = names + noffs[r];
	for (uint32_t t = 0; t < ln; ++t) d[t] = rec[BI_NAME_OFF + t];
	if (comments) {
		bi_rec_t R;
		R.flag = M.flag[i]; R.l_seq = M.lseq[i]; R.l_name = ln; R.seq_off = M.seqoff[i]; R.qual_off = R.seq_off + (R.l_seq + 1) / 2; R.tag_off = R.qual_off + R.l_seq; R.size = starts[i + 1] - s;
		const uint32_t cl = clen[r] - 1;
		uint32_t lo;
		uint8_t *c = cm + coffs[r];
		(void)bi_comment(rec, R, c, cl, &lo);
		c[cl] = 0;
	}
}

}   // namespace

struct bmh_bam_dev_t {
	hipStream_t st = nullptr;
	dev_buf<uint8_t> b, starts, kept, kidx, krec, flag, lseq, lname, seqoff, rclen, rleft, ctl, tmp;
	dev_buf<uint8_t> lens, nlen, clen, rrec, left, rend, offs, noffs, coffs, ascii, codes, quals, names, cm;
	pin_buf<uint8_t> h_starts, h_small, h_lens, h_left, h_rend, h_offs, h_noffs, h_coffs;
	dev_buf<uint8_t> grp, rgrp, g_ids, g_off; bool g_up = false;      // a run that keeps read groups: per record, per read, the table (sent once)
	std::vector<uint32_t> walked;
	~bmh_bam_dev_t() { if (st) (void)hipStreamDestroy(st); }

	int run(const bmh_bam_state_t &S, const bmh_bam_win_t &w, const bmh_batch_alloc_t &alloc, bmh_read_set_t *rs, bmh_bam_res_t &R)
	{
		if (!st) HIPCK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
		R = bmh_bam_res_t(); R.qual = S.qual;
		if (!w.chain) bmh_bam_chain(w.buf, w.have, walked);
		const std::vector<uint32_t> &chain = w.chain ? *w.chain : walked;
		const uint32_t nrec = (uint32_t)(chain.size() - 1);
		const size_t chain_end = chain.back();
		if (w.eof && chain_end < w.have) return 2;              // bytes that are no whole record end the file: the host delivers what is before them, then names them
		if (nrec == 0) { R.final_ = w.eof; return 1; }
		const size_t n4 = (size_t)nrec * 4;
		if (h_starts.need(n4 + 4) != BMH_OK || h_small.need(64 * sizeof(uint32_t)) != BMH_OK) return BMH_ENOMEM;
		memcpy(h_starts.p, chain.data(), n4 + 4);
		if (b.need(chain_end + 16) != BMH_OK || starts.need(n4 + 4) != BMH_OK || kept.need(n4 + 4) != BMH_OK || kidx.need(n4 + 4) != BMH_OK || krec.need(n4 + 4) != BMH_OK || flag.need(n4) != BMH_OK ||
		    lseq.need(n4) != BMH_OK || lname.need(n4) != BMH_OK || seqoff.need(n4) != BMH_OK || rclen.need(n4) != BMH_OK || rleft.need(n4) != BMH_OK ||
		    ctl.need(sizeof(bin_ctl_t)) != BMH_OK) return BMH_ENOMEM;
		uint32_t *hs = h_small.as<uint32_t>();
		const uint8_t *db = b.as<uint8_t>();
		const uint32_t *ds = starts.as<uint32_t>();
		bin_ctl_t *dctl = ctl.as<bin_ctl_t>();
		const bool rg = S.keep_rg();
		if (rg && grp.need(n4) != BMH_OK) return BMH_ENOMEM;
		if (rg && !g_up) {
			const size_t ob = 4 * S.rg_off.size();
			if (g_ids.need(S.rg_ids.size() + 16) != BMH_OK || g_off.need(ob) != BMH_OK) return BMH_ENOMEM;
			HIPCK(hipMemcpyAsync(g_ids.p, S.rg_ids.data(), S.rg_ids.size(), hipMemcpyHostToDevice, st));
			HIPCK(hipMemcpyAsync(g_off.p, S.rg_off.data(), ob, hipMemcpyHostToDevice, st));
			HIPCK(hipStreamSynchronize(st));                       // (the state's arrays are pageable: the copy has left them before anything else happens)
			g_up = true;
		}
		const bi_groups_t G = {rg ? g_ids.as<uint8_t>() : nullptr, rg ? g_off.as<uint32_t>() : nullptr, rg ? (uint32_t)S.rg_off.size() - 1 : 0u};
		const bin_rec_t M = {kept.as<uint32_t>(), flag.as<uint32_t>(), lseq.as<uint32_t>(), lname.as<uint32_t>(), seqoff.as<uint32_t>(), rclen.as<uint32_t>(), rleft.as<uint32_t>(), rg ? grp.as<uint32_t>() : nullptr};
		HIPCK(hipMemcpyAsync(b.p, w.buf, chain_end, hipMemcpyHostToDevice, st));
		HIPCK(hipMemcpyAsync(starts.p, h_starts.p, n4 + 4, hipMemcpyHostToDevice, st));
		HIPCK(hipMemsetAsync(ctl.p, 0, sizeof(bin_ctl_t), st));
		HIPCK(hipMemsetAsync(kept.p + n4, 0, 4, st));            // (one entry behind the records: the scan's last entry is then the number kept)
		const unsigned gr = (nrec + 255) / 256;
		if (rg) hipLaunchKernelGGL(bin_validate<true>, dim3(gr), dim3(256), 0, st, db, ds, nrec, w.comments ? 1 : 0, M, dctl, G);
		else hipLaunchKernelGGL(bin_validate<false>, dim3(gr), dim3(256), 0, st, db, ds, nrec, w.comments ? 1 : 0, M, dctl, G);
		{
			size_t tb = 0;
			HIPCK(rocprim::exclusive_scan(nullptr, tb, kept.as<uint32_t>(), kidx.as<uint32_t>(), 0u, (size_t)nrec + 1, rocprim::plus<uint32_t>(), st));
			if (tb > tmp.cap) { HIPCK(hipStreamSynchronize(st)); if (tmp.need(tb) != BMH_OK) return BMH_ENOMEM; }
			HIPCK(rocprim::exclusive_scan(tmp.p, tb, kept.as<uint32_t>(), kidx.as<uint32_t>(), 0u, (size_t)nrec + 1, rocprim::plus<uint32_t>(), st));
		}
		hipLaunchKernelGGL(bin_compact, dim3(gr), dim3(256), 0, st, nrec, kept.as<uint32_t>(), kidx.as<uint32_t>(), krec.as<uint32_t>());
		HIPCK(hipMemcpyAsync(hs, kidx.as<uint32_t>() + nrec, 4, hipMemcpyDeviceToHost, st));
		HIPCK(hipMemcpyAsync(hs + 4, ctl.p, sizeof(bin_ctl_t), hipMemcpyDeviceToHost, st));
		HIPCK(hipStreamSynchronize(st));
		const bin_ctl_t c1 = *(const bin_ctl_t *)(hs + 4);
		if (c1.flag) return 2;
		if (c1.n_qual && c1.n_noqual) return 2;                 // records with and without qualities: the host names the first that differs
		const int qual = c1.n_qual ? 1 : c1.n_noqual ? 2 : S.qual;
		if (S.qual && qual != S.qual) return 2;
		const uint32_t nkept = hs[0];
		if (S.paired && (nkept & 1u) && w.eof) return 2;        // a record without its partner ends the file
		const uint32_t nuse = S.paired ? nkept & ~1u : nkept;
		R.final_ = w.eof;
		if (nuse == 0) {
			if (w.eof) { R.consumed = chain_end; R.n_recs = nrec; R.skipped = nrec; }
			return 1;
		}
		const size_t t4 = (size_t)nuse * 4, t8 = ((size_t)nuse + 1) * 8;
		if (lens.need(t4 + 4) != BMH_OK || nlen.need(t4 + 4) != BMH_OK || clen.need(t4 + 4) != BMH_OK || rrec.need(t4) != BMH_OK || left.need(t4) != BMH_OK || rend.need(t4) != BMH_OK ||
		    offs.need(t8) != BMH_OK || noffs.need(t8) != BMH_OK || coffs.need(t8) != BMH_OK) return BMH_ENOMEM;
		if (h_lens.need(t4) != BMH_OK || h_left.need(t4) != BMH_OK || h_rend.need(t4) != BMH_OK || h_offs.need(t8) != BMH_OK || h_noffs.need(t8) != BMH_OK || h_coffs.need(t8) != BMH_OK) return BMH_ENOMEM;
		// (every read's entry is set before the scans read it, also in a window that bin_place flags: its sizes are not used then, but they are defined)
		HIPCK(hipMemsetAsync(lens.p, 0, t4 + 4, st)); HIPCK(hipMemsetAsync(nlen.p, 0, t4 + 4, st)); HIPCK(hipMemsetAsync(clen.p, 0, t4 + 4, st));
		if (rg && rgrp.need(t4) != BMH_OK) return BMH_ENOMEM;
		if (rg) hipLaunchKernelGGL(bin_place<true>, dim3((nuse + 255) / 256), dim3(256), 0, st, db, ds, nuse, S.paired, M, krec.as<uint32_t>(), lens.as<uint32_t>(), nlen.as<uint32_t>(), clen.as<uint32_t>(),
		                           rrec.as<uint32_t>(), left.as<uint32_t>(), rend.as<uint32_t>(), dctl, rgrp.as<uint32_t>());
		else hipLaunchKernelGGL(bin_place<false>, dim3((nuse + 255) / 256), dim3(256), 0, st, db, ds, nuse, S.paired, M, krec.as<uint32_t>(), lens.as<uint32_t>(), nlen.as<uint32_t>(), clen.as<uint32_t>(),
		                        rrec.as<uint32_t>(), left.as<uint32_t>(), rend.as<uint32_t>(), dctl, (uint32_t *)nullptr);
		{
			size_t tb = 0;
			auto in = rocprim::make_transform_iterator(lens.as<uint32_t>(), bin_to64());
			HIPCK(rocprim::exclusive_scan(nullptr, tb, in, offs.as<uint64_t>(), (uint64_t)0, (size_t)nuse + 1, rocprim::plus<uint64_t>(), st));
			if (tb > tmp.cap) { HIPCK(hipStreamSynchronize(st)); if (tmp.need(tb) != BMH_OK) return BMH_ENOMEM; }
			HIPCK(rocprim::exclusive_scan(tmp.p, tb, in, offs.as<uint64_t>(), (uint64_t)0, (size_t)nuse + 1, rocprim::plus<uint64_t>(), st));
			auto in2 = rocprim::make_transform_iterator(nlen.as<uint32_t>(), bin_to64());
			HIPCK(rocprim::exclusive_scan(tmp.p, tb, in2, noffs.as<uint64_t>(), (uint64_t)0, (size_t)nuse + 1, rocprim::plus<uint64_t>(), st));
			auto in3 = rocprim::make_transform_iterator(clen.as<uint32_t>(), bin_to64());
			HIPCK(rocprim::exclusive_scan(tmp.p, tb, in3, coffs.as<uint64_t>(), (uint64_t)0, (size_t)nuse + 1, rocprim::plus<uint64_t>(), st));
		}
		HIPCK(hipMemcpyAsync(h_lens.p, lens.p, t4, hipMemcpyDeviceToHost, st));
		HIPCK(hipMemcpyAsync(h_left.p, left.p, t4, hipMemcpyDeviceToHost, st));
		HIPCK(hipMemcpyAsync(h_rend.p, rend.p, t4, hipMemcpyDeviceToHost, st));
		HIPCK(hipMemcpyAsync(h_offs.p, offs.p, t8, hipMemcpyDeviceToHost, st));
		HIPCK(hipMemcpyAsync(h_noffs.p, noffs.p, t8, hipMemcpyDeviceToHost, st));
		HIPCK(hipMemcpyAsync(h_coffs.p, coffs.p, t8, hipMemcpyDeviceToHost, st));
		HIPCK(hipMemcpyAsync(hs + 4, ctl.p, sizeof(bin_ctl_t), hipMemcpyDeviceToHost, st));
		HIPCK(hipStreamSynchronize(st));
		if (((const bin_ctl_t *)(hs + 4))->flag) return 2;
		const uint32_t *hl = h_lens.as<uint32_t>(), *hle = h_left.as<uint32_t>(), *hre = h_rend.as<uint32_t>();
		const uint64_t *ho = h_offs.as<uint64_t>(), *hn = h_noffs.as<uint64_t>(), *hc = h_coffs.as<uint64_t>();
		bool complete = false;
		const uint64_t k = w.take_all ? nuse : bmh_cut_batch(hl, nuse, S.paired ? 2 : 1, w.want_bases, w.want_reads, w.even, &complete);
		R.complete = complete; R.final_ = w.eof && !complete;
		if (!(complete || w.take_all || R.final_)) return 1;      // the window is too short for the batch: the pump reads on
		const uint64_t nb = ho[k], nn = hn[k], nc = w.comments ? hc[k] : 0;
		const bool fq = qual == 1;
		if (ascii.need(nb + 16) != BMH_OK || codes.need(nb + 16) != BMH_OK || names.need(nn + 16) != BMH_OK || (fq && quals.need(nb + 16) != BMH_OK) || (w.comments && cm.need(nc + 16) != BMH_OK)) return BMH_ENOMEM;
		memset(rs, 0, sizeof(*rs));
		const int arc = alloc(k, nb, nn, nc, fq, rs);
		if (arc != BMH_OK) return arc;
		hipLaunchKernelGGL(bin_scatter, dim3((unsigned)((k + 3) / 4)), dim3(256), 0, st, db, ds, (uint32_t)k, M, rrec.as<uint32_t>(), offs.as<uint64_t>(), ascii.as<uint8_t>(), codes.as<uint8_t>(),
		                   fq ? quals.as<uint8_t>() : (uint8_t *)nullptr);
		hipLaunchKernelGGL(bin_names, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, st, db, ds, (uint32_t)k, w.comments ? 1 : 0, M, rrec.as<uint32_t>(), clen.as<uint32_t>(), noffs.as<uint64_t>(),
		                   coffs.as<uint64_t>(), names.as<uint8_t>(), cm.as<uint8_t>());
		HIPCK(hipMemcpyAsync(rs->ascii, ascii.p, nb, hipMemcpyDeviceToHost, st));
		if (rs->codes) HIPCK(hipMemcpyAsync(rs->codes, codes.p, nb, hipMemcpyDeviceToHost, st));
		if (fq && rs->quals) HIPCK(hipMemcpyAsync(rs->quals, quals.p, nb, hipMemcpyDeviceToHost, st));
		HIPCK(hipMemcpyAsync(rs->names, names.p, nn, hipMemcpyDeviceToHost, st));
		if (w.comments && rs->comments) HIPCK(hipMemcpyAsync(rs->comments, cm.p, nc, hipMemcpyDeviceToHost, st));
		if (rg && rs->groups) HIPCK(hipMemcpyAsync(rs->groups, rgrp.p, k * 4, hipMemcpyDeviceToHost, st));
		HIPCK(hipMemcpyAsync(hs + 1, krec.as<uint32_t>() + (k - 1), 4, hipMemcpyDeviceToHost, st));     // the last kept record taken: the records before its end
		memcpy(rs->offs, ho, k * 8); memcpy(rs->lens, hl, k * 4); memcpy(rs->name_offs, hn, k * 8);
		if (w.comments && rs->comment_offs) memcpy(rs->comment_offs, hc, k * 8);
		HIPCK(hipStreamSynchronize(st));
		rs->n_reads = k; rs->n_bases = nb; rs->n_name_bytes = nn; rs->n_comment_bytes = nc;
		R.n_reads = k; R.qual = qual;
		for (uint64_t r = 0; r < k; ++r) R.tags_left_out += hle[r];
		if (R.final_ && k == nkept) { R.consumed = chain_end; R.n_recs = nrec; }       // (the skipped records behind the last read go with it)
		else { R.consumed = hre[k - 1]; R.n_recs = (uint64_t)hs[1] + 1; }
		R.skipped = R.n_recs - k;
		return 1;
	}
};

bmh_bam_dev_t *bmh_bam_dev_create() { return new bmh_bam_dev_t(); }
void bmh_bam_dev_free(bmh_bam_dev_t *d) { delete d; }
int bmh_bam_dev_run(bmh_bam_dev_t *d, const bmh_bam_state_t &st, const bmh_bam_win_t &w, const bmh_batch_alloc_t &alloc, bmh_read_set_t *rs, bmh_bam_res_t &R) { return d->run(st, w, alloc, rs, R); }

// ---- the step on its own: uncompressed BAM records in host memory (no header) -> a read set
extern "C" int bmh_bam_reads_device(const uint8_t *records, uint64_t n_bytes, int flags, bmh_read_set_t *out)
{
	if ((!records && n_bytes) || !out) { bmh_set_error("bmh_bam_reads_device: null argument"); return BMH_EINVAL; }
	int nd = 0;
	if (hipGetDeviceCount(&nd) != hipSuccess || nd == 0) { (void)hipGetLastError(); bmh_set_error("bmh_bam_reads_device: no HIP device (bmh_bam_reads_host decodes on the host)"); return BMH_ENODEV; }
	bmh_bam_dev_t d;
	return bmh_bam_reads_run("bmh_bam_reads_device", &d, records, n_bytes, flags, out);
}

// ... with a table of read group IDs: out->groups [n_reads] is every read's index in it (csrc/bam_in_core.h: bi_read_group)
extern "C" int bmh_bam_reads_groups_device(const uint8_t *records, uint64_t n_bytes, int flags, const char *const *rg_ids, int n_groups, bmh_read_set_t *out)
{
	if ((!records && n_bytes) || !out || !rg_ids) { bmh_set_error("bmh_bam_reads_groups_device: null argument"); return BMH_EINVAL; }
	int nd = 0;
	if (hipGetDeviceCount(&nd) != hipSuccess || nd == 0) { (void)hipGetLastError(); bmh_set_error("bmh_bam_reads_groups_device: no HIP device (bmh_bam_reads_groups_host decodes on the host)"); return BMH_ENODEV; }
	bmh_bam_dev_t d;
	return bmh_bam_reads_run("bmh_bam_reads_groups_device", &d, records, n_bytes, flags, out, rg_ids, n_groups);
}
