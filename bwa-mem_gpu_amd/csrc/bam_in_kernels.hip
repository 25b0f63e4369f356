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
//
// Mates collated by name (--collate; csrc/bam_collate_core.h has the definition and the pool): step 3 is replaced, per window, by
//   3a per kept    the key: 64-bit FNV-1a of the name, the kept record's index as the value; the pool's resident keys (hash; role and slot) in front        (bcl_keys)
//   3b             stable radix sort of the keys by hash                                                                                                 (rocPRIM)
//   3c per entry   the first entry of a run of equal hashes decides the run: one entry is an open record; one 0x40 and one 0x80 record are a pair once their names
//                  are compared (two window records here, a pool record and a window record on the host, which holds both); anything else raises the status
//                  word's second flag and the window is the host form's                                                                                  (bcl_match)
//   3d             exclusive scans of "completes a pair" and "pool record matched": a pair's rank in the order of completion, the matched pool records in order
//   3e             the host copies the matched pool records behind the window's bytes and extends `starts`; bin_validate fills their fields like any record's
//   3f per kept    a completion writes its pair's two reads (the 0x40 record read 2r, the 0x80 record 2r + 1) and where the pair ends                     (bcl_place)
// and, once the batch is cut, the open records of the consumed prefix are compacted into an index list (bcl_finish, bcl_olist: the host copies their bytes into
// the pool and names their slots) and the resident keys are rewritten without the closed ones and with the new ones behind (bcl_pool_update).  A window's work
// grows with the pool's keys (they are sorted again), never with its bytes: a pool record goes up again only when it is matched.
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
#include "bam_collate_core.h"

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

// ---- mates collated by name
enum : uint32_t { BCL_NONE = 0xffffffffu, BCL_POOL = 0x80000000u };

// entries [0, np): the pool's resident keys; [np, np + nkept): the window's kept records (a record's role and the 0x1 mix are checked here: bin_place does not run)
__global__ void __launch_bounds__(256) bcl_keys(const uint8_t *__restrict__ b, const uint32_t *__restrict__ starts, uint32_t np, uint32_t nkept, const uint32_t *__restrict__ krec, bin_rec_t M, int bits,
                                                const uint64_t *__restrict__ pk_hash, uint64_t *__restrict__ hash, uint32_t *__restrict__ val, bin_ctl_t *ctl)
{
	const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
	if (e >= np + nkept) return;
	if (e < np) { hash[e] = pk_hash[e]; val[e] = BCL_POOL | e; return; }
	const uint32_t j = e - np, i = krec[j], flag = M.flag[i];
	if (!(flag & 1u) || bi_role(flag) == 3) ctl->flag = 1;
	hash[e] = bcl_hash(b + starts[i] + BI_NAME_OFF, M.lname[i] - 1, bits);
	val[e] = j;
}

// hs / vs: the sorted keys.  part[j]: the kept record's partner (a kept index, or BCL_POOL | the pool key's position); cmpl[j]: the kept index its pair completes at
__global__ void __launch_bounds__(256) bcl_match(const uint8_t *__restrict__ b, const uint32_t *__restrict__ starts, uint32_t n, const uint64_t *__restrict__ hs, const uint32_t *__restrict__ vs,
                                                 const uint32_t *__restrict__ krec, bin_rec_t M, const uint32_t *__restrict__ pk_info, uint32_t *__restrict__ part, uint32_t *__restrict__ cmpl,
                                                 uint32_t *__restrict__ cflag, uint32_t *__restrict__ pmatch, uint32_t *__restrict__ pflag, bin_ctl_t *ctl)
{
	const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
	if (e >= n) return;
	const uint64_t h = hs[e];
	if (e > 0 && hs[e - 1] == h) return;                     // (the run's first entry decides)
	if (e + 1 >= n || hs[e + 1] != h) return;               // a run of one: an open record
	if (e + 2 < n && hs[e + 2] == h) {                      // three or more: the host's, unless they are all open records of the pool
		for (uint32_t t = e; t < n && hs[t] == h; ++t) if (!(vs[t] & BCL_POOL)) { ctl->pad = 1; break; }
		return;
	}
	uint32_t v0 = vs[e], v1 = vs[e + 1];
	if ((v0 & BCL_POOL) && (v1 & BCL_POOL)) return;         // two open records of the pool share a hash: nothing happens to them here
	if (v1 & BCL_POOL) { const uint32_t t = v0; v0 = v1; v1 = t; }
	const uint32_t j1 = v1, i1 = krec[j1], role1 = bi_role(M.flag[i1]);
	if (v0 & BCL_POOL) {
		const uint32_t p = v0 & ~BCL_POOL;
		if ((pk_info[p] >> 31) + 1 == role1) { ctl->pad = 1; return; }
		part[j1] = v0; cmpl[j1] = j1; cflag[j1] = 1; pmatch[p] = j1; pflag[p] = 1;          // (the host compares the two names)
		return;
	}
	if (v0 > v1) { const uint32_t t = v0; v0 = v1; v1 = t; }
	const uint32_t lo = v0, hi = v1, ilo = krec[lo], ihi = krec[hi], ln = M.lname[ilo];
	bool same = bi_role(M.flag[ilo]) + bi_role(M.flag[ihi]) == 3 && M.lname[ihi] == ln;
	if (same) {
		const uint8_t *n1 = b + starts[ilo] + BI_NAME_OFF, *n2 = b + starts[ihi] + BI_NAME_OFF;
		for (uint32_t k = 0; k < ln; ++k) if (n1[k] != n2[k]) { same = false; break; }
	}
	if (!same) { ctl->pad = 1; return; }
	part[lo] = hi; part[hi] = lo; cmpl[lo] = hi; cmpl[hi] = hi; cflag[hi] = 1;
}

// the matched pool keys in order: their slots, the kept records that close them and those records' indices in the window
__global__ void __launch_bounds__(256) bcl_plist(uint32_t np, const uint32_t *__restrict__ pmatch, const uint32_t *__restrict__ pq, const uint32_t *__restrict__ pk_info, const uint32_t *__restrict__ krec,
                                                 uint32_t *__restrict__ lslot, uint32_t *__restrict__ lj, uint32_t *__restrict__ li)
{
	const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
	if (p >= np || pmatch[p] == BCL_NONE) return;
	const uint32_t q = pq[p];
	lslot[q] = pk_info[p] & ~BCL_POOL; lj[q] = pmatch[p]; li[q] = krec[pmatch[p]];
}

// kept record j: a completion (rank r among them) writes its pair's reads 2r, 2r + 1; dsz[j]: what the record does to the open bytes (+ its own size when it
// opens, - its partner's when it closes).  A matched pool record is record nrec + pq[its key] of the extended window
template <bool RG>
__global__ void __launch_bounds__(256) bcl_place(const uint32_t *__restrict__ starts, uint32_t nrec, uint32_t nkept, bin_rec_t M, const uint32_t *__restrict__ krec, const uint32_t *__restrict__ part,
                                                 const uint32_t *__restrict__ cmpl, const uint32_t *__restrict__ rank, const uint32_t *__restrict__ pq,
                                                 uint32_t *__restrict__ lens, uint32_t *__restrict__ nlen, uint32_t *__restrict__ clen, uint32_t *__restrict__ rrec, uint32_t *__restrict__ left_out, uint32_t *__restrict__ rgrp,
                                                 uint32_t *__restrict__ p_rec, uint32_t *__restrict__ p_j, uint32_t *__restrict__ p_end, uint32_t *__restrict__ p_adj, int32_t *__restrict__ dsz, bin_ctl_t *ctl)
{
	const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= nkept) return;
	const uint32_t i = krec[j];
	if (cmpl[j] != j) { dsz[j] = (int32_t)(starts[i + 1] - starts[i]); return; }
	const uint32_t pv = part[j], ip = (pv & BCL_POOL) ? nrec + pq[pv & ~BCL_POOL] : krec[pv], r = rank[j];
	dsz[j] = -(int32_t)(starts[ip + 1] - starts[ip]);
	p_rec[r] = i; p_j[r] = j; p_end[r] = starts[i + 1]; p_adj[r] = (!(pv & BCL_POOL) && pv + 1 == j) ? 1u : 0u;
	if (RG && M.grp[ip] != M.grp[i]) { ctl->flag = 1; return; }        // a pair of two read groups
	const uint32_t second = bi_role(M.flag[i]) == 2 ? 1u : 0u;
	const uint32_t rr[2] = {2 * r + second, 2 * r + 1 - second}, ii[2] = {i, ip};
	for (int t = 0; t < 2; ++t) {
		lens[rr[t]] = M.lseq[ii[t]]; nlen[rr[t]] = M.lname[ii[t]]; clen[rr[t]] = M.clen[ii[t]]; rrec[rr[t]] = ii[t]; left_out[rr[t]] = M.left_out[ii[t]];
		if (RG) rgrp[rr[t]] = M.grp[ii[t]];
	}
}

// the batch is cut behind kept record jcut: a kept record up to it is open when its pair completes behind it (or never); a pool key closed up to it leaves
__global__ void __launch_bounds__(256) bcl_finish(uint32_t jcut, const uint32_t *__restrict__ part, const uint32_t *__restrict__ cmpl, uint32_t *__restrict__ oflag, uint32_t *__restrict__ pclosed)
{
	const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j > jcut) return;
	const uint32_t c = cmpl[j];
	oflag[j] = c > jcut ? 1u : 0u;                            // (BCL_NONE is behind every record)
	if (c == j && (part[j] & BCL_POOL)) pclosed[part[j] & ~BCL_POOL] = 1;
}

__global__ void __launch_bounds__(256) bcl_olist(uint32_t jcut, const uint32_t *__restrict__ oflag, const uint32_t *__restrict__ opos, const uint32_t *__restrict__ krec, uint32_t *__restrict__ olist_i, uint32_t *__restrict__ olist_j)
{
	const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j > jcut || !oflag[j]) return;
	olist_i[opos[j]] = krec[j]; olist_j[opos[j]] = j;
}

// the resident keys rewritten: the np old ones without the closed (cpos: exclusive scan of pclosed), then the `no` new open records with the slots the host gave them
__global__ void __launch_bounds__(256) bcl_pool_update(uint32_t np, uint32_t no, uint32_t nkeep, const uint32_t *__restrict__ pclosed, const uint32_t *__restrict__ cpos, const uint64_t *__restrict__ pk_hash,
                                                       const uint32_t *__restrict__ pk_info, const uint64_t *__restrict__ whash, const uint32_t *__restrict__ olist_i, const uint32_t *__restrict__ olist_j,
                                                       const uint32_t *__restrict__ oslots, bin_rec_t M, uint64_t *__restrict__ pk_hash2, uint32_t *__restrict__ pk_info2)
{
	const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
	if (e < np) {
		if (!pclosed[e]) { const uint32_t d = e - cpos[e]; pk_hash2[d] = pk_hash[e]; pk_info2[d] = pk_info[e]; }
		return;
	}
	const uint32_t t = e - np;
	if (t >= no) return;
	pk_hash2[nkeep + t] = whash[olist_j[t]];
	pk_info2[nkeep + t] = ((bi_role(M.flag[olist_i[t]]) - 1u) << 31) | oslots[t];
}

}   // namespace

struct bmh_bam_dev_t {
	hipStream_t st = nullptr;
	dev_buf<uint8_t> b, starts, kept, kidx, krec, flag, lseq, lname, seqoff, rclen, rleft, ctl, tmp;
	dev_buf<uint8_t> lens, nlen, clen, rrec, left, rend, offs, noffs, coffs, ascii, codes, quals, names, cm;
	pin_buf<uint8_t> h_starts, h_small, h_lens, h_left, h_rend, h_offs, h_noffs, h_coffs;
	dev_buf<uint8_t> grp, rgrp, g_ids, g_off; bool g_up = false;      // a run that keeps read groups: per record, per read, the table (sent once)
	std::vector<uint32_t> walked;
	// mates collated by name: the window's keys and what the match leaves (c_*), the pool's resident keys (pk_*: hash; role << 31 | slot) and the pool version they stand for
	dev_buf<uint8_t> c_hash, c_hash2, c_val, c_val2, c_part, c_cmpl, c_cflag, c_rank, c_pmatch, c_pflag, c_pq, c_lslot, c_lj, c_li, c_prec, c_pj, c_pend, c_padj, c_dsz, c_oflag, c_opos, c_oli, c_olj,
	                 c_pclosed, c_cpos, c_oslots, pk_hash, pk_info, pk_hash2, pk_info2;
	pin_buf<uint8_t> h_keys, h_list, h_ext, h_pair, h_dsz, h_open;
	uint32_t np_dev = 0; uint64_t synced = ~(uint64_t)0; const bcl_pool_t *synced_pool = nullptr;
	~bmh_bam_dev_t() { if (st) (void)hipStreamDestroy(st); }

	int scan32(const uint32_t *in, uint32_t *out, size_t n)
	{
		size_t tb = 0;
		HIPCK(rocprim::exclusive_scan(nullptr, tb, in, out, 0u, n, rocprim::plus<uint32_t>(), st));
		if (tb > tmp.cap) { HIPCK(hipStreamSynchronize(st)); if (tmp.need(tb) != BMH_OK) return BMH_ENOMEM; }
		HIPCK(rocprim::exclusive_scan(tmp.p, tb, in, out, 0u, n, rocprim::plus<uint32_t>(), st));
		return BMH_OK;
	}

	// the window's kept records (krec [nkept], their fields in M) matched by name, against each other and against the pool's keys; everything behind bin_compact
	int collate(const bmh_bam_state_t &S, const bmh_bam_win_t &w, const bmh_batch_alloc_t &alloc, bmh_read_set_t *rs, bmh_bam_res_t &R, const std::vector<uint32_t> &chain, uint32_t nkept, int qual,
	            const bin_rec_t &M, const bi_groups_t &G, bool rg)
	{
		bcl_pool_t &P = *S.col;
		const uint32_t nrec = (uint32_t)(chain.size() - 1);
		const size_t chain_end = chain.back();
		uint32_t *hs = h_small.as<uint32_t>();
		bin_ctl_t *dctl = ctl.as<bin_ctl_t>();
		const uint32_t *ds = starts.as<uint32_t>();
		R.final_ = w.eof;
		if (nkept == 0) {
			if (w.eof) { R.consumed = chain_end; R.n_recs = nrec; R.skipped = nrec; }
			return 1;
		}
		// the resident keys follow the pool: after a window of the host form (or at the first window) they are sent whole -- keys, never records
		if (synced_pool != &P || synced != P.version) {
			const size_t nu = (size_t)P.n;
			if (h_keys.need(nu * 12 + 16) != BMH_OK || pk_hash.need(nu * 8 + 8) != BMH_OK || pk_info.need(nu * 4 + 4) != BMH_OK) return BMH_ENOMEM;
			uint64_t *kh = h_keys.as<uint64_t>(); uint32_t *ki = (uint32_t *)(kh + nu);
			size_t k = 0;
			for (size_t s = 0; s < P.slots.size(); ++s) if (P.slots[s].used) { kh[k] = P.slots[s].hash; ki[k] = ((P.role((uint32_t)s) - 1u) << 31) | (uint32_t)s; ++k; }
			if (nu) {
				HIPCK(hipMemcpyAsync(pk_hash.p, kh, nu * 8, hipMemcpyHostToDevice, st));
				HIPCK(hipMemcpyAsync(pk_info.p, ki, nu * 4, hipMemcpyHostToDevice, st));
				HIPCK(hipStreamSynchronize(st));
			}
			np_dev = (uint32_t)nu; synced = P.version; synced_pool = &P;
		}
		const uint32_t np = np_dev, n = np + nkept;
		const size_t k4 = ((size_t)nkept + 1) * 4, p4 = ((size_t)np + 1) * 4;
		if (c_hash.need((size_t)n * 8) != BMH_OK || c_hash2.need((size_t)n * 8) != BMH_OK || c_val.need((size_t)n * 4) != BMH_OK || c_val2.need((size_t)n * 4) != BMH_OK || c_part.need(k4) != BMH_OK ||
		    c_cmpl.need(k4) != BMH_OK || c_cflag.need(k4) != BMH_OK || c_rank.need(k4) != BMH_OK || c_pmatch.need(p4) != BMH_OK || c_pflag.need(p4) != BMH_OK || c_pq.need(p4) != BMH_OK ||
		    c_lslot.need(p4) != BMH_OK || c_lj.need(p4) != BMH_OK || c_li.need(p4) != BMH_OK || c_dsz.need(k4) != BMH_OK || c_oflag.need(k4 + 4) != BMH_OK || c_opos.need(k4 + 4) != BMH_OK ||
		    c_oli.need(k4) != BMH_OK || c_olj.need(k4) != BMH_OK || c_pclosed.need(p4) != BMH_OK || c_cpos.need(p4) != BMH_OK) return BMH_ENOMEM;
		HIPCK(hipMemsetAsync(c_part.p, 0xff, k4, st)); HIPCK(hipMemsetAsync(c_cmpl.p, 0xff, k4, st)); HIPCK(hipMemsetAsync(c_cflag.p, 0, k4, st));
		HIPCK(hipMemsetAsync(c_pmatch.p, 0xff, p4, st)); HIPCK(hipMemsetAsync(c_pflag.p, 0, p4, st));
		hipLaunchKernelGGL(bcl_keys, dim3((n + 255) / 256), dim3(256), 0, st, b.as<uint8_t>(), ds, np, nkept, krec.as<uint32_t>(), M, P.hash_bits, pk_hash.as<uint64_t>(), c_hash.as<uint64_t>(), c_val.as<uint32_t>(), dctl);
		{
			size_t tb = 0;
			HIPCK(rocprim::radix_sort_pairs(nullptr, tb, c_hash.as<uint64_t>(), c_hash2.as<uint64_t>(), c_val.as<uint32_t>(), c_val2.as<uint32_t>(), (size_t)n, 0, 64, st));
			if (tb > tmp.cap) { HIPCK(hipStreamSynchronize(st)); if (tmp.need(tb) != BMH_OK) return BMH_ENOMEM; }
			HIPCK(rocprim::radix_sort_pairs(tmp.p, tb, c_hash.as<uint64_t>(), c_hash2.as<uint64_t>(), c_val.as<uint32_t>(), c_val2.as<uint32_t>(), (size_t)n, 0, 64, st));
		}
		hipLaunchKernelGGL(bcl_match, dim3((n + 255) / 256), dim3(256), 0, st, b.as<uint8_t>(), ds, n, c_hash2.as<uint64_t>(), c_val2.as<uint32_t>(), krec.as<uint32_t>(), M, pk_info.as<uint32_t>(),
		                   c_part.as<uint32_t>(), c_cmpl.as<uint32_t>(), c_cflag.as<uint32_t>(), c_pmatch.as<uint32_t>(), c_pflag.as<uint32_t>(), dctl);
		RCK(scan32(c_cflag.as<uint32_t>(), c_rank.as<uint32_t>(), (size_t)nkept + 1));
		RCK(scan32(c_pflag.as<uint32_t>(), c_pq.as<uint32_t>(), (size_t)np + 1));
		if (np) hipLaunchKernelGGL(bcl_plist, dim3((np + 255) / 256), dim3(256), 0, st, np, c_pmatch.as<uint32_t>(), c_pq.as<uint32_t>(), pk_info.as<uint32_t>(), krec.as<uint32_t>(), c_lslot.as<uint32_t>(),
		                           c_lj.as<uint32_t>(), c_li.as<uint32_t>());
		HIPCK(hipMemcpyAsync(hs + 1, c_rank.as<uint32_t>() + nkept, 4, hipMemcpyDeviceToHost, st));
		HIPCK(hipMemcpyAsync(hs + 2, c_pq.as<uint32_t>() + np, 4, hipMemcpyDeviceToHost, st));
		HIPCK(hipMemcpyAsync(hs + 4, ctl.p, sizeof(bin_ctl_t), hipMemcpyDeviceToHost, st));
		HIPCK(hipStreamSynchronize(st));
		const bin_ctl_t c2 = *(const bin_ctl_t *)(hs + 4);
		if (c2.flag) return 2;
		if (c2.pad) { ++P.cnt.windows_to_host_for_hash_runs; return 2; }
		const uint32_t npairs = hs[1], nq = hs[2];
		if (npairs == 0) return w.eof ? 2 : 1;                  // no pair completes here: the pump reads on; at the file's end the host names the open record
		// the pool records this window closes: names compared here (the host holds both records), their bytes behind the window's, `starts` extended
		size_t ext = 0;
		if (nq) {
			if (h_list.need((size_t)nq * 12) != BMH_OK) return BMH_ENOMEM;
			uint32_t *ls = h_list.as<uint32_t>(), *lj = ls + nq, *li = lj + nq;
			HIPCK(hipMemcpyAsync(ls, c_lslot.p, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
			HIPCK(hipMemcpyAsync(lj, c_lj.p, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
			HIPCK(hipMemcpyAsync(li, c_li.p, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
			HIPCK(hipStreamSynchronize(st));
			for (uint32_t q = 0; q < nq; ++q) {
				if (strcmp(P.name(ls[q]), (const char *)w.buf + chain[li[q]] + BI_NAME_OFF) != 0) { ++P.cnt.windows_to_host_for_hash_runs; return 2; }      // equal hashes, two names
				ext += P.slots[ls[q]].bytes.size();
			}
			if (chain_end + ext >= ((size_t)1 << 31) - 4096) return 2;       // (the extended window keeps 32-bit offsets: the host form needs no copy)
			if (h_ext.need(ext + 16) != BMH_OK) return BMH_ENOMEM;
			uint32_t *hst = h_starts.as<uint32_t>();
			size_t o = 0;
			for (uint32_t q = 0; q < nq; ++q) {
				const std::vector<uint8_t> &pb = P.slots[ls[q]].bytes;
				memcpy(h_ext.p + o, pb.data(), pb.size()); o += pb.size();
				hst[nrec + 1 + q] = (uint32_t)(chain_end + o);
			}
			if (b.cap < chain_end + ext + 16) {                    // (rare: the window goes up again into a larger buffer)
				HIPCK(hipStreamSynchronize(st));
				if (b.need(chain_end + ext + 16) != BMH_OK) return BMH_ENOMEM;
				HIPCK(hipMemcpyAsync(b.p, w.buf, chain_end, hipMemcpyHostToDevice, st));
			}
			HIPCK(hipMemcpyAsync(b.p + chain_end, h_ext.p, ext, hipMemcpyHostToDevice, st));
			HIPCK(hipMemcpyAsync(starts.as<uint32_t>() + nrec + 1, hst + nrec + 1, (size_t)nq * 4, hipMemcpyHostToDevice, st));
			bin_rec_t M2 = M;
			M2.kept += nrec; M2.flag += nrec; M2.lseq += nrec; M2.lname += nrec; M2.seqoff += nrec; M2.clen += nrec; M2.left_out += nrec; if (rg) M2.grp += nrec;
			if (rg) hipLaunchKernelGGL(bin_validate<true>, dim3((nq + 255) / 256), dim3(256), 0, st, b.as<uint8_t>(), ds + nrec, nq, w.comments ? 1 : 0, M2, dctl, G);
			else hipLaunchKernelGGL(bin_validate<false>, dim3((nq + 255) / 256), dim3(256), 0, st, b.as<uint8_t>(), ds + nrec, nq, w.comments ? 1 : 0, M2, dctl, G);
		}
		const uint8_t *db = b.as<uint8_t>();
		const uint32_t nuse = 2 * npairs;
		const size_t t4 = (size_t)nuse * 4, t8 = ((size_t)nuse + 1) * 8, q4 = (size_t)npairs * 4;
		if (lens.need(t4 + 4) != BMH_OK || nlen.need(t4 + 4) != BMH_OK || clen.need(t4 + 4) != BMH_OK || rrec.need(t4) != BMH_OK || left.need(t4) != BMH_OK ||
		    offs.need(t8) != BMH_OK || noffs.need(t8) != BMH_OK || coffs.need(t8) != BMH_OK || c_prec.need(q4) != BMH_OK || c_pj.need(q4) != BMH_OK || c_pend.need(q4) != BMH_OK || c_padj.need(q4) != BMH_OK) return BMH_ENOMEM;
		if (h_lens.need(t4) != BMH_OK || h_left.need(t4) != BMH_OK || h_offs.need(t8) != BMH_OK || h_noffs.need(t8) != BMH_OK || h_coffs.need(t8) != BMH_OK || h_pair.need(q4 * 4) != BMH_OK ||
		    h_dsz.need((size_t)nkept * 4) != BMH_OK) return BMH_ENOMEM;
		HIPCK(hipMemsetAsync(lens.p, 0, t4 + 4, st)); HIPCK(hipMemsetAsync(nlen.p, 0, t4 + 4, st)); HIPCK(hipMemsetAsync(clen.p, 0, t4 + 4, st));
		if (rg && rgrp.need(t4) != BMH_OK) return BMH_ENOMEM;
		if (rg) hipLaunchKernelGGL(bcl_place<true>, dim3((nkept + 255) / 256), dim3(256), 0, st, ds, nrec, nkept, M, krec.as<uint32_t>(), c_part.as<uint32_t>(), c_cmpl.as<uint32_t>(), c_rank.as<uint32_t>(), c_pq.as<uint32_t>(),
		                           lens.as<uint32_t>(), nlen.as<uint32_t>(), clen.as<uint32_t>(), rrec.as<uint32_t>(), left.as<uint32_t>(), rgrp.as<uint32_t>(), c_prec.as<uint32_t>(), c_pj.as<uint32_t>(),
		                           c_pend.as<uint32_t>(), c_padj.as<uint32_t>(), c_dsz.as<int32_t>(), dctl);
		else hipLaunchKernelGGL(bcl_place<false>, dim3((nkept + 255) / 256), dim3(256), 0, st, ds, nrec, nkept, M, krec.as<uint32_t>(), c_part.as<uint32_t>(), c_cmpl.as<uint32_t>(), c_rank.as<uint32_t>(), c_pq.as<uint32_t>(),
		                        lens.as<uint32_t>(), nlen.as<uint32_t>(), clen.as<uint32_t>(), rrec.as<uint32_t>(), left.as<uint32_t>(), (uint32_t *)nullptr, c_prec.as<uint32_t>(), c_pj.as<uint32_t>(),
		                        c_pend.as<uint32_t>(), c_padj.as<uint32_t>(), c_dsz.as<int32_t>(), dctl);
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
		uint32_t *hp_rec = h_pair.as<uint32_t>(), *hp_j = hp_rec + npairs, *hp_end = hp_j + npairs, *hp_adj = hp_end + npairs;
		HIPCK(hipMemcpyAsync(h_lens.p, lens.p, t4, hipMemcpyDeviceToHost, st));
		HIPCK(hipMemcpyAsync(h_left.p, left.p, t4, hipMemcpyDeviceToHost, st));
		HIPCK(hipMemcpyAsync(h_offs.p, offs.p, t8, hipMemcpyDeviceToHost, st));
		HIPCK(hipMemcpyAsync(h_noffs.p, noffs.p, t8, hipMemcpyDeviceToHost, st));
		HIPCK(hipMemcpyAsync(h_coffs.p, coffs.p, t8, hipMemcpyDeviceToHost, st));
		HIPCK(hipMemcpyAsync(hp_rec, c_prec.p, q4, hipMemcpyDeviceToHost, st));
		HIPCK(hipMemcpyAsync(hp_j, c_pj.p, q4, hipMemcpyDeviceToHost, st));
		HIPCK(hipMemcpyAsync(hp_end, c_pend.p, q4, hipMemcpyDeviceToHost, st));
		HIPCK(hipMemcpyAsync(hp_adj, c_padj.p, q4, hipMemcpyDeviceToHost, st));
		HIPCK(hipMemcpyAsync(h_dsz.p, c_dsz.p, (size_t)nkept * 4, hipMemcpyDeviceToHost, st));
		HIPCK(hipMemcpyAsync(hs + 4, ctl.p, sizeof(bin_ctl_t), hipMemcpyDeviceToHost, st));
		HIPCK(hipStreamSynchronize(st));
		if (((const bin_ctl_t *)(hs + 4))->flag) return 2;
		const uint32_t *hl = h_lens.as<uint32_t>(), *hle = h_left.as<uint32_t>();
		const uint64_t *ho = h_offs.as<uint64_t>(), *hn = h_noffs.as<uint64_t>(), *hc = h_coffs.as<uint64_t>();
		bool complete = false;
		const uint64_t k = w.take_all ? nuse : bmh_cut_batch(hl, nuse, 2, w.want_bases, w.want_reads, w.even, &complete);
		R.complete = complete; R.final_ = w.eof && !complete;
		if (!(complete || w.take_all || R.final_)) return 1;      // the window is too short for the batch: the pump reads on
		const uint32_t npc = (uint32_t)(k / 2), jcut = hp_j[npc - 1], icut = hp_rec[npc - 1];
		// the open records and their bytes over the prefix, as the definition counts them; beyond the cap the host form names the record
		uint64_t cur_n = P.n, cur_b = P.bytes, pk_n = cur_n, pk_b = cur_b;
		{
			const int32_t *dz = h_dsz.as<int32_t>();
			for (uint32_t j = 0; j <= jcut; ++j) {
				if (dz[j] > 0) { ++cur_n; cur_b += (uint64_t)dz[j]; if (cur_n > pk_n) pk_n = cur_n; if (cur_b > pk_b) pk_b = cur_b; }
				else { --cur_n; cur_b -= (uint64_t)(-(int64_t)dz[j]); }
			}
			if (pk_b > P.cap) return 2;
		}
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
		// hand-back: the open records of the prefix as an index list, the pool keys the prefix closes
		HIPCK(hipMemsetAsync(c_oflag.p, 0, ((size_t)jcut + 2) * 4, st)); HIPCK(hipMemsetAsync(c_pclosed.p, 0, p4, st));
		hipLaunchKernelGGL(bcl_finish, dim3((jcut + 256) / 256), dim3(256), 0, st, jcut, c_part.as<uint32_t>(), c_cmpl.as<uint32_t>(), c_oflag.as<uint32_t>(), c_pclosed.as<uint32_t>());
		RCK(scan32(c_oflag.as<uint32_t>(), c_opos.as<uint32_t>(), (size_t)jcut + 2));
		RCK(scan32(c_pclosed.as<uint32_t>(), c_cpos.as<uint32_t>(), (size_t)np + 1));
		hipLaunchKernelGGL(bcl_olist, dim3((jcut + 256) / 256), dim3(256), 0, st, jcut, c_oflag.as<uint32_t>(), c_opos.as<uint32_t>(), krec.as<uint32_t>(), c_oli.as<uint32_t>(), c_olj.as<uint32_t>());
		HIPCK(hipMemcpyAsync(hs + 1, c_opos.as<uint32_t>() + jcut + 1, 4, hipMemcpyDeviceToHost, st));
		HIPCK(hipMemcpyAsync(hs + 2, c_cpos.as<uint32_t>() + np, 4, hipMemcpyDeviceToHost, st));
		memcpy(rs->offs, ho, k * 8); memcpy(rs->lens, hl, k * 4); memcpy(rs->name_offs, hn, k * 8);
		if (w.comments && rs->comment_offs) memcpy(rs->comment_offs, hc, k * 8);
		HIPCK(hipStreamSynchronize(st));
		const uint32_t no = hs[1], nclosed = hs[2];
		if (h_open.need((size_t)no * 8 + 16) != BMH_OK || c_oslots.need((size_t)no * 4 + 4) != BMH_OK) return BMH_ENOMEM;
		uint32_t *oi = h_open.as<uint32_t>(), *oslot = oi + no;
		if (no) { HIPCK(hipMemcpyAsync(oi, c_oli.p, (size_t)no * 4, hipMemcpyDeviceToHost, st)); HIPCK(hipStreamSynchronize(st)); }
		// the pool follows: closed records leave (their slots are the next ones taken), the prefix's open records enter with their file indices
		if (nq) {
			const uint32_t *ls = h_list.as<uint32_t>(), *lj = ls + nq;
			for (uint32_t q = 0; q < nq; ++q) if (lj[q] <= jcut) P.remove(ls[q]);
		}
		for (uint32_t t = 0; t < no; ++t) oslot[t] = P.add(w.buf + chain[oi[t]], chain[oi[t] + 1] - chain[oi[t]], S.n_recs + oi[t]);
		const uint32_t nkeep = np - nclosed, np_new = nkeep + no;
		if (nclosed || no) {
			if (pk_hash2.need((size_t)np_new * 8 + 8) != BMH_OK || pk_info2.need((size_t)np_new * 4 + 4) != BMH_OK) return BMH_ENOMEM;
			if (no) HIPCK(hipMemcpyAsync(c_oslots.p, oslot, (size_t)no * 4, hipMemcpyHostToDevice, st));
			hipLaunchKernelGGL(bcl_pool_update, dim3((np + no + 255) / 256), dim3(256), 0, st, np, no, nkeep, c_pclosed.as<uint32_t>(), c_cpos.as<uint32_t>(), pk_hash.as<uint64_t>(), pk_info.as<uint32_t>(),
			                   c_hash.as<uint64_t>() + np, c_oli.as<uint32_t>(), c_olj.as<uint32_t>(), c_oslots.as<uint32_t>(), M, pk_hash2.as<uint64_t>(), pk_info2.as<uint32_t>());
			HIPCK(hipStreamSynchronize(st));
			pk_hash.swap(pk_hash2); pk_info.swap(pk_info2);
		}
		np_dev = np_new; synced = P.version;
		uint64_t adj = 0;
		for (uint32_t r = 0; r < npc; ++r) adj += hp_adj[r];
		P.cnt.pairs += npc; P.cnt.pairs_adjacent += adj;
		P.cnt.open_records_peak = std::max(P.cnt.open_records_peak, pk_n); P.cnt.open_bytes_peak = std::max(P.cnt.open_bytes_peak, pk_b);
		rs->n_reads = k; rs->n_bases = nb; rs->n_name_bytes = nn; rs->n_comment_bytes = nc;
		R.n_reads = k; R.qual = qual;
		for (uint64_t r = 0; r < k; ++r) R.tags_left_out += hle[r];
		if (R.final_ && k == nuse && jcut == nkept - 1 && no == 0) { R.consumed = chain_end; R.n_recs = nrec; R.skipped = nrec - nkept; }      // (the skipped records behind the last pair go with it)
		else { R.consumed = hp_end[npc - 1]; R.n_recs = (uint64_t)icut + 1; R.skipped = R.n_recs - ((uint64_t)jcut + 1); }
		return 1;
	}

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
		// (a run that collates: up to min(pool, records) matched pool records are appended to the window as records of their own)
		const size_t n4 = (size_t)nrec * 4, x4 = S.collate() ? 4 * (size_t)std::min<uint64_t>(S.col->n, nrec) : 0;
		if (h_starts.need(n4 + x4 + 4) != BMH_OK || h_small.need(64 * sizeof(uint32_t)) != BMH_OK) return BMH_ENOMEM;
		memcpy(h_starts.p, chain.data(), n4 + 4);
		if (b.need(chain_end + 16) != BMH_OK || starts.need(n4 + x4 + 4) != BMH_OK || kept.need(n4 + x4 + 4) != BMH_OK || kidx.need(n4 + 4) != BMH_OK || krec.need(n4 + 4) != BMH_OK || flag.need(n4 + x4) != BMH_OK ||
		    lseq.need(n4 + x4) != BMH_OK || lname.need(n4 + x4) != BMH_OK || seqoff.need(n4 + x4) != BMH_OK || rclen.need(n4 + x4) != BMH_OK || rleft.need(n4 + x4) != BMH_OK ||
		    ctl.need(sizeof(bin_ctl_t)) != BMH_OK) return BMH_ENOMEM;
		uint32_t *hs = h_small.as<uint32_t>();
		const uint8_t *db = b.as<uint8_t>();
		const uint32_t *ds = starts.as<uint32_t>();
		bin_ctl_t *dctl = ctl.as<bin_ctl_t>();
		const bool rg = S.keep_rg();
		if (rg && grp.need(n4 + x4) != BMH_OK) return BMH_ENOMEM;
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
		if (S.collate()) return collate(S, w, alloc, rs, R, chain, nkept, qual, M, G, rg);
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

// every option of the step in one call: flags may hold BMH_READS_HOST (the host form, no device), rg_ids may be NULL, collate_mem caps the collation's open records
extern "C" int bmh_bam_reads_ex(const uint8_t *records, uint64_t n_bytes, int flags, const char *const *rg_ids, int n_groups, uint64_t collate_mem, bmh_read_set_t *out)
{
	if ((!records && n_bytes) || !out) { bmh_set_error("bmh_bam_reads_ex: null argument"); return BMH_EINVAL; }
	if (flags & BMH_READS_HOST) return bmh_bam_reads_run("bmh_bam_reads_ex", nullptr, records, n_bytes, flags, out, rg_ids, n_groups, collate_mem);
	int nd = 0;
	if (hipGetDeviceCount(&nd) != hipSuccess || nd == 0) { (void)hipGetLastError(); bmh_set_error("bmh_bam_reads_ex: no HIP device (BMH_READS_HOST decodes on the host)"); return BMH_ENODEV; }
	bmh_bam_dev_t d;
	return bmh_bam_reads_run("bmh_bam_reads_ex", &d, records, n_bytes, flags, out, rg_ids, n_groups, collate_mem);
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
