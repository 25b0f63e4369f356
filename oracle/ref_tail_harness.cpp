/*
 * oracle/ref_tail_harness.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Thin driver around the REFERENCE's own region tail: mem_sort_dedup_patch, mem_mark_primary_se and mem_approx_mapq_se
 * (src/bwamem.c:620-680, 715-761, 1690-1717), compiled by oracle/Makefile (target _ref/libref_tail.so) from where the reference
 * lies, unchanged.  The driver fills arrays of mem_alnreg_t from this project's region records ([n][8]: bmh_merge_regs' layout)
 * the way mem_align1_core leaves them when it hands them to the tail (src/bwamem.c:2297-2325: truesc = score, w = opt->w, the
 * sequence and is_alt of every region, frac_rep of the read), runs the three functions and writes the regions back as records
 * of 16 ints.  It pins bmh_finalize_regs (csrc/regs_post.cpp) to the reference on inputs natural data does not produce: ties
 * of every sort key, collisions of the tie-break hash, long tandem windows (tests/test_regs_cases.py).  A second entry point,
 * ref_tail_reg2aln, runs the reference's mem_reg2aln on one region (tests/cigar_cases.py, tests/golden/make_cigar_golden.py).
 *
 * The reference reads the genome through bns->l_pac and pac only on this path (bwa_gen_cigar2 -> bns_get_seq), so the
 * bntseq_t is one in memory with nothing but l_pac (ref_tail_reg2aln adds one contig: mem_reg2aln looks the position up).  bwamem.c names five data globals that fastmap.c defines; they are
 * defined here (never read on this path).  The GASAL entry points stay unresolved (the library is loaded lazily) and are
 * never called.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "bntseq.h"
#include "bwa.h"
#include "bwamem.h"

/* the reference's, defined in src/bwamem.c without a declaration in its headers (C++ linkage: the reference is compiled as C++) */
int mem_sort_dedup_patch(const mem_opt_t *opt, const bntseq_t *bns, const uint8_t *pac, uint8_t *query, int n, mem_alnreg_t *a);
int mem_mark_primary_se(const mem_opt_t *opt, int n, mem_alnreg_t *a, int64_t id);
int mem_approx_mapq_se(const mem_opt_t *opt, const mem_alnreg_t *a);

/* what src/fastmap.c defines for src/bwamem.c (timing counters of the reference's extension, its GPU storage); types are
 * irrelevant to the linker, nothing on this path reads them */
extern "C" {
void *extension_time = 0;
void *no_of_extensions = 0;
void *load_balance_waste_time = 0;
double total_load_balance_waste_time = 0;
void *gpu_storage_vec_arr = 0;
}

/*
 * opt_i = {a, b, o_del, e_del, o_ins, e_ins, w, min_seed_len, max_chain_gap, mapQ_coef_fac}
 * opt_f = {mask_level, mask_level_redun, mapQ_coef_len}
 * query: the read as codes 0..4; regs8 [n][8] = {-, score, qb, qe, rb_lo, rb_hi, re_lo, re_hi}; rid / is_alt per region.
 * out [n][16] = {-, score, qb, qe, rb_lo, rb_hi, re_lo, re_hi, truesc, w, sub, sub_n, secondary, mem_approx_mapq_se (secondary < 0) or 0,
 *                secondary_all, is_alt | alt_sc << 2}, in the order mem_mark_primary_se leaves the regions.  Returns their number.
 */
extern "C" int ref_tail_run(const int *opt_i, const float *opt_f, int64_t l_pac, const uint8_t *pac, int l_query, const uint8_t *query,
                            int64_t id, float frac_rep, int n, const int32_t *regs8, const int32_t *rid, const uint8_t *is_alt, int32_t *out)
{
	mem_opt_t *opt = mem_opt_init();
	opt->a = opt_i[0]; opt->b = opt_i[1]; opt->o_del = opt_i[2]; opt->e_del = opt_i[3]; opt->o_ins = opt_i[4]; opt->e_ins = opt_i[5];
	opt->w = opt_i[6]; opt->min_seed_len = opt_i[7]; opt->max_chain_gap = opt_i[8]; opt->mapQ_coef_fac = opt_i[9];
	opt->mask_level = opt_f[0]; opt->mask_level_redun = opt_f[1]; opt->mapQ_coef_len = opt_f[2];
	bwa_fill_scmat(opt->a, opt->b, opt->mat);
	bntseq_t bns;
	memset(&bns, 0, sizeof(bns));
	bns.l_pac = l_pac;
	mem_alnreg_t *a = (mem_alnreg_t *)calloc(n > 0 ? n : 1, sizeof(mem_alnreg_t));
	uint8_t *q = (uint8_t *)malloc(l_query > 0 ? l_query : 1);      /* (bwa_gen_cigar2 reverses the query in place and back) */
	memcpy(q, query, l_query);
	for (int i = 0; i < n; ++i) {
		const int32_t *r = regs8 + 8 * (size_t)i;
		mem_alnreg_t *p = &a[i];
		p->score = p->truesc = r[1]; p->qb = r[2]; p->qe = r[3];
		p->rb = (int64_t)(uint32_t)r[4] | (int64_t)r[5] << 32; p->re = (int64_t)(uint32_t)r[6] | (int64_t)r[7] << 32;
		p->w = opt->w; p->rid = rid[i]; p->is_alt = is_alt ? is_alt[i] : 0; p->frac_rep = frac_rep;
		p->secondary = p->secondary_all = -1;
	}
	int m = mem_sort_dedup_patch(opt, &bns, pac, q, n, a);
	mem_mark_primary_se(opt, m, a, id);
	for (int i = 0; i < m; ++i) {
		const mem_alnreg_t *p = &a[i];
		int32_t *o = out + 16 * (size_t)i;
		o[0] = 0; o[1] = p->score; o[2] = p->qb; o[3] = p->qe;
		o[4] = (int32_t)(uint32_t)p->rb; o[5] = (int32_t)(p->rb >> 32); o[6] = (int32_t)(uint32_t)p->re; o[7] = (int32_t)(p->re >> 32);
		o[8] = p->truesc; o[9] = p->w; o[10] = p->sub; o[11] = p->sub_n; o[12] = p->secondary;
		o[13] = p->secondary < 0 ? mem_approx_mapq_se(opt, p) : 0;
		o[14] = p->secondary_all; o[15] = (p->is_alt ? 1 : 0) | p->alt_sc << 2;
	}
	free(q); free(a); free(opt);
	return m;
}

/*
 * The reference's unchanged mem_reg2aln (src/bwamem.c:2344-2438: band inference, the retry loop, bwa_gen_cigar2 with the strand
 * flip, NM and MD, the squeeze of a leading / trailing deletion, the clips) on one region of one read.  It pins oracle_reg2aln and
 * csrc/cigar_kernels.hip on the hand-made regions of tests/cigar_cases.py.
 *
 * opt_i = {a, b, o_del, e_del, o_ins, e_ins, w}; the genome is one contig of l_pac bases; read: the letters as they stand in the
 * FASTQ record (mem_reg2aln converts them); reg = {qb, qe, truesc, w} and [rb, re) of a mem_alnreg_t with rid 0, secondary -1 and
 * score = truesc.  The region must be one bwa_gen_cigar2 accepts (not empty, not bridging the strands): for the others the
 * reference has no CIGAR to return.
 * out = {pos_lo, pos_hi, is_rev, n_cigar, NM, l_MD}; cigar (capacity cap) and md (capacity md_cap, NUL terminated) receive what
 * fits.  Returns 0, or -1 where a capacity was too small.
 */
extern "C" int ref_tail_reg2aln(const int *opt_i, int64_t l_pac, const uint8_t *pac, int l_query, const char *read, const int32_t *reg,
                                int64_t rb, int64_t re, int32_t *out, uint32_t *cigar, int cap, char *md, int md_cap)
{
	mem_opt_t *opt = mem_opt_init();
	opt->a = opt_i[0]; opt->b = opt_i[1]; opt->o_del = opt_i[2]; opt->e_del = opt_i[3]; opt->o_ins = opt_i[4]; opt->e_ins = opt_i[5];
	opt->w = opt_i[6];
	bwa_fill_scmat(opt->a, opt->b, opt->mat);
	bntann1_t ann;
	memset(&ann, 0, sizeof(ann));
	ann.offset = 0; ann.len = (int32_t)l_pac;
	bntseq_t bns;
	memset(&bns, 0, sizeof(bns));
	bns.l_pac = l_pac; bns.n_seqs = 1; bns.anns = &ann;
	mem_alnreg_t ar;
	memset(&ar, 0, sizeof(ar));
	ar.qb = reg[0]; ar.qe = reg[1]; ar.score = ar.truesc = reg[2]; ar.w = reg[3];
	ar.rb = rb; ar.re = re; ar.rid = 0; ar.secondary = ar.secondary_all = -1;
	mem_aln_t a = mem_reg2aln(opt, &bns, pac, l_query, read, &ar);
	const char *m = (const char *)(a.cigar + a.n_cigar);
	const int l_md = (int)strlen(m);
	out[0] = (int32_t)(uint32_t)a.pos; out[1] = (int32_t)(a.pos >> 32); out[2] = a.is_rev; out[3] = a.n_cigar; out[4] = (int32_t)a.NM; out[5] = l_md;
	for (int i = 0; i < a.n_cigar && i < cap; ++i) cigar[i] = a.cigar[i];
	if (md_cap > 0) { const int n = l_md < md_cap - 1 ? l_md : md_cap - 1; memcpy(md, m, n); md[n] = 0; }
	const int rc = (a.n_cigar > cap || l_md + 1 > md_cap) ? -1 : 0;
	free(a.cigar); free(opt);
	return rc;
}
