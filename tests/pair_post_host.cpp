// The host walk of interleaved pairs (csrc/pair_post.cpp: bmh_finalize_pairs, no mate rescue) as a plain C++ program for tests/test_pair_dev.py, built with
// -fsanitize=address,undefined together with the host sources it needs: every array of the case lives in a heap block of exactly its size.  The device entry
// points the walk can call with a device (never without one) are stubs that fail.
// usage: pair_post_host <case file> <result file>
//   case:   int32 n_reads, n_regs, n_contigs, read length, has_alt, sizeof of the four option structs; the structs (chain, extension, post, pair); uint8 alt[n_contigs];
//           int64 contig offsets; int32 contig lengths; int64 l_pac; the 2-bit reference (l_pac / 4 + 2 bytes); the reads' codes; regions [n_regs][8]; regions per read; frac_rep
//   result: int64 m; records [m][16]; per read; h_rec; unflag; pes [4][5]
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include "../include/bwamem_hip.h"
#include "../bwa-mem_gpu_amd/csrc/pair_kernels.h"

static char g_err[512];
extern "C" void bmh_set_error(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap); }
extern "C" int bmh_tune(const char *, int dflt) { return dflt; }
int bmh_matesw_device_takes(int, int64_t, int) { return 0; }
int bmh_matesw_batch_device(const bmh_index_t *, const uint8_t *, const uint32_t *, const bmh_ext_params_t *, bmh_msw_job_t *, uint64_t, int32_t *, void *) { return BMH_EINVAL; }
int64_t bmh_rescue_count_device(const bmh_index_t *, const bmh_rescue_in_t *, const bmh_ext_params_t *, int, const bmh_pe_opt_t *, const double *, uint32_t, uint32_t *, uint8_t *, void *) { return BMH_EINVAL; }
int bmh_rescue_run_device(const bmh_index_t *, const uint8_t *, const uint32_t *, const bmh_ext_params_t *, bmh_msw_key_t *, int32_t *, void *) { return BMH_EINVAL; }

template <class T> static std::unique_ptr<T[]> take(FILE *f, size_t n)
{
	std::unique_ptr<T[]> p(new T[n ? n : 1]);
	if (n && fread(p.get(), sizeof(T), n, f) != n) { fprintf(stderr, "pair_post_host: short case file\n"); exit(2); }
	return p;
}

int main(int argc, char **argv)
{
	if (argc != 3) { fprintf(stderr, "usage: pair_post_host <case file> <result file>\n"); return 2; }
	FILE *f = fopen(argv[1], "rb");
	if (!f) { perror(argv[1]); return 2; }
	auto hd = take<int32_t>(f, 9);
	const size_t n = (size_t)hd[0], nr = (size_t)hd[1], nc = (size_t)hd[2], L = (size_t)hd[3];
	if (hd[5] != (int)sizeof(bmh_chain_opt_t) || hd[6] != (int)sizeof(bmh_ext_params_t) || hd[7] != (int)sizeof(bmh_post_opt_t) || hd[8] != (int)sizeof(bmh_pe_opt_t)) { fprintf(stderr, "pair_post_host: the option structs have other sizes here\n"); return 2; }
	auto co = take<bmh_chain_opt_t>(f, 1); auto ep = take<bmh_ext_params_t>(f, 1); auto po = take<bmh_post_opt_t>(f, 1); auto pe = take<bmh_pe_opt_t>(f, 1);
	auto alt = take<uint8_t>(f, nc); auto off = take<int64_t>(f, nc); auto len = take<int32_t>(f, nc); auto lp = take<int64_t>(f, 1);
	auto pac = take<uint8_t>(f, (size_t)(lp[0] / 4 + 2)); auto reads = take<uint8_t>(f, n * L); auto regs = take<int32_t>(f, 8 * nr); auto rpr = take<uint32_t>(f, n); auto fr = take<float>(f, n);
	fclose(f);
	co[0].contig_is_alt = hd[4] ? alt.get() : nullptr; po[0].contig_is_alt = hd[4] ? alt.get() : nullptr; po[0].rg_id = nullptr;
	std::unique_ptr<uint64_t[]> offs(new uint64_t[n ? n : 1]); std::unique_ptr<uint32_t[]> lens(new uint32_t[n ? n : 1]);
	for (size_t r = 0; r < n; ++r) { offs[r] = r * L; lens[r] = (uint32_t)L; }
	const uint64_t cap = nr;                                          // (without the rescue nothing is added)
	std::unique_ptr<int32_t[]> out(new int32_t[16 * (cap ? cap : 1)]), h(new int32_t[n ? n : 1]), uf(new int32_t[n ? n : 1]);
	std::unique_ptr<uint32_t[]> opr(new uint32_t[n ? n : 1]);
	double pes[20];
	const int64_t m = bmh_finalize_pairs(co.get(), ep.get(), po.get(), pe.get(), lp[0], pac.get(), (uint32_t)n, reads.get(), offs.get(), lens.get(), regs.get(), rpr.get(), fr.get(),
	                                     (int)nc, nc > 1 ? off.get() : nullptr, nc > 1 ? len.get() : nullptr, out.get(), cap, opr.get(), h.get(), uf.get(), pes, 3);
	if (m < 0) { fprintf(stderr, "pair_post_host: bmh_finalize_pairs: %lld: %s\n", (long long)m, g_err); return 1; }
	FILE *o = fopen(argv[2], "wb");
	if (!o) { perror(argv[2]); return 2; }
	fwrite(&m, 8, 1, o); fwrite(out.get(), 64, (size_t)m, o); fwrite(opr.get(), 4, n, o); fwrite(h.get(), 4, n, o); fwrite(uf.get(), 4, n, o); fwrite(pes, 8, 20, o);
	return fclose(o) == 0 ? 0 : 2;
}
