// The optical step of csrc/bam_dup_core.h and csrc/bam_dup_host.cpp -- the name parser, the templates' locations, the clustering core through bdp_optical_host -- as
// plain C++ for tests/test_bam_optical.py, built with -fsanitize=address,undefined: every name and every stream sits in an allocation of exactly its size.
//   in : u32 n_names, per name u32 len and the bytes; u32 n_cases, per case i64 distance, u32 max_set, u32 n_groups, per group u32 len, the ID, i32 library;
//        u64 n_bytes and the record stream
//   out: per name i32 located, u32 tile, x, y; per case i32 status; for status 0: u32 T, T locations of 16 bytes, u64 counts[8], u64 optical[3], u32 n_lib,
//        u64 lib_optical[3 * n_lib]
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#define BDP_STANDALONE
#include "../bwa-mem_gpu_amd/csrc/bam_dup_host.cpp"

static char g_msg[512];
void bmh_set_error(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_msg, sizeof g_msg, fmt, ap); va_end(ap); }

template <class T> static bool get(FILE *f, T *v) { return fread(v, sizeof(T), 1, f) == 1; }

int main(int argc, char **argv)
{
	if (argc != 3) return 2;
	FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
	if (!f || !o) return 2;
	uint32_t n_names, n_cases;
	if (!get(f, &n_names)) return 2;
	for (uint32_t k = 0; k < n_names; ++k) {
		uint32_t len;
		if (!get(f, &len)) return 2;
		uint8_t *name = new uint8_t[len ? len : 1];
		if (len && fread(name, 1, len, f) != len) return 2;
		uint32_t v[3] = {0, 0, 0};
		const int32_t ok = bdp_name_location(name, len, v) ? 1 : 0;
		fwrite(&ok, 4, 1, o); fwrite(v, 4, 3, o);
		delete[] name;
	}
	if (!get(f, &n_cases)) return 2;
	for (uint32_t c = 0; c < n_cases; ++c) {
		int64_t D; uint32_t max_set, n_groups; uint64_t nb;
		if (!get(f, &D) || !get(f, &max_set) || !get(f, &n_groups)) return 2;
		std::vector<std::string> ids(n_groups); std::vector<const char *> idp; std::vector<int32_t> lib(n_groups);
		for (uint32_t g = 0; g < n_groups; ++g) {
			uint32_t len;
			if (!get(f, &len)) return 2;
			ids[g].resize(len);
			if (len && fread(&ids[g][0], 1, len, f) != len) return 2;
			if (!get(f, &lib[g])) return 2;
		}
		for (const std::string &s : ids) idp.push_back(s.c_str());
		if (!get(f, &nb)) return 2;
		uint8_t *all = new uint8_t[nb ? nb : 1];
		if (nb && fread(all, 1, nb, f) != nb) return 2;
		std::vector<uint64_t> off(1, 0);
		int32_t rc = BMH_OK;
		for (uint64_t p = 0; p < nb;) {
			const uint64_t sz = bsr_record_bytes(all + p, nb - p);
			if (!sz) { rc = BMH_EINVAL; break; }
			p += sz; off.push_back(p);
		}
		bdp_plan_t P; bdp_table_t &T = P.table;
		if (rc == BMH_OK && n_groups) rc = bdp_table_make(T, idp.data(), lib.data(), (int)n_groups, "test");
		if (rc == BMH_OK) rc = bdp_optical_check(D, max_set, "test");
		const uint32_t n = (uint32_t)(off.size() - 1);
		for (uint32_t i = 0; rc == BMH_OK && i < n; ++i) if (!bdp_record_whole(all + off[i], off[i + 1] - off[i])) rc = BMH_EINVAL;
		// the locations on their own, then the whole of it
		std::vector<uint32_t> tpl; std::vector<bdp_entry_t> E; std::vector<bdp_loc_t> L; uint64_t info[2] = {0, 0};
		if (rc == BMH_OK) rc = bdp_entries_host(all, off.data(), n, tpl, E, info, "test", P, &L);
		uint64_t counts[BDP_N_COUNTS], opt[BDP_OPT_N];
		std::vector<uint64_t> lib_counts((size_t)BDP_N_COUNTS * T.n_lib + 1), lib_opt((size_t)BDP_OPT_N * T.n_lib + 1);
		P.opt = {D, max_set ? max_set : (uint32_t)BDP_OPT_MAX_SET, opt, n_groups ? lib_opt.data() : nullptr}; P.lib_counts = n_groups ? lib_counts.data() : nullptr;
		if (rc == BMH_OK) rc = bdp_markdup_host(all, off, counts, "test", P);
		fwrite(&rc, 4, 1, o);
		if (rc == BMH_OK) {
			const uint32_t nt = (uint32_t)L.size(), nl = n_groups ? T.n_lib : 0;
			fwrite(&nt, 4, 1, o);
			if (nt) fwrite(L.data(), sizeof(bdp_loc_t), nt, o);
			fwrite(counts, 8, BDP_N_COUNTS, o); fwrite(opt, 8, BDP_OPT_N, o);
			fwrite(&nl, 4, 1, o);
			if (nl) fwrite(lib_opt.data(), 8, (size_t)BDP_OPT_N * nl, o);
		}
		delete[] all;
	}
	fclose(o); fclose(f);
	return 0;
}
