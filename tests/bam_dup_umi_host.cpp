// The barcode rules of csrc/bam_dup_core.h and csrc/bam_dup_host.cpp -- the barcode word, the name's last field, the tag walk, the widened keys through
// bdp_markdup_host -- as plain C++ for tests/test_bam_umi.py, built with -fsanitize=address,undefined: every value, every name and every stream sits in an
// allocation of exactly its size.
//   in : u32 n_values, per value u32 len and the bytes; u32 n_names, per name u32 len and the bytes; u32 n_cases, per case u32 mode, 2 tag bytes, i64 distance
//        (-1: no optical step), u32 max_set, u32 n_groups, per group u32 len, the ID, i32 library; u64 n_bytes and the record stream
//   out: per value u64 word; per name u32 where the last field begins (len + 1: none), u32 the length the location parser is given; per case i32 status; for
//        status 0: u32 T, T words of 8 bytes, u64 counts[8], u64 no_barcode, u64 optical[3], u32 n_lib, u64 lib_counts[8 * n_lib], u64 lib_optical[3 * n_lib],
//        the marked stream (n_bytes); for any other status: u32 len and the message
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

// len bytes of the file in an allocation of exactly that size (of one byte for none, never read)
static uint8_t *exact(FILE *f, uint64_t len)
{
	uint8_t *p = new uint8_t[len ? len : 1];
	if (len && fread(p, 1, len, f) != len) { delete[] p; return nullptr; }
	return p;
}

int main(int argc, char **argv)
{
	if (argc != 3) return 2;
	FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
	if (!f || !o) return 2;
	uint32_t n_values, n_names, n_cases;
	if (!get(f, &n_values)) return 2;
	for (uint32_t k = 0; k < n_values; ++k) {
		uint32_t len;
		if (!get(f, &len)) return 2;
		uint8_t *v = exact(f, len);
		if (!v) return 2;
		const uint64_t w = bdp_barcode_word(v, len);
		fwrite(&w, 8, 1, o);
		delete[] v;
	}
	if (!get(f, &n_names)) return 2;
	for (uint32_t k = 0; k < n_names; ++k) {
		uint32_t len;
		if (!get(f, &len)) return 2;
		uint8_t *name = exact(f, len);
		if (!name) return 2;
		const uint32_t a = bdp_name_last_field(name, len), cut = bdp_located_name_len(name, len, true);
		fwrite(&a, 4, 1, o); fwrite(&cut, 4, 1, o);
		delete[] name;
	}
	if (!get(f, &n_cases)) return 2;
	for (uint32_t c = 0; c < n_cases; ++c) {
		uint32_t mode, max_set, n_groups; char tag[2]; int64_t D; uint64_t nb;
		if (!get(f, &mode) || fread(tag, 1, 2, f) != 2 || !get(f, &D) || !get(f, &max_set) || !get(f, &n_groups)) return 2;
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
		uint8_t *all = exact(f, nb);
		if (!all) return 2;
		std::vector<uint64_t> off(1, 0);
		int32_t rc = BMH_OK;
		g_msg[0] = 0;
		for (uint64_t p = 0; p < nb;) {
			const uint64_t sz = bsr_record_bytes(all + p, nb - p);
			if (!sz) { rc = BMH_EINVAL; break; }
			p += sz; off.push_back(p);
		}
		bdp_plan_t P; bdp_table_t &T = P.table; bdp_bc_t &bc = P.bc;
		if (rc == BMH_OK && n_groups) rc = bdp_table_make(T, idp.data(), lib.data(), (int)n_groups, "test");
		if (rc == BMH_OK) rc = bdp_barcode_check((int)mode, tag, "test", &bc);
		if (rc == BMH_OK && D != -1) rc = bdp_optical_check(D, max_set, "test");
		const uint32_t n = (uint32_t)(off.size() - 1);
		for (uint32_t i = 0; rc == BMH_OK && i < n; ++i) if (!bdp_record_whole(all + off[i], off[i + 1] - off[i])) rc = BMH_EINVAL;
		// the words on their own, then the whole of it
		std::vector<uint32_t> tpl; std::vector<bdp_entry_t> E; std::vector<uint64_t> W; uint64_t info[2] = {0, 0};
		if (rc == BMH_OK) rc = bdp_entries_host(all, off.data(), n, tpl, E, info, "test", P, nullptr, &W);
		uint64_t counts[BDP_N_COUNTS], opt[BDP_OPT_N] = {0, 0, 0}, no_bc = 0;
		std::vector<uint64_t> lib_counts((size_t)BDP_N_COUNTS * T.n_lib + 1), lib_opt((size_t)BDP_OPT_N * T.n_lib + 1);
		if (D != -1) P.opt = {D, max_set ? max_set : (uint32_t)BDP_OPT_MAX_SET, opt, n_groups ? lib_opt.data() : nullptr};
		P.lib_counts = n_groups ? lib_counts.data() : nullptr; P.no_barcode = &no_bc;
		if (rc == BMH_OK) rc = bdp_markdup_host(all, off, counts, "test", P);
		fwrite(&rc, 4, 1, o);
		if (rc == BMH_OK) {
			const uint32_t nt = (uint32_t)W.size(), nl = n_groups ? T.n_lib : 0;
			fwrite(&nt, 4, 1, o);
			if (nt) fwrite(W.data(), 8, nt, o);
			fwrite(counts, 8, BDP_N_COUNTS, o); fwrite(&no_bc, 8, 1, o); fwrite(opt, 8, BDP_OPT_N, o);
			fwrite(&nl, 4, 1, o);
			if (nl) { fwrite(lib_counts.data(), 8, (size_t)BDP_N_COUNTS * nl, o); fwrite(lib_opt.data(), 8, (size_t)BDP_OPT_N * nl, o); }
			if (nb) fwrite(all, 1, nb, o);
		} else {
			const uint32_t len = (uint32_t)strlen(g_msg);
			fwrite(&len, 4, 1, o); fwrite(g_msg, 1, len, o);
		}
		delete[] all;
	}
	fclose(o); fclose(f);
	return 0;
}
