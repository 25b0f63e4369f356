// csrc/bam_dup_core.h's library rules and the host forms of csrc/bam_dup_host.cpp with read groups, as plain C++ for tests/test_read_groups.py, built with
// -fsanitize=address,undefined: every stream sits in an allocation of exactly its size, and so does every ID of the table.
//   in : u32 n_cases, per case u32 n_groups, per group u8 id_len, the ID's bytes and i32 library; then u64 n_bytes and the record stream
//   out: per case i32 status (0, or -2: refused -- the table, a cut stream, a template without a known read group, ...); for status 0: u32 n records, u16 flag of
//        every record after marking, u64 counts[8], u32 n_lib, u64 lib_counts[8 * n_lib]
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

int main(int argc, char **argv)
{
	if (argc != 3) return 2;
	FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
	if (!f || !o) return 2;
	uint32_t n_cases;
	if (fread(&n_cases, 4, 1, f) != 1) return 2;
	for (uint32_t c = 0; c < n_cases; ++c) {
		uint32_t ng;
		if (fread(&ng, 4, 1, f) != 1) return 2;
		std::vector<char *> ids; std::vector<int32_t> lib;
		for (uint32_t g = 0; g < ng; ++g) {
			uint8_t l; int32_t v;
			if (fread(&l, 1, 1, f) != 1) return 2;
			char *id = new char[(size_t)l + 1];
			if (l && fread(id, 1, l, f) != l) return 2;
			id[l] = 0;
			if (fread(&v, 4, 1, f) != 1) return 2;
			ids.push_back(id); lib.push_back(v);
		}
		uint64_t nb;
		if (fread(&nb, 8, 1, f) != 1) return 2;
		uint8_t *all = new uint8_t[nb ? nb : 1];
		if (nb && fread(all, 1, nb, f) != nb) return 2;
		bdp_plan_t P; bdp_table_t &T = P.table;
		int32_t rc = bdp_table_make(T, ids.data(), lib.data(), (int)ng, "test");
		for (char *id : ids) delete[] id;                          // (the table keeps its own copy of the IDs)
		std::vector<uint64_t> off(1, 0);
		for (uint64_t p = 0; rc == BMH_OK && p < nb;) {
			const uint64_t sz = bsr_record_bytes(all + p, nb - p);
			if (!sz) { rc = BMH_EINVAL; break; }
			p += sz; off.push_back(p);
		}
		uint64_t counts[BDP_N_COUNTS];
		std::vector<uint64_t> lc((size_t)BDP_N_COUNTS * (T.n_lib ? T.n_lib : 1), 0);
		P.lib_counts = lc.data();
		if (rc == BMH_OK) rc = bdp_markdup_host(all, off, counts, "test", P);
		fwrite(&rc, 4, 1, o);
		if (rc == BMH_OK) {
			const uint32_t n = (uint32_t)(off.size() - 1);
			fwrite(&n, 4, 1, o);
			for (uint32_t i = 0; i < n; ++i) { const uint16_t fl = (uint16_t)bsr_flag(all + off[i]); fwrite(&fl, 2, 1, o); }
			fwrite(counts, 8, BDP_N_COUNTS, o);
			fwrite(&T.n_lib, 4, 1, o);
			fwrite(lc.data(), 8, (size_t)BDP_N_COUNTS * T.n_lib, o);
		}
		delete[] all;
	}
	fclose(o); fclose(f);
	return 0;
}
