// csrc/bam_dup_core.h and the host forms of csrc/bam_dup_host.cpp as plain C++ for tests/test_bam_dup.py, built with -fsanitize=address,undefined: every stream
// sits in an allocation of exactly its size.
//   in : u32 n_cases, per case u64 n_bytes and the record stream
//   out: per case i32 status (0, or -2: refused -- cut, no template at its head, a paired template without both primary lines); for status 0: u32 n records,
//        u16 flag of every record after marking, u64 counts[8]
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
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
		uint64_t nb;
		if (fread(&nb, 8, 1, f) != 1) return 2;
		uint8_t *all = new uint8_t[nb ? nb : 1];
		if (nb && fread(all, 1, nb, f) != nb) return 2;
		std::vector<uint64_t> off(1, 0);
		int32_t rc = BMH_OK;
		for (uint64_t p = 0; p < nb;) {
			const uint64_t sz = bsr_record_bytes(all + p, nb - p);
			if (!sz) { rc = BMH_EINVAL; break; }
			p += sz; off.push_back(p);
		}
		uint64_t counts[BDP_N_COUNTS];
		if (rc == BMH_OK) rc = bdp_markdup_host(all, off, counts, "test", bdp_plan_t());
		fwrite(&rc, 4, 1, o);
		if (rc == BMH_OK) {
			const uint32_t n = (uint32_t)(off.size() - 1);
			fwrite(&n, 4, 1, o);
			for (uint32_t i = 0; i < n; ++i) { const uint16_t fl = (uint16_t)bsr_flag(all + off[i]); fwrite(&fl, 2, 1, o); }
			fwrite(counts, 8, BDP_N_COUNTS, o);
		}
		delete[] all;
	}
	fclose(o); fclose(f);
	return 0;
}
