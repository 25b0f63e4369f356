// csrc/bam_post_core.h and the host heads / check path (bdp_entries_host under BDP_TPL_NAME, csrc/bam_dup_host.cpp) as plain C++ for tests/test_bam_post.py, built
// with -fsanitize=address,undefined: every stream sits in an allocation of exactly its size, so a read past a record's end is a finding.
//   in : u32 n_cases, per case i32 n_ref, u32 mode (1: marking, 2: coverage), u64 n_bytes and the record stream (cut by block_size; bytes behind the last whole
//        record are left alone)
//   out: per case u32 n records; per record i32 code (bpo_fix; 0: taken), u16 bin and u16 flag afterwards, u8 head (bpo_head); then i32 status of
//        bdp_entries_host over the records before the first refused one's template (0, or -2) and, for 0, u32 n_templates
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
		int32_t n_ref; uint32_t mode; uint64_t nb;
		if (fread(&n_ref, 4, 1, f) != 1 || fread(&mode, 4, 1, f) != 1 || fread(&nb, 8, 1, f) != 1) return 2;
		uint8_t *all = new uint8_t[nb ? nb : 1];
		if (nb && fread(all, 1, nb, f) != nb) return 2;
		std::vector<uint64_t> off(1, 0);
		for (uint64_t p = 0; nb - p >= 4;) {                          // the chain: block_size alone says where the next record begins
			const uint64_t e = p + 4 + bsr_u32(all + p);
			if (e > nb) break;
			off.push_back(e); p = e;
		}
		const uint32_t n = (uint32_t)(off.size() - 1);
		fwrite(&n, 4, 1, o);
		uint32_t first_bad = n;
		for (uint32_t i = 0; i < n; ++i) {
			uint32_t changed = 0;
			const uint64_t sz = off[i + 1] - off[i];
			const int32_t code = bpo_fix(all + off[i], sz, n_ref, mode, &changed);
			if (code != BPO_OK && first_bad == n) first_bad = i;
			const uint16_t bin = sz >= BSR_FIXED ? (uint16_t)bsr_bin(all + off[i]) : 0, fl = sz >= BSR_FIXED ? (uint16_t)bsr_flag(all + off[i]) : 0;
			const uint8_t head = bpo_head(all, off.data(), i) ? 1 : 0;
			fwrite(&code, 4, 1, o); fwrite(&bin, 2, 1, o); fwrite(&fl, 2, 1, o); fwrite(&head, 1, 1, o);
		}
		uint32_t n_ok = first_bad;
		while (n_ok > 0 && n_ok < n && !bpo_head(all, off.data(), n_ok)) --n_ok;
		std::vector<uint32_t> tpl; std::vector<bdp_entry_t> E; uint64_t info[2] = {0, 0};
		const int32_t rc = bdp_entries_host(all, off.data(), n_ok, tpl, E, info, "test", bdp_plan_t(), nullptr, nullptr, BDP_TPL_NAME, 0);
		fwrite(&rc, 4, 1, o);
		if (rc == BMH_OK) { const uint32_t nt = (uint32_t)E.size(); fwrite(&nt, 4, 1, o); }
		delete[] all;
	}
	fclose(o); fclose(f);
	return 0;
}
