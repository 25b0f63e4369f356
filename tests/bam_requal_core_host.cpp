// csrc/bam_requal_core.h and the host form of csrc/bam_requal.h as plain C++ for tests/test_bam_requal.py, built with -fsanitize=address,undefined.  Every record
// stream sits between two rows of canary bytes, which are checked behind the run: the host form writes quality bytes and nothing else.
//   in : u32 n_cases, then per case i32 n_groups (0: the one group `*`, no IDs), i32 min_qual, i32 max_cycle, the group IDs (NUL-terminated each),
//        cycle_m (groups x 94 x 2 max_cycle x 2 u64), context_m (groups x 94 x 17 x 2 u64), u32 window (records; 0: all in one), u64 n_bytes and the record stream
//   out: i32 status (0; -2: refused; -3: a canary was overwritten), u64 the refused record's index, i32 its code (0: the table or the stream itself was refused);
//        for status 0 the int16 tables, the stream as rewritten, the counts' words
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#define BRC_STANDALONE
#include "../bwa-mem_gpu_amd/csrc/bam_recal.h"

static char g_msg[512];
void bmh_set_error(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_msg, sizeof g_msg, fmt, ap); va_end(ap); }

static bool get(FILE *f, void *p, size_t n) { return !n || fread(p, 1, n, f) == n; }
static bool get_name(FILE *f, std::string &s) { s.clear(); for (int c; (c = fgetc(f)) != EOF;) { if (!c) return true; s.push_back((char)c); } return false; }

enum { CANARY = 64 };

int main(int argc, char **argv)
{
	if (argc != 3) return 2;
	FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
	if (!f || !o) return 2;
	uint32_t n_cases;
	if (!get(f, &n_cases, 4)) return 2;
	for (uint32_t c = 0; c < n_cases; ++c) {
		int32_t ng, min_qual, max_cycle; uint32_t window; uint64_t nb;
		if (!get(f, &ng, 4) || !get(f, &min_qual, 4) || !get(f, &max_cycle, 4)) return 2;
		std::vector<std::string> ids((size_t)ng); std::vector<const char *> idp;
		for (std::string &s : ids) if (!get_name(f, s)) return 2;
		for (const std::string &s : ids) idp.push_back(s.c_str());
		const size_t g = ng ? (size_t)ng : 1, ncy = g * 94 * 2 * (size_t)max_cycle * 2, ncx = g * 94 * 17 * 2;
		uint64_t *cy = new uint64_t[ncy], *cx = new uint64_t[ncx];           // (exactly their size: the table's checks read no word beyond)
		if (!get(f, cy, 8 * ncy) || !get(f, cx, 8 * ncx) || !get(f, &window, 4) || !get(f, &nb, 8)) return 2;
		uint8_t *all = new uint8_t[nb + 2 * CANARY];
		memset(all, 0xa5, nb + 2 * CANARY);
		uint8_t *recs = all + CANARY;
		if (!get(f, recs, nb)) return 2;
		std::vector<uint64_t> off(1, 0);
		int32_t rc = BMH_OK, code = 0; uint64_t index = 0;
		for (uint64_t p = 0; p < nb;) {
			const uint64_t sz = bsr_record_bytes(recs + p, nb - p);
			if (!sz) { rc = BMH_EINVAL; break; }
			p += sz; off.push_back(p);
		}
		brq_run_t U; brq_host_t H;
		if (rc == BMH_OK) rc = brq_run_make(U, (int32_t)g, min_qual, max_cycle, 94, cy, cx, ng ? idp.data() : nullptr, "test");
		if (rc == BMH_OK) {
			H.begin(U);
			const size_t n = off.size() - 1, W = window ? window : (n ? n : 1);
			for (size_t a = 0; a < n && rc == BMH_OK; a += W) rc = H.window(recs, off.data() + a, (uint32_t)((a + W < n ? a + W : n) - a), "test");
			if (rc != BMH_OK) {                                              // the record the host form stopped at, and why
				brq_rec_t r; const brq_tab_t T = U.host_tab();
				index = H.n_seen; code = brq_prep(recs + off[index], off[index + 1] - off[index], U.P, T, r);
			}
		}
		for (size_t k = 0; k < CANARY; ++k) if (all[k] != 0xa5 || all[CANARY + nb + k] != 0xa5) rc = -3;
		fwrite(&rc, 4, 1, o); fwrite(&index, 8, 1, o); fwrite(&code, 4, 1, o);
		if (rc == BMH_OK) { fwrite(U.t.data(), 2, U.t.size(), o); fwrite(recs, 1, nb, o); fwrite(H.R.w.data(), 8, H.R.w.size(), o); }
		delete[] all; delete[] cx; delete[] cy;
	}
	fclose(o); fclose(f);
	return 0;
}
