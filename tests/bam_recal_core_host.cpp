// csrc/bam_recal_core.h, the host form and the mask parser of csrc/bam_recal_host.cpp as plain C++ for tests/test_bam_recal.py, built with
// -fsanitize=address,undefined: every stream, reference, mask and text sits in an allocation of exactly its size.
//   in : u32 n_cases, then per case u32 kind.
//        kind 0 (a table): u32 n_contigs, i32 contig_len [n_contigs], i32 min_qual, i32 max_cycle, u32 window (records; 0: all in one), u32 masked (0 / 1),
//        u32 n_groups, the group IDs (NUL-terminated each), u64 l_pac, the pac body ((l_pac + 3) / 4 bytes), with masked the mask ((l_pac + 63) / 64 words),
//        u64 n_bytes and the record stream
//        kind 1 (a mask): u32 n_contigs, per contig i32 its length and its NUL-terminated name, u32 piece (the text is fed in pieces of that many bytes),
//        the NUL-terminated file name, u64 n_bytes and the text
//   out: kind 0: i32 status (0, or -2: refused), u64 the refused record's index, i32 its code; for status 0 the accumulator's words
//        kind 1: i32 status, the message (256 bytes, NUL-padded), for status 0 the mask's words
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#define BRC_STANDALONE
#include "../bwa-mem_gpu_amd/csrc/bam_recal_host.cpp"

static char g_msg[512];
void bmh_set_error(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_msg, sizeof g_msg, fmt, ap); va_end(ap); }

static bool get(FILE *f, void *p, size_t n) { return !n || fread(p, 1, n, f) == n; }
static bool get_name(FILE *f, std::string &s) { s.clear(); for (int c; (c = fgetc(f)) != EOF;) { if (!c) return true; s.push_back((char)c); } return false; }

int main(int argc, char **argv)
{
	if (argc != 3) return 2;
	FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
	if (!f || !o) return 2;
	uint32_t n_cases;
	if (!get(f, &n_cases, 4)) return 2;
	for (uint32_t c = 0; c < n_cases; ++c) {
		uint32_t kind, nc;
		if (!get(f, &kind, 4) || !get(f, &nc, 4)) return 2;
		if (kind == 1) {
			std::vector<brc_contig_t> contigs; uint64_t at = 0;
			for (uint32_t k = 0; k < nc; ++k) {
				int32_t len; std::string nm;
				if (!get(f, &len, 4) || !get_name(f, nm)) return 2;
				contigs.push_back(brc_contig_t{nm, at, len}); at += (uint64_t)len;
			}
			uint32_t piece; uint64_t nb; std::string file;
			if (!get(f, &piece, 4) || !get_name(f, file) || !get(f, &nb, 8)) return 2;
			char *text = new char[nb ? nb : 1];
			if (!get(f, text, nb)) return 2;
			uint64_t *mask = new uint64_t[(at + 63) / 64 + 1]();
			brc_mask_parser_t M; M.file = file; M.contigs = &contigs; M.mask = mask;
			int32_t rc = BMH_OK;
			g_msg[0] = 0;
			for (uint64_t p = 0; p < nb && rc == BMH_OK; p += piece ? piece : nb) rc = M.feed(text + p, (size_t)(nb - p < (piece ? piece : nb) ? nb - p : (piece ? piece : nb)));
			if (rc == BMH_OK) rc = M.finish();
			char msg[256]; memset(msg, 0, sizeof msg); strncpy(msg, g_msg, sizeof msg - 1);
			fwrite(&rc, 4, 1, o); fwrite(msg, 1, sizeof msg, o);
			if (rc == BMH_OK) fwrite(mask, 8, (at + 63) / 64, o);
			delete[] mask; delete[] text;
			continue;
		}
		std::vector<int32_t> clen(nc ? nc : 1);
		int32_t min_qual, max_cycle; uint32_t window, masked, ng; uint64_t l_pac, nb;
		if (!get(f, clen.data(), 4 * (size_t)nc) || !get(f, &min_qual, 4) || !get(f, &max_cycle, 4) || !get(f, &window, 4) || !get(f, &masked, 4) || !get(f, &ng, 4)) return 2;
		std::vector<std::string> ids(ng); std::vector<const char *> idp;
		for (std::string &s : ids) if (!get_name(f, s)) return 2;
		for (const std::string &s : ids) idp.push_back(s.c_str());
		if (!get(f, &l_pac, 8)) return 2;
		const size_t pb = (size_t)((l_pac + 3) / 4), mw = (size_t)((l_pac + 63) / 64);
		uint8_t *pac = new uint8_t[pb ? pb : 1]; uint64_t *mask = new uint64_t[mw ? mw : 1];
		if (!get(f, pac, pb) || (masked && !get(f, mask, 8 * mw)) || !get(f, &nb, 8)) return 2;
		uint8_t *all = new uint8_t[nb ? nb : 1];
		if (!get(f, all, nb)) return 2;
		std::vector<uint64_t> off(1, 0);
		int32_t rc = BMH_OK, code = 0; uint64_t index = 0;
		for (uint64_t p = 0; p < nb;) {
			const uint64_t sz = bsr_record_bytes(all + p, nb - p);
			if (!sz) { rc = BMH_EINVAL; break; }
			p += sz; off.push_back(p);
		}
		brc_run_t U; brc_host_t H;
		if (rc == BMH_OK) rc = brc_run_make(U, min_qual, max_cycle, pac, l_pac, nullptr, masked ? mask : nullptr, masked ? mw : 0, (int32_t)ng, idp.data(), (int)nc, clen.data(), true, "test");
		if (rc == BMH_OK) {
			H.begin(U);
			const size_t n = off.size() - 1, W = window ? window : (n ? n : 1);
			for (size_t a = 0; a < n && rc == BMH_OK; a += W) rc = H.window(all, off.data() + a, (uint32_t)((a + W < n ? a + W : n) - a), "test");
			if (rc == BMH_OK) H.finish();
			else {                                                       // the record the host form stopped at, and why
				brc_rec_t r; const brc_ref_t F = U.host_ref();
				index = H.n_seen; code = brc_prep(all + off[index], off[index + 1] - off[index], U.P, F, r);
			}
		}
		fwrite(&rc, 4, 1, o); fwrite(&index, 8, 1, o); fwrite(&code, 4, 1, o);
		if (rc == BMH_OK) fwrite(H.R.w.data(), 8, H.R.w.size(), o);
		delete[] all; delete[] mask; delete[] pac;
	}
	fclose(o); fclose(f);
	return 0;
}
