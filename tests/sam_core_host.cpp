// csrc/sam_core.h as plain C++ (no HIP header) over a trivial array-backed Src: the counting sink, then the pointer sink into a buffer of EXACTLY the
// counted size per read -- under -fsanitize=address a byte past the count is a heap overflow.  usage: sam_core_host <table file>; the text goes to stdout.
// The table file (tests/sam_table.py: write_table) is a row of sections, each an int64 byte count and the bytes padded to 8.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../bwa-mem_gpu_amd/csrc/sam_core.h"

namespace {

struct tab_src {
	const int32_t *opt; double drop_; const char *rg_; int rg_n;      // opt: flag_all softclip sa max_XA_hits max_XA_hits_alt paired copy_comment n_contigs
	const uint32_t *fpr; const int32_t *fin; const int32_t *slot; const int32_t *alns; const uint32_t *cig_off, *packed;
	const char *names; const uint64_t *name_off; const uint8_t *bases; const uint64_t *read_off; const uint32_t *read_len; const uint8_t *quals;
	const char *comments; const uint64_t *comment_off; const char *ctg_names; const uint32_t *ctg_name_off; const int64_t *ctg_offs;
	const int32_t *h_recs, *unflags;
	std::vector<uint64_t> rec_off;
	struct read_t {
		const tab_src &S; uint64_t base; int n; const int32_t *fin;
		sam_core::aln_t aln(int i) const
		{
			sam_core::aln_t x = {nullptr, nullptr, nullptr};
			const int32_t s = S.slot[base + i];
			if (s >= 0) { x.aln = S.alns + 8 * s; x.cigar = S.packed + S.cig_off[s]; x.md = (const char *)(x.cigar + x.aln[3]); }
			return x;
		}
	};
	read_t read(uint32_t r) const { return read_t{*this, rec_off[r], (int)fpr[r], fin + 16 * rec_off[r]}; }
	bool flag_all() const { return opt[0]; }
	bool softclip() const { return opt[1]; }
	int sa() const { return opt[2]; }
	double drop() const { return drop_; }
	int max_XA_hits() const { return opt[3]; }
	int max_XA_hits_alt() const { return opt[4]; }
	const char *rg() const { return rg_; }
	int rg_len() const { return rg_n; }
	bool paired() const { return opt[5]; }
	int h_rec(uint32_t r) const { return h_recs[r]; }
	int unflag(uint32_t r) const { return opt[5] ? unflags[r] : 0; }
	int md_len(const sam_core::aln_t &x) const { return x.aln[6]; }
	const char *name(uint32_t r) const { return names + name_off[r]; }
	int name_len(uint32_t r) const { return (int)(name_off[r + 1] - name_off[r]) - 1; }
	int l_seq(uint32_t r) const { return (int)read_len[r]; }
	const uint8_t *seq(uint32_t r) const { return bases + read_off[r]; }
	const uint8_t *qual(uint32_t r) const { return quals ? quals + read_off[r] : nullptr; }
	const char *comment(uint32_t r, int &len) const { if (!opt[6]) return nullptr; len = (int)(comment_off[r + 1] - comment_off[r]) - 1; return comments + comment_off[r]; }
	char letter(uint8_t c, bool rev) const { for (int k = 0; k < 4; ++k) if ((c & 0xDF) == "ACGT"[k]) return (rev ? "TGCA" : "ACGT")[k]; return 'N'; }
	int n_contigs() const { return opt[7]; }
	long long ctg_off(int i) const { return ctg_offs[i]; }
	long long ctg0(int rid) const { return opt[7] > 1 ? ctg_offs[rid] : 0; }
	const char *ctg(int rid) const { return ctg_names + ctg_name_off[rid]; }
	int ctg_len(int rid) const { return (int)(ctg_name_off[rid + 1] - ctg_name_off[rid]) - 1; }
};

}

int main(int argc, char **argv)
{
	if (argc != 2) { fprintf(stderr, "usage: sam_core_host <table>\n"); return 2; }
	FILE *f = fopen(argv[1], "rb");
	if (!f) { perror(argv[1]); return 2; }
	std::vector<std::vector<uint64_t>> sec;                   // (8-byte units: every section is aligned for its type)
	std::vector<size_t> bytes;
	for (int64_t nb; fread(&nb, 8, 1, f) == 1;) {
		sec.emplace_back((size_t)(nb + 7) / 8 + 1, 0);
		if (fread(sec.back().data(), 8, (size_t)(nb + 7) / 8, f) != (size_t)(nb + 7) / 8) { fprintf(stderr, "short table\n"); return 2; }
		bytes.push_back((size_t)nb);
	}
	fclose(f);
	if (sec.size() != 22) { fprintf(stderr, "22 sections expected, %zu found\n", sec.size()); return 2; }
	auto at = [&](int i) { return (const void *)sec[i].data(); };
	tab_src S;
	S.opt = (const int32_t *)at(0); S.drop_ = *(const double *)at(1); S.rg_ = (const char *)at(2); S.rg_n = (int)bytes[2];
	S.fpr = (const uint32_t *)at(3); S.fin = (const int32_t *)at(4); S.slot = (const int32_t *)at(5); S.alns = (const int32_t *)at(6);
	S.cig_off = (const uint32_t *)at(7); S.packed = (const uint32_t *)at(8); S.names = (const char *)at(9); S.name_off = (const uint64_t *)at(10);
	S.bases = (const uint8_t *)at(11); S.read_off = (const uint64_t *)at(12); S.read_len = (const uint32_t *)at(13); S.quals = bytes[14] ? (const uint8_t *)at(14) : nullptr;
	S.comments = (const char *)at(15); S.comment_off = (const uint64_t *)at(16); S.ctg_names = (const char *)at(17); S.ctg_name_off = (const uint32_t *)at(18);
	S.ctg_offs = (const int64_t *)at(19); S.h_recs = (const int32_t *)at(20); S.unflags = (const int32_t *)at(21);
	const uint32_t n = (uint32_t)(bytes[3] / 4);
	S.rec_off.assign((size_t)n + 1, 0);
	for (uint32_t r = 0; r < n; ++r) S.rec_off[r + 1] = S.rec_off[r] + S.fpr[r];
	for (uint32_t r = 0; r < n; ++r) {
		sam_core::count_out c;
		if (sam_core::read_records(S, r, c) >= 0) { fprintf(stderr, "read %u: a record has no alignment (counting)\n", r); return 3; }
		char *buf = (char *)malloc(c.n ? c.n : 1);
		sam_core::ptr_out<char *> w{buf};
		if (sam_core::read_records(S, r, w) >= 0) { fprintf(stderr, "read %u: a record has no alignment (writing)\n", r); return 3; }
		if ((size_t)(w.p - buf) != c.n) { fprintf(stderr, "read %u: %u bytes counted, %zu written\n", r, c.n, (size_t)(w.p - buf)); return 4; }
		fwrite(buf, 1, c.n, stdout);
		free(buf);
	}
	return 0;
}
