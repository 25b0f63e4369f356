// csrc/bam_tpl_core.h as plain C++ for tests/test_bam_post_collate.py, built with -fsanitize=address,undefined: every stream sits in an allocation of exactly its
// size, so a read past a record's end is a finding.  The grouping is the host form's (a stable sort by the key, the fold of every set); every folded set is also
// laid out as adjacent records and given to bdp_entry, and -- in a second pass under a table of read groups and the barcode tag RX -- to bdp_entry_lib,
// bdp_location and bdp_barcode: the fold must say what they say.
//   in : u32 n_cases, per case u32 hash_bits, u64 n_bytes and the record stream (whole records)
//   out: per case u32 n records, u64 the refusal word (all ones: none); without a refusal u32 n_templates, u32 tpl [n], the entries (24 bytes each)
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <numeric>
#include <vector>
#include "../bwa-mem_gpu_amd/csrc/bam_tpl_core.h"

static int fail(const char *what, uint32_t c, uint32_t i) { fprintf(stderr, "bam_tpl_core_host: case %u, set of record %u: %s\n", c, i, what); return 3; }

int main(int argc, char **argv)
{
	if (argc != 3) return 2;
	FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
	if (!f || !o) return 2;
	uint32_t n_cases;
	if (fread(&n_cases, 4, 1, f) != 1) return 2;
	const char ids[] = "abc"; const uint32_t id_off[4] = {0, 1, 2, 3}; const uint8_t lib[3] = {0, 1, 0};
	const bdp_groups_t G = {ids, id_off, lib, 3};
	const bdp_bc_t bc = {BDP_BC_TAG, 'R', 'X', 0};
	for (uint32_t c = 0; c < n_cases; ++c) {
		uint32_t bits; uint64_t nb;
		if (fread(&bits, 4, 1, f) != 1 || fread(&nb, 8, 1, f) != 1) return 2;
		uint8_t *all = new uint8_t[nb ? nb : 1];
		if (nb && fread(all, 1, nb, f) != nb) return 2;
		std::vector<uint64_t> off(1, 0);
		for (uint64_t p = 0; p < nb;) {
			const uint64_t sz = bsr_record_bytes(all + p, nb - p);
			if (!sz || bpo_check(all + p, sz, 0x7fffffff, BPO_MARKDUP) != BPO_OK) return fail("a record of the case is not whole", c, (uint32_t)off.size() - 1);
			p += sz; off.push_back(p);
		}
		const uint32_t n = (uint32_t)(off.size() - 1);
		for (int pass = 0; pass < 2; ++pass) {                          // 0: plain, written out; 1: read groups, barcodes and locations, compared only
			const bool opt = pass == 1;
			std::vector<btp_part_t> P(n); std::vector<uint64_t> W(n, 0); std::vector<bdp_loc_t> L(n);
			for (uint32_t i = 0; i < n; ++i) P[i] = btp_part(all + off[i], off[i + 1] - off[i], opt ? &G : nullptr, opt ? &bc : nullptr, &W[i], &L[i], bits);
			std::vector<uint32_t> idx(n), ord(n, 0), tpl(n, 0);
			std::iota(idx.begin(), idx.end(), 0u);
			std::stable_sort(idx.begin(), idx.end(), [&P](uint32_t a, uint32_t b) { return P[a].h1 != P[b].h1 ? P[a].h1 < P[b].h1 : P[a].h0 < P[b].h0; });
			for (uint32_t j = 0; j < n; ++j) if (j == 0 || !btp_key_equal(P[idx[j]], P[idx[j - 1]])) ord[idx[j]] = 1;
			uint32_t T = 0;
			for (uint32_t i = 0; i < n; ++i) { const uint32_t h = ord[i]; ord[i] = T; T += h; }
			std::vector<bdp_entry_t> E(T);
			uint64_t word = BPO_NONE;
			for (uint32_t j = 0; j < n;) {
				uint32_t k = j + 1;
				while (k < n && btp_key_equal(P[idx[k]], P[idx[j]])) ++k;
				for (uint32_t q = j + 1; q < k; ++q) if (idx[q] <= idx[q - 1]) return fail("the members are not in file order", c, idx[j]);
				const uint32_t fi = idx[j], t = ord[fi]; uint32_t role = 0; btp_lines_t ln;
				const int st = btp_fold(P.data(), idx.data() + j, k - j, opt, opt, &E[t], &role, &ln);
				if (st != BDP_E_OK) word = std::min(word, bpo_refusal(fi, st));
				for (uint32_t q = j; q < k; ++q) tpl[idx[q]] = t;
				// the same records next to each other, as bdp_entry takes them
				std::vector<uint8_t> run; std::vector<uint64_t> roff(1, 0);
				for (uint32_t q = j; q < k; ++q) { run.insert(run.end(), all + off[idx[q]], all + off[idx[q] + 1]); roff.push_back(run.size()); }
				bdp_entry_t e; uint32_t role2 = 0, row = 0;
				if (!opt) {
					const bool ok = bdp_entry(run.data(), roff.data(), 0, k - j, &e, &role2);
					if (ok != (st == BDP_E_OK)) return fail("the fold's verdict is not bdp_entry's", c, fi);
					if (ok && (memcmp(&e, &E[t], sizeof e) || role != role2)) return fail("the fold's entry is not bdp_entry's", c, fi);
				} else if (st == BDP_E_OK) {
					if (bdp_entry_lib(run.data(), roff.data(), 0, k - j, G, &e, &role2, &row) != BDP_E_OK || memcmp(&e, &E[t], sizeof e)) return fail("the fold's entry is not bdp_entry_lib's", c, fi);
					const bdp_loc_t a = btp_location(L[fi], role, P[fi], true), b = bdp_location(run.data(), role2, row, false);
					if (a.x != b.x || a.y != b.y || a.tile != b.tile || a.rg != b.rg || a.flags != b.flags) return fail("the fold's location is not bdp_location's", c, fi);
					uint64_t w = 0;
					if (bdp_barcode(run.data(), roff[1], bc, &w, false) != BDP_AUX_FOUND || w != W[fi]) return fail("the fold's barcode word is not bdp_barcode's", c, fi);
				}
				j = k;
			}
			if (opt) continue;
			fwrite(&n, 4, 1, o); fwrite(&word, 8, 1, o);
			if (word != BPO_NONE) continue;
			fwrite(&T, 4, 1, o);
			if (n) fwrite(tpl.data(), 4, n, o);
			if (T) fwrite(E.data(), sizeof(bdp_entry_t), T, o);
		}
		delete[] all;
	}
	fclose(o); fclose(f);
	return 0;
}
