// The CSI rules of csrc/bam_sort_core.h as plain C++ for tests/test_bam_csi.py, built with -fsanitize=address,undefined: every record sits in an allocation of exactly
// its size.
//   in : u32 n_ref, i32 len[n_ref], i32 min_shift, u64 n_bytes, the record stream
//   out: u32 n (0xffffffff: the stream is cut), i32 depth (of the longest contig), u32 pseudo-bin, u32 first bin of every level 0 .. depth, then per record in sorted
//        order u32 lo, u32 hi (its windows of 2^min_shift bases on its reference; 0, 0 without one), u32 bin, u32 head (does it begin a chunk on (refID, CSI bin))
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <numeric>
#include <vector>
#include "../bwa-mem_gpu_amd/csrc/bam_sort_core.h"

int main(int argc, char **argv)
{
	if (argc != 3) return 2;
	FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
	if (!f || !o) return 2;
	uint32_t n_ref; int32_t shift; uint64_t nb;
	if (fread(&n_ref, 4, 1, f) != 1) return 2;
	std::vector<int32_t> len(n_ref + 1);
	if (n_ref && fread(len.data(), 4, n_ref, f) != n_ref) return 2;
	if (fread(&shift, 4, 1, f) != 1 || fread(&nb, 8, 1, f) != 1) return 2;
	std::vector<uint8_t> all(nb);
	if (nb && fread(all.data(), 1, nb, f) != nb) return 2;
	std::vector<std::vector<uint8_t>> recs;
	for (uint64_t p = 0; p < nb;) {
		const uint64_t sz = bsr_record_bytes(all.data() + p, nb - p);
		if (!sz) { const uint32_t bad = 0xffffffffu; fwrite(&bad, 4, 1, o); fclose(o); return 0; }
		recs.emplace_back(all.begin() + p, all.begin() + p + sz); p += sz;
	}
	const uint32_t n = (uint32_t)recs.size();
	std::vector<uint32_t> ord(n); std::iota(ord.begin(), ord.end(), 0u);
	std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return bsr_key(recs[a].data()) < bsr_key(recs[b].data()); });
	int64_t longest = 0;
	for (uint32_t c = 0; c < n_ref; ++c) longest = std::max<int64_t>(longest, len[c]);
	const int32_t depth = bsr_csi_depth(longest, shift);
	const uint32_t meta = bsr_csi_meta_bin(depth);
	fwrite(&n, 4, 1, o); fwrite(&depth, 4, 1, o); fwrite(&meta, 4, 1, o);
	for (int l = 0; l <= depth; ++l) { const uint32_t b = bsr_csi_level_first(depth, l); fwrite(&b, 4, 1, o); }
	for (uint32_t j = 0; j < n; ++j) {
		const uint8_t *r = recs[ord[j]].data(), *prev = j ? recs[ord[j - 1]].data() : nullptr;
		const bool has = bsr_ref(r) >= 0 && (uint32_t)bsr_ref(r) < n_ref;
		const uint32_t nw = has ? bsr_n_windows_at(len[bsr_ref(r)], shift) : 1u;
		uint32_t lo = 0, hi = 0;
		if (has) bsr_windows_at(r, nw, shift, &lo, &hi);
		const uint32_t bin = bsr_csi_rec_bin(r, nw, shift, depth), head = bsr_csi_chunk_head(r, prev, nw, shift, depth) ? 1 : 0;
		if (has && bin != bsr_csi_bin(lo, hi, depth)) return 3;
		fwrite(&lo, 4, 1, o); fwrite(&hi, 4, 1, o); fwrite(&bin, 4, 1, o); fwrite(&head, 4, 1, o);
	}
	fclose(o); fclose(f);
	return 0;
}
