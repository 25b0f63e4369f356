// csrc/bam_sort_core.h as plain C++ for tests/test_bam_sort.py, built with -fsanitize=address,undefined: every record sits in an allocation of exactly its size.
//   in : u32 n_ref, i32 len[n_ref], u64 n_bytes, the record stream
//   out: u32 n (0xffffffff: the stream is cut), the sorted stream, then per sorted record u64 key, i64 end, u32 lo, u32 hi, u32 head, u64 voff -- the windows of its
//        reference (0, 0 without one), whether it begins a chunk, and its virtual offset in a window whose member m begins at 1000 + 100 m; last the offset behind it
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <numeric>
#include <vector>
#include "../bwa-mem_gpu_amd/csrc/bam_sort_core.h"

int main(int argc, char **argv)
{
	if (argc != 3) return 2;
	FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
	if (!f || !o) return 2;
	uint32_t n_ref; uint64_t nb;
	if (fread(&n_ref, 4, 1, f) != 1) return 2;
	std::vector<int32_t> len(n_ref + 1);
	if (n_ref && fread(len.data(), 4, n_ref, f) != n_ref) return 2;
	if (fread(&nb, 8, 1, f) != 1) return 2;
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
	fwrite(&n, 4, 1, o);
	uint64_t total = 0;
	for (uint32_t i : ord) { fwrite(recs[i].data(), 1, recs[i].size(), o); total += recs[i].size(); }
	std::vector<uint64_t> moff;
	for (uint64_t m = 0; m <= (total + BSR_PIECE - 1) / BSR_PIECE; ++m) moff.push_back(100 * m);
	uint64_t u = 0;
	for (uint32_t j = 0; j < n; ++j) {
		const uint8_t *r = recs[ord[j]].data(), *prev = j ? recs[ord[j - 1]].data() : nullptr;
		const uint64_t key = bsr_key(r), v = bsr_voff(1000, moff.data(), total, u); const int64_t end = bsr_end(r);
		uint32_t lo = 0, hi = 0, head = bsr_chunk_head(r, prev) ? 1 : 0;
		if (bsr_ref(r) >= 0 && (uint32_t)bsr_ref(r) < n_ref) bsr_windows(r, bsr_n_windows(len[bsr_ref(r)]), &lo, &hi);
		fwrite(&key, 8, 1, o); fwrite(&end, 8, 1, o); fwrite(&lo, 4, 1, o); fwrite(&hi, 4, 1, o); fwrite(&head, 4, 1, o); fwrite(&v, 8, 1, o);
		u += recs[ord[j]].size();
	}
	const uint64_t v = bsr_voff(1000, moff.data(), total, u);
	fwrite(&v, 8, 1, o);
	fclose(o); fclose(f);
	return 0;
}
