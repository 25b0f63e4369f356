// csrc/bam_collate_core.h as plain C++ under AddressSanitizer and UBSan (tests/test_bam_collate.py builds and runs this): the definition of --collate walked over
// windows of a few records, each window a heap block of exactly its records' bytes, so that a read outside a window -- or of a pool record that has been freed --
// is reported.  A window that completes no pair is doubled, as the pump doubles its windows; a window that does is consumed up to the record that completes its
// last pair, and the open records inside that prefix live on in the pool alone.
//   in : u64 cap, u32 records per window, u32 n, then n x (u32 size, bytes)
//   out: text -- "pair <index of the 0x40 record> <index of the 0x80 record>" in the order of completion, then one of "same_role <i> <j>", "over_cap <i>",
//        "open <i>" when the input is refused, then "counts <pairs> <pairs_adjacent> <open_records_peak> <open_bytes_peak>"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../bwa-mem_gpu_amd/csrc/bam_collate_core.h"

int main(int argc, char **argv)
{
	if (argc != 3) { fprintf(stderr, "usage: %s case.bin result.txt\n", argv[0]); return 2; }
	FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "w");
	if (!fi || !fo) { fprintf(stderr, "cannot open the files\n"); return 2; }
	uint64_t cap = 0; uint32_t per = 0, n = 0;
	if (fread(&cap, 8, 1, fi) != 1 || fread(&per, 4, 1, fi) != 1 || fread(&n, 4, 1, fi) != 1 || per == 0) return 2;
	std::vector<std::vector<uint8_t>> recs(n);
	for (uint32_t c = 0; c < n; ++c) {
		uint32_t size = 0;
		if (fread(&size, 4, 1, fi) != 1) return 2;
		recs[c].resize(size);
		if (size && fread(recs[c].data(), 1, size, fi) != size) return 2;
	}
	bcl_pool_t P;
	P.cap = cap;
	size_t first = 0, want = per;
	bool refused = false;
	while (first < n && !refused) {
		const size_t cnt = std::min<size_t>(want, n - first);
		const bool eof = first + cnt == n;
		size_t bytes = 0;
		for (size_t k = 0; k < cnt; ++k) bytes += recs[first + k].size();
		uint8_t *buf = (uint8_t *)malloc(bytes ? bytes : 1);
		std::vector<uint32_t> starts(1, 0u);
		for (size_t k = 0; k < cnt; ++k) { memcpy(buf + starts.back(), recs[first + k].data(), recs[first + k].size()); starts.push_back(starts.back() + (uint32_t)recs[first + k].size()); }
		bcl_walk_t W(P, buf, starts.data(), first);
		std::vector<uint64_t> out;
		for (size_t k = 0; k < cnt && !refused; ++k) {
			bi_rec_t B;
			if (bi_check(buf + starts[k], starts[k + 1] - starts[k], &B) != BI_OK) { fprintf(stderr, "record %zu is damaged\n", first + k); return 3; }
			const uint32_t role = bi_role(B.flag);
			if (role == 0) continue;
			if (role == 3) { fprintf(stderr, "record %zu has no role\n", first + k); return 3; }
			bcl_partner_t pt;
			const int ev = W.step((uint32_t)k, role, &pt);
			if (ev == BCL_OPENED) continue;
			if (ev == BCL_PAIR) {
				// the partner's bytes are read (a freed pool record would be reported): its name equals this record's
				if (strcmp((const char *)pt.bytes + BI_NAME_OFF, (const char *)buf + starts[k] + BI_NAME_OFF) != 0) { fprintf(stderr, "record %zu was paired with another name\n", first + k); return 3; }
				out.push_back(role == 2 ? pt.index : first + k); out.push_back(role == 2 ? first + k : pt.index);
				W.commit((uint32_t)k);
				continue;
			}
			for (size_t q = 0; q < out.size(); q += 2) fprintf(fo, "pair %llu %llu\n", (unsigned long long)out[q], (unsigned long long)out[q + 1]);
			out.clear();
			if (ev == BCL_SAME_ROLE) fprintf(fo, "same_role %llu %zu\n", (unsigned long long)pt.index, first + k);
			else fprintf(fo, "over_cap %llu\n", (unsigned long long)pt.index);
			refused = true;
		}
		if (!refused) {
			if (W.committed) {
				for (size_t q = 0; q < out.size(); q += 2) fprintf(fo, "pair %llu %llu\n", (unsigned long long)out[q], (unsigned long long)out[q + 1]);
				W.deliver();
				first += (size_t)W.c_rec + 1;
				want = per;
			} else if (eof) {
				const int64_t s = P.smallest(), fo_ = W.first_open();
				if (s >= 0) { fprintf(fo, "open %llu\n", (unsigned long long)P.slots[(size_t)s].index); refused = true; }
				else if (fo_ >= 0) { fprintf(fo, "open %llu\n", (unsigned long long)(first + (size_t)fo_)); refused = true; }
				first = n;
			} else want *= 2;
		}
		free(buf);
	}
	if (!refused && P.n) { fprintf(fo, "open %llu\n", (unsigned long long)P.slots[(size_t)P.smallest()].index); }
	fprintf(fo, "counts %llu %llu %llu %llu\n", (unsigned long long)P.cnt.pairs, (unsigned long long)P.cnt.pairs_adjacent, (unsigned long long)P.cnt.open_records_peak, (unsigned long long)P.cnt.open_bytes_peak);
	fclose(fi); fclose(fo);
	return 0;
}
