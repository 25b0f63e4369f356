// SAM record lines in device memory -> BAM records (bmh_sam_to_bam_device; the BAM output of csrc/align_pipeline.hip), and the same on host threads.
//
// The lines are found as csrc/reads_parse.hip finds records: every thread counts the '\n' of a 64-byte chunk, a scan places them, a second walk writes
// the line ends.  Then one lane per record, twice, with the per-record logic of csrc/bam_core.h: a sizes pass (status and bytes of every record), an
// exclusive scan, a write pass -- which repeats the record into its slot, bounded by the slot, and flags a record whose bytes differ from the counted
// ones (BAM_ESIZE: the check bmh_sam_text_check makes for the text).  A refused record has no slot and writes nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <cstring>
#include <rocprim/rocprim.hpp>
#include <algorithm>
#include <atomic>
#include <string>
#include <thread>
#include <vector>
#include "bmh_internal.h"
#include "bam_core.h"
#include "bam_ws.h"

namespace {

constexpr uint32_t CH = 64;        // bytes of text per thread of the newline walks

__global__ void __launch_bounds__(256) bam_nl_count(const uint8_t *__restrict__ text, uint64_t n, uint32_t *__restrict__ cnt, uint64_t n_chunks)
{
	const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (c >= n_chunks) return;
	const uint64_t a = c * CH, b = a + CH < n ? a + CH : n;
	uint32_t k = 0;
	for (uint64_t i = a; i < b; ++i) k += text[i] == '\n';
	cnt[c] = k;
}

__global__ void __launch_bounds__(256) bam_nl_fill(const uint8_t *__restrict__ text, uint64_t n, const uint32_t *__restrict__ off, uint64_t *__restrict__ line_end, uint64_t n_chunks, uint32_t n_lines)
{
	const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (c >= n_chunks) return;
	const uint64_t a = c * CH, b = a + CH < n ? a + CH : n;
	uint32_t k = off[c];
	for (uint64_t i = a; i < b; ++i) if (text[i] == '\n') { if (k < n_lines) line_end[k] = i; ++k; }
}

// flags: [0] refused records, [1] the first of them, [2] the write pass met a record of another size
template <bool WRITE>
__global__ void __launch_bounds__(256) bam_records(const uint8_t *__restrict__ text, uint64_t n, const uint64_t *__restrict__ line_end, uint32_t n_lines, uint32_t n_records,
                                                   bam_refs_t R, uint32_t *size, uint32_t *status, const uint64_t *__restrict__ off, uint8_t *bam, uint64_t bam_bytes, uint32_t *flags)
{
	const uint32_t r = blockIdx.x * 256 + threadIdx.x;
	if (r >= n_records) return;
	if (WRITE && status[r] != BAM_OK) return;
	const uint64_t a = r ? line_end[r - 1] + 1 : 0, b = r < n_lines ? line_end[r] : n;
	uint32_t st, sz = 0;
	if (b - a >= (1ull << 31)) st = BAM_ESIZE;
	else if (!WRITE) st = bam_record(text + a, (uint32_t)(b - a), R, nullptr, 0, &sz);
	else {
		const uint32_t cap = size[r];
		st = off[r] > bam_bytes || cap > bam_bytes - off[r] ? (uint32_t)BAM_ESIZE : bam_record(text + a, (uint32_t)(b - a), R, bam + off[r], cap, &sz);
		if (st == BAM_OK && sz != cap) st = BAM_ESIZE;
		if (st != BAM_OK) { status[r] = BAM_ESIZE; atomicOr(flags + 2, 1u); }
		return;
	}
	if (st == BAM_OK && r >= n_lines) st = BAM_ENOEOL;
	status[r] = st; size[r] = st == BAM_OK ? sz : 0;
	if (st != BAM_OK) { atomicAdd(flags, 1u); atomicMin(flags + 1, r); }
}

const char *bam_what(uint32_t s)
{
	static const char *const w[] = {"ok", "fewer than 11 fields", "a read name that is empty or longer than 254 bytes", "a bad CIGAR, or more than 65535 operations",
	                                "a tag that is not XX:T:value with T one of A i f Z H", "SEQ and QUAL of different lengths", "the last line has no newline",
	                                "a contig name that is not in the table", "a number outside its field's range", "an integer tag outside [-2^31, 2^32)",
	                                "a float tag that is not [-+]?digits[.digits] of at most 15 digits", "a B (array) tag", "internal: the write pass disagrees with the sizes pass"};
	return s < sizeof(w) / sizeof(w[0]) ? w[s] : "unknown status";
}

}   // namespace

extern "C" const char *bmh_bam_status_name(uint32_t status) { return bam_what(status); }

extern "C" bmh_bam_ws_t *bmh_bam_ws_create(void) { return new bmh_bam_ws(); }
extern "C" void bmh_bam_ws_free(bmh_bam_ws_t *ws) { delete ws; }

extern "C" int bmh_sam_to_bam_device(bmh_bam_ws_t *ws, const char *d_text, uint64_t n, int n_contigs, const char *d_ctg_names, const uint32_t *d_ctg_name_off, void *stream_, bmh_bam_out_t *out)
{
	const char *fn = "bmh_sam_to_bam_device";
	if (!ws || !out || (n && !d_text) || n_contigs < 0 || (n_contigs && (!d_ctg_names || !d_ctg_name_off))) { bmh_set_error("%s: null argument", fn); return BMH_EINVAL; }
	memset(out, 0, sizeof(*out));
	out->first_refused = 0xffffffffu;
	if (n == 0) return BMH_OK;
	hipStream_t st = (hipStream_t)stream_;
	const uint8_t *text = (const uint8_t *)d_text;
	const uint64_t n_chunks = (n + CH - 1) / CH;
	if (n_chunks >= 0xffffff00ull) { bmh_set_error("%s: %llu bytes of text in one call", fn, (unsigned long long)n); return BMH_EINVAL; }
	RCK(ws->cnt.need(4 * (n_chunks + 1))); RCK(ws->cnt_off.need(4 * (n_chunks + 1))); RCK(ws->flags.need(64));
	size_t tb = scan_tmp_bytes<uint32_t, uint32_t>(n_chunks + 1);
	RCK(ws->tmp.need(tb));
	uint32_t *cnt = (uint32_t *)ws->cnt.p, *cnt_off = (uint32_t *)ws->cnt_off.p, *flags = (uint32_t *)ws->flags.p;
	HIPCK(hipMemsetAsync(cnt + n_chunks, 0, 4, st));
	bam_nl_count<<<(unsigned)((n_chunks + 255) / 256), 256, 0, st>>>(text, n, cnt, n_chunks);
	HIPCK(rocprim::exclusive_scan(ws->tmp.p, tb, cnt, cnt_off, 0u, (size_t)n_chunks + 1, rocprim::plus<uint32_t>(), st));
	uint32_t n_lines = 0; uint8_t last = 0;
	HIPCK(hipMemcpyAsync(&n_lines, cnt_off + n_chunks, 4, hipMemcpyDeviceToHost, st));
	HIPCK(hipMemcpyAsync(&last, text + n - 1, 1, hipMemcpyDeviceToHost, st));
	HIPCK(hipStreamSynchronize(st));
	const uint32_t n_rec = n_lines + (last != '\n' ? 1u : 0u);
	if (n_rec < n_lines) { bmh_set_error("%s: 2^32 lines", fn); return BMH_EINVAL; }
	RCK(ws->line_end.need(8 * ((size_t)n_lines + 1))); RCK(ws->size.need(4 * ((size_t)n_rec + 1))); RCK(ws->status.need(4 * ((size_t)n_rec + 1))); RCK(ws->off.need(8 * ((size_t)n_rec + 2)));
	tb = scan_tmp_bytes<uint32_t, uint64_t>((size_t)n_rec + 1);
	RCK(ws->tmp.need(tb));
	uint64_t *line_end = (uint64_t *)ws->line_end.p, *off = (uint64_t *)ws->off.p; uint32_t *size = (uint32_t *)ws->size.p, *status = (uint32_t *)ws->status.p;
	bam_nl_fill<<<(unsigned)((n_chunks + 255) / 256), 256, 0, st>>>(text, n, cnt_off, line_end, n_chunks, n_lines);
	const uint32_t f0[4] = {0, 0xffffffffu, 0, 0};
	HIPCK(hipMemcpyAsync(flags, f0, 16, hipMemcpyHostToDevice, st));
	HIPCK(hipMemsetAsync(size + n_rec, 0, 4, st));
	bam_refs_t R; R.names = d_ctg_names; R.off = d_ctg_name_off; R.n = n_contigs;
	bam_records<false><<<(n_rec + 255) / 256, 256, 0, st>>>(text, n, line_end, n_lines, n_rec, R, size, status, nullptr, nullptr, 0, flags);
	HIPCK(rocprim::exclusive_scan(ws->tmp.p, tb, size, off, (uint64_t)0, (size_t)n_rec + 1, rocprim::plus<uint64_t>(), st));
	uint64_t total = 0; uint32_t fl[4] = {0, 0, 0, 0};
	HIPCK(hipMemcpyAsync(&total, off + n_rec, 8, hipMemcpyDeviceToHost, st));
	HIPCK(hipMemcpyAsync(fl, flags, 16, hipMemcpyDeviceToHost, st));
	HIPCK(hipStreamSynchronize(st));
	RCK(ws->bam.need((size_t)total + 16));
	bam_records<true><<<(n_rec + 255) / 256, 256, 0, st>>>(text, n, line_end, n_lines, n_rec, R, size, status, off, (uint8_t *)ws->bam.p, total, flags);
	uint32_t bad = 0;
	HIPCK(hipMemcpyAsync(&bad, flags + 2, 4, hipMemcpyDeviceToHost, st));
	HIPCK(hipStreamSynchronize(st));
	HIPCK(hipGetLastError());
	if (bad) { bmh_set_error("%s: internal error: a record's bytes differ from its counted size", fn); return BMH_EINVAL; }
	out->d_bam = (const uint8_t *)ws->bam.p; out->bam_bytes = total; out->d_status = status; out->n_records = n_rec;
	out->n_refused = fl[0]; out->first_refused = fl[1];
	if (fl[0]) HIPCK(hipMemcpy(&out->first_status, status + fl[1], 4, hipMemcpyDeviceToHost));
	return BMH_OK;
}

// the name of record `rec` of the text the work space has just converted (for messages): its first field, at most 254 bytes
std::string bmh_bam_record_name_device(bmh_bam_ws_t *ws, const char *d_text, uint64_t n, uint32_t rec)
{
	uint64_t a = 0;
	if (rec && hipMemcpy(&a, (const uint64_t *)ws->line_end.p + (rec - 1), 8, hipMemcpyDeviceToHost) != hipSuccess) return "?";
	if (rec) ++a;
	char buf[256];
	const size_t k = (size_t)std::min<uint64_t>(255, a < n ? n - a : 0);
	if (k && hipMemcpy(buf, d_text + a, k, hipMemcpyDeviceToHost) != hipSuccess) return "?";
	size_t l = 0;
	while (l < k && buf[l] != '\t' && buf[l] != '\n') ++l;
	return std::string(buf, l);
}

extern "C" int bmh_sam_to_bam_host(const char *text_, uint64_t n, int n_contigs, const char *ctg_names, const uint32_t *ctg_name_off, int n_threads,
                                   uint8_t **bam, uint64_t *bam_bytes, uint32_t **status, uint32_t *n_records)
{
	const char *fn = "bmh_sam_to_bam_host";
	if (!bam || !bam_bytes || !status || !n_records || (n && !text_) || n_contigs < 0 || (n_contigs && (!ctg_names || !ctg_name_off))) { bmh_set_error("%s: null argument", fn); return BMH_EINVAL; }
	*bam = nullptr; *bam_bytes = 0; *status = nullptr; *n_records = 0;
	const uint8_t *text = (const uint8_t *)text_;
	std::vector<uint64_t> line_end;
	for (uint64_t i = 0; i < n; ++i) if (text[i] == '\n') line_end.push_back(i);
	const uint64_t n_lines = line_end.size(), n_rec = n_lines + (n && text[n - 1] != '\n' ? 1 : 0);
	if (n_rec >= 0xffffffffull) { bmh_set_error("%s: 2^32 lines", fn); return BMH_EINVAL; }
	bam_refs_t R; R.names = ctg_names; R.off = ctg_name_off; R.n = n_contigs;
	std::vector<uint32_t> size(n_rec + 1, 0); std::vector<uint64_t> off(n_rec + 1, 0);
	uint32_t *st = (uint32_t *)malloc(4 * (n_rec + 1));
	if (!st) { bmh_set_error("%s: out of memory", fn); return BMH_ENOMEM; }
	const unsigned T = (unsigned)std::max<int64_t>(1, std::min<int64_t>(n_threads > 0 ? n_threads : bmh_effective_cpus(), (int64_t)(n_rec + 4095) / 4096));
	uint8_t *o = nullptr; std::atomic<int> bad{0};
	auto work = [&](unsigned t, bool write) {
		for (uint64_t r = n_rec * t / T; r < n_rec * (t + 1) / T; ++r) {
			if (write && st[r] != BAM_OK) continue;
			const uint64_t a = r ? line_end[r - 1] + 1 : 0, b = r < n_lines ? line_end[r] : n;
			uint32_t s, sz = 0;
			if (b - a >= (1ull << 31)) s = BAM_ESIZE;
			else s = bam_record(text + a, (uint32_t)(b - a), R, write ? o + off[r] : nullptr, write ? size[r] : 0, &sz);
			if (write) { if (s != BAM_OK || sz != size[r]) { st[r] = BAM_ESIZE; bad = 1; } continue; }
			if (s == BAM_OK && r >= n_lines) s = BAM_ENOEOL;
			st[r] = s; size[r] = s == BAM_OK ? sz : 0;
		}
	};
	auto run = [&](bool write) {
		if (T == 1) work(0, write);
		else { std::vector<std::thread> th; for (unsigned t = 0; t < T; ++t) th.emplace_back(work, t, write); for (auto &x : th) x.join(); }
	};
	run(false);
	for (uint64_t r = 0; r < n_rec; ++r) off[r + 1] = off[r] + size[r];
	o = (uint8_t *)malloc(off[n_rec] + 1);
	if (!o) { free(st); bmh_set_error("%s: out of memory", fn); return BMH_ENOMEM; }
	run(true);
	if (bad.load()) { free(st); free(o); bmh_set_error("%s: internal error: a record's bytes differ from its counted size", fn); return BMH_EINVAL; }
	*bam = o; *bam_bytes = off[n_rec]; *status = st; *n_records = (uint32_t)n_rec;
	return BMH_OK;
}

extern "C" int bmh_bam_header(const char *header_text, int n_contigs, const char *const *contig_names, const int32_t *contig_len, uint8_t **out, uint64_t *out_bytes)
{
	if (!header_text || !out || !out_bytes || n_contigs < 0 || (n_contigs && (!contig_names || !contig_len))) { bmh_set_error("bmh_bam_header: null argument"); return BMH_EINVAL; }
	std::string h;
	auto u32 = [&](uint32_t v) { for (int k = 0; k < 4; ++k) h.push_back((char)(v >> (8 * k))); };
	const size_t lt = strlen(header_text);
	if (lt > 0x7fffffffu) { bmh_set_error("bmh_bam_header: a header text of 2^31 bytes or more"); return BMH_EINVAL; }
	h += "BAM\1"; u32((uint32_t)lt); h.append(header_text, lt); u32((uint32_t)n_contigs);
	for (int c = 0; c < n_contigs; ++c) { const size_t l = strlen(contig_names[c]) + 1; u32((uint32_t)l); h.append(contig_names[c], l); u32((uint32_t)contig_len[c]); }
	uint8_t *o = (uint8_t *)malloc(h.size() + 1);
	if (!o) { bmh_set_error("bmh_bam_header: out of memory"); return BMH_ENOMEM; }
	memcpy(o, h.data(), h.size());
	*out = o; *out_bytes = h.size();
	return BMH_OK;
}
