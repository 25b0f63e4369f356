// Read files cut into records on the device (bmh_reads_load_files, bmh_aligner_run_files): multi-line FASTA, four-line FASTQ, one file or an R1 / R2 pair.
//
// A window of each file's text (csrc/reads_src.cpp delivers it, inflated if need be, into pinned memory) goes to HBM and comes back as the arrays of a
// bmh_read_set_t batch, laid out as bmh_fasta_fill lays them out.  The window starts at a record; per window and file (offsets are 32-bit):
//   1 per byte   "byte i-1 is '\n'" scanned to line ids, line starts scattered to L[]                                     (rocPRIM scan, rp_line_starts)
//   2 per line   kind from the first byte (> @ + other, empty, a lone CR), length without the line end and a trailing CR    (rp_line_kind)
//   3 per line   records: FASTA = scan of the '>' lines, every other non-empty line is sequence (a multi-line record is joined by the scan of the kept
//                lengths: its length is a difference of that scan); FASTQ = the non-empty lines counted, four to a record, '@' / seq / '+' / qual  (rp_line_role)
//   4 per record length, name (to the first isspace byte, "/<digit>" trimmed) and comment spans, where the record ends; with two files record i of
//                file f is read 2i+f                                                                                     (rp_records)
//   5 per read   exclusive scans of the lengths -> offs, name_offs, comment_offs                                           (rocPRIM)
//   6 per byte   kept bytes -> letters, nt4 codes, qualities; per read its name and comment                                (rp_scatter, rp_names)
// The device takes the regular grammar and validates it.  Whatever it cannot decide from a line and its neighbours raises the window's flag (a plain store
// to a status word): a FASTQ record that is not four lines, a '+' / '@' where a FASTA sequence line belongs, text before the first header, a lone CR where
// kseq would keep it as a base, an empty sequence, qualities of another length, a last line without its '\n' that is a header or ends in CR.  A flagged
// window is walked by the host (csrc/reads_io.cpp: bmh_walk_record), which parses it or refuses it with a message.
// Records that are not complete in the window (a FASTA record is complete when the next header is there, or the file ends) stay in the text: the pump moves
// the text behind the last record taken to the front of the buffer and reads on.  A batch always comes from ONE parse: if the window does not reach the
// wanted bases, more text is read and the window is parsed again (the window is sized from the batch before it, so this is rare).
// A BGZF file that holds a BAM is the pump's third kind (bam_open, bam_fill, bam_next below): its windows hold records instead of text, the host walks their chain
// of starts and csrc/bam_in_kernels.hip decodes them; the carry rule, the batch cut and the growth of the window are the ones above.
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <mutex>
#include <string>
#include <vector>
#define BMH_CK_PREFIX "reads parser: "
#include "bmh_internal.h"
#include "devmem.h"

namespace {

enum { LK_BLANK = 0, LK_SEQ = 1, LK_GT = 2, LK_AT = 3, LK_PLUS = 4, LK_LCR = 5 };
enum { RL_HDR = 0, RL_SEQ = 1, RL_PLUS = 2, RL_QUAL = 3, RL_NONE = 4 };

struct rp_ctl_t { uint32_t flag, n_flag_lines, seq_total, pad; };

struct rp_ls_flag {
	const uint8_t *b;
	__host__ __device__ uint32_t operator()(uint32_t i) const { return (i == 0 || b[i - 1] == '\n') ? 1u : 0u; }
};
struct rp_to64 { __host__ __device__ uint64_t operator()(uint32_t v) const { return v; } };

// nst_nt4_table (src/bntseq.c): A/a 0, C/c 1, G/g 2, T/t 3, everything else 4
__device__ __forceinline__ uint8_t rp_nt4(uint8_t c)
{
	switch (c) {
	case 'A': case 'a': return 0;
	case 'C': case 'c': return 1;
	case 'G': case 'g': return 2;
	case 'T': case 't': return 3;
	default: return 4;
	}
}
__device__ __forceinline__ bool rp_isspace(uint8_t c) { return c == ' ' || (c >= '\t' && c <= '\r'); }

__global__ void __launch_bounds__(256) rp_line_starts(const uint8_t *__restrict__ b, uint32_t n, const uint32_t *__restrict__ lid, uint32_t *__restrict__ L)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	if (i == 0 || b[i - 1] == '\n') L[lid[i] - 1] = i;
}

// kind, kept length and the flag that is scanned (FASTA: a '>' line; FASTQ: a complete non-empty line)
__global__ void __launch_bounds__(256) rp_line_kind(const uint8_t *__restrict__ b, uint32_t n, uint32_t m, int eof, int fq, const uint32_t *__restrict__ L,
                                                    uint8_t *__restrict__ kind, uint32_t *__restrict__ klen, uint32_t *__restrict__ flag, rp_ctl_t *ctl)
{
	const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= m) return;
	const uint32_t s = L[j], e = j + 1 < m ? L[j + 1] : n;
	const bool nl = b[e - 1] == '\n';
	const uint32_t c = e - s - (nl ? 1u : 0u);
	uint32_t k = c; int kd;
	if (c == 0) kd = LK_BLANK;
	else if (c == 1 && b[s] == '\r') { kd = LK_LCR; k = 0; }
	else {
		const uint8_t f = b[s];
		kd = f == '>' ? LK_GT : f == '@' ? LK_AT : f == '+' ? LK_PLUS : LK_SEQ;
		if (b[s + c - 1] == '\r') k = c - 1;
	}
	bool bad = false;
	if (j == m - 1 && eof && !nl && (b[e - 1] == '\r' || (!fq && kd == LK_GT))) bad = true;      // the file's last line, unfinished: kseq's end-of-file rules (host)
	uint32_t fl;
	if (!fq) {
		fl = kd == LK_GT;
		if (kd == LK_AT || kd == LK_PLUS) bad = true;
		if (kd == LK_LCR) {                                    // dropped by kseq only behind sequence bytes of the same record
			bool ok = nl && j > 0;
			if (ok) {
				const uint32_t ps = L[j - 1], pc = s - ps - 1;
				const uint8_t pf = b[ps];
				ok = pc >= 1 && !(pc == 1 && pf == '\r') && pf != '>' && pf != '@' && pf != '+';
			}
			if (!ok) bad = true;
		}
	} else fl = (nl || eof) && kd != LK_BLANK && kd != LK_LCR;
	kind[j] = (uint8_t)kd; klen[j] = k; flag[j] = fl;
	if (bad) ctl->flag = 1;
}

// the record and the role of every line; fs: exclusive scan of flag
__global__ void __launch_bounds__(256) rp_line_role(uint32_t m, int fq, const uint8_t *__restrict__ kind, const uint32_t *__restrict__ klen, const uint32_t *__restrict__ flag,
                                                    const uint32_t *__restrict__ fs, uint8_t *__restrict__ role, uint32_t *__restrict__ rec, uint32_t *__restrict__ seqk,
                                                    uint32_t *__restrict__ hdr_line, uint32_t *__restrict__ seq_line, uint32_t *__restrict__ qual_line, rp_ctl_t *ctl)
{
	const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= m) return;
	const uint32_t total = fs[m - 1] + flag[m - 1];
	const int kd = kind[j];
	int ro = RL_NONE; uint32_t r = 0; bool bad = false;
	if (!fq) {
		const uint32_t cnt = fs[j] + flag[j];
		if (cnt == 0) { if (kd != LK_BLANK) bad = true; }        // text before the first header
		else {
			r = cnt - 1;
			if (kd == LK_GT) { ro = RL_HDR; hdr_line[r] = j; }
			else if (kd == LK_SEQ) ro = RL_SEQ;
		}
	} else {
		const uint32_t nq = total / 4, ord = fs[j];
		if (flag[j]) {
			r = ord >> 2;
			if (r < nq) {
				ro = (int)(ord & 3u);
				if (ro == RL_HDR) { if (kd != LK_AT) bad = true; hdr_line[r] = j; }
				else if (ro == RL_SEQ) { if (kd != LK_SEQ) bad = true; seq_line[r] = j; }
				else if (ro == RL_PLUS) { if (kd != LK_PLUS) bad = true; }
				else qual_line[r] = j;
			}
		} else if (kd == LK_LCR && (ord & 3u) != 0) bad = true;  // a lone CR inside a record: kseq may keep it
	}
	role[j] = (uint8_t)ro; rec[j] = r; seqk[j] = ro == RL_SEQ ? klen[j] : 0u;
	if (j == m - 1) { ctl->n_flag_lines = total; }
	if (bad) ctl->flag = 1;
}

struct rp_file_t {      // one file's window on the device
	const uint8_t *b; uint32_t n, m; int eof, fq;
	const uint32_t *L, *klen, *flag, *fs, *seqk, *sloff, *hdr_line, *seq_line, *qual_line, *lid, *rec; const uint8_t *role;
	uint32_t *rend, *rsl;
};

// record r of file f -> read nf * r + f: its length, name and comment spans, where it ends in the text
__global__ void __launch_bounds__(256) rp_records(rp_file_t F, int f, int nf, uint32_t nuse, int comments, uint32_t *__restrict__ lens, uint32_t *__restrict__ nlen,
                                                  uint32_t *__restrict__ clen, uint32_t *__restrict__ nstart, uint32_t *__restrict__ cstart, rp_ctl_t *ctl)
{
	const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
	if (r >= nuse) return;
	const uint8_t *b = F.b;
	const uint32_t m = F.m, n = F.n;
	const uint32_t h = F.hdr_line[r], s = F.L[h];
	uint32_t e = h + 1 < m ? F.L[h + 1] : n;
	if (b[e - 1] == '\n') --e;
	uint32_t len, rsl, rend; bool bad = false;
	if (!F.fq) {
		const uint32_t nh = F.fs[m - 1] + F.flag[m - 1], tot = F.sloff[m - 1] + F.seqk[m - 1];
		rsl = F.sloff[h];
		if (r + 1 < nh) { const uint32_t h2 = F.hdr_line[r + 1]; len = F.sloff[h2] - rsl; rend = F.L[h2]; }
		else { len = tot - rsl; rend = n; }
	} else {
		const uint32_t sl = F.seq_line[r], ql = F.qual_line[r];
		len = F.klen[sl]; rsl = F.sloff[sl];
		if (F.klen[ql] != len) bad = true;
		rend = ql + 1 < m ? F.L[ql + 1] : n;
	}
	if (len == 0) bad = true;
	uint32_t q = s + 1;
	while (q < e && !rp_isspace(b[q])) ++q;
	uint32_t nl_ = q - (s + 1);
	if (nl_ > 2 && b[s + nl_ - 1] == '/' && b[s + nl_] >= '0' && b[s + nl_] <= '9') nl_ -= 2;
	uint32_t cl = 0;
	if (q < e) { cl = e - (q + 1); if (cl > 1 && b[e - 1] == '\r') --cl; }
	const uint32_t idx = (uint32_t)nf * r + (uint32_t)f;
	lens[idx] = len; nlen[idx] = nl_ + 1; clen[idx] = comments ? cl + 1 : 0u; nstart[idx] = s + 1; cstart[idx] = q + 1;
	F.rend[r] = rend; F.rsl[r] = rsl;
	if (bad) ctl->flag = 1;
}

__global__ void __launch_bounds__(256) rp_scatter(rp_file_t F, int f, int nf, uint32_t nuse, const uint32_t *__restrict__ lens, const uint64_t *__restrict__ offs,
                                                  uint8_t *__restrict__ ascii, uint8_t *__restrict__ codes, uint8_t *__restrict__ quals)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= F.n) return;
	const uint32_t j = F.lid[i] - 1;
	const int ro = F.role[j];
	if (ro != RL_SEQ && ro != RL_QUAL) return;
	const uint32_t r = F.rec[j];
	if (r >= nuse) return;
	const uint32_t t = i - F.L[j];
	if (t >= F.klen[j]) return;
	const uint32_t idx = (uint32_t)nf * r + (uint32_t)f, len = lens[idx];
	const uint8_t c = F.b[i];
	if (ro == RL_SEQ) {
		const uint32_t w = F.sloff[j] - F.rsl[r] + t;
		if (w < len) { const uint64_t d = offs[idx] + w; ascii[d] = c; codes[d] = rp_nt4(c); }
	} else if (t < len) quals[offs[idx] + t] = c;
}

__global__ void __launch_bounds__(256) rp_names(const uint8_t *__restrict__ b0, const uint8_t *__restrict__ b1, int nf, uint32_t nt, int comments,
                                                const uint32_t *__restrict__ nlen, const uint32_t *__restrict__ clen, const uint32_t *__restrict__ nstart, const uint32_t *__restrict__ cstart,
                                                const uint64_t *__restrict__ noffs, const uint64_t *__restrict__ coffs, uint8_t *__restrict__ names, uint8_t *__restrict__ cm)
{
	const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= nt) return;
	const uint8_t *b = (nf == 2 && (idx & 1u)) ? b1 : b0;
	{
		const uint32_t l = nlen[idx] - 1, s = nstart[idx]; uint8_t *d = names + noffs[idx];
		for (uint32_t k = 0; k < l; ++k) d[k] = b[s + k];
		d[l] = 0;
	}
	if (comments) {
		const uint32_t l = clen[idx] - 1, s = cstart[idx]; uint8_t *d = cm + coffs[idx];
		for (uint32_t k = 0; k < l; ++k) d[k] = b[s + k];
		d[l] = 0;
	}
}

// one file: its source and the window of its text
struct stream_t {
	std::string path; bmh_text_src_t *src = nullptr;
	uint8_t *buf = nullptr; size_t cap = 0, have = 0; bool eof = false, pinned = false; int kind = 0; uint64_t bytes = 0;
	// a BGZF file inflated on the device (csrc/inflate_kernels.hip): the window's text is dtext[cur][0 .. have) in HBM and never was on the host; whole compressed
	// members go up from hcomp, the statuses come back in hstat with the parser's first wait (check_status), and buf is the host's copy for the walker (mirror)
	bool on_dev = false, comp_busy = false; int cur = 0; uint32_t n_stat = 0; uint64_t n_dev_members = 0, comp_seen = 0, text_seen = 0;
	dev_buf<uint8_t> dtext[2], dcomp, dtab, dstat; pin_buf<uint8_t> hcomp, htab, hstat; std::vector<bmh_inflate_member_t> tab;
	uint8_t *text_dev() const { return dtext[cur].as<uint8_t>(); }
	int check_status()
	{
		comp_busy = false;
		const uint32_t *h = hstat.as<uint32_t>();
		for (uint32_t i = 0; i < n_stat; ++i) if (h[i]) { n_stat = 0; bmh_set_error("reads file: %s: damaged BGZF member (inflate, length or CRC)", path.c_str()); return BMH_EINVAL; }
		n_stat = 0;
		return BMH_OK;
	}
	// room for `bytes` of text, the text held kept
	int grow_text(size_t bytes, hipStream_t st)
	{
		if (dtext[cur].cap >= bytes) return BMH_OK;
		dev_buf<uint8_t> &o = dtext[1 - cur];
		if (o.need(bytes) != BMH_OK) return BMH_ENOMEM;
		if (have) { HIPCK(hipMemcpyAsync(o.p, dtext[cur].p, have, hipMemcpyDeviceToDevice, st)); HIPCK(hipStreamSynchronize(st)); }
		cur = 1 - cur;
		return BMH_OK;
	}
	int fill_dev(size_t target, hipStream_t st)
	{
		while (!eof && have < target) {
			if (comp_busy) { HIPCK(hipStreamSynchronize(st)); const int rc = check_status(); if (rc != BMH_OK) return rc; }     // (a second round of one window: poorly compressed members)
			const size_t want = target - have;
			// room for the compressed bytes of the text wanted, by the ratio this file has shown so far (half the text before any is known; at most all of it plus the
			// members' headers), so that a poorly compressed file does not take two rounds, and a fourth host wait, per window
			const double ratio = text_seen ? std::min(1.05, 1.25 * (double)comp_seen / (double)text_seen) : 0.5;
			if (hcomp.need(bmh_text_pending(src) + std::max<size_t>((size_t)1 << 20, (size_t)((double)want * ratio) + (256u << 10))) != BMH_OK) return BMH_ENOMEM;
			uint64_t text = 0; bool end = false;
			const int64_t r = bmh_text_members(src, hcomp.as<uint8_t>(), hcomp.cap, want, tab, &text, &end);
			if (r < 0) return BMH_EINVAL;
			if (end) eof = true;
			if (tab.empty()) { if (eof) break; bmh_set_error("reads file: %s: no whole BGZF member in %zu bytes", path.c_str(), hcomp.cap); return BMH_EINVAL; }
			const size_t nm = tab.size(), tb = nm * sizeof(bmh_inflate_member_t);
			if (nm >= 0xFFFFFFF0ull) { bmh_set_error("reads file: %s: 2^32 BGZF members in one window", path.c_str()); return BMH_EINVAL; }
			const int grc = grow_text(have + text + 16, st);
			if (grc != BMH_OK) return grc;
			if (dcomp.need((size_t)r + 16) != BMH_OK || dtab.need(tb) != BMH_OK || dstat.need(nm * 4) != BMH_OK || htab.need(tb) != BMH_OK || hstat.need(nm * 4) != BMH_OK) return BMH_ENOMEM;
			memcpy(htab.p, tab.data(), tb);
			HIPCK(hipMemcpyAsync(dcomp.p, hcomp.p, (size_t)r, hipMemcpyHostToDevice, st));
			HIPCK(hipMemcpyAsync(dtab.p, htab.p, tb, hipMemcpyHostToDevice, st));
			const int irc = bmh_inflate_members_device(dcomp.as<uint8_t>(), (uint64_t)r, dtab.as<bmh_inflate_member_t>(), (uint32_t)nm, text_dev() + have, text, dstat.as<uint32_t>(), st);
			if (irc != BMH_OK) return irc;
			HIPCK(hipMemcpyAsync(hstat.p, dstat.p, nm * 4, hipMemcpyDeviceToHost, st));
			comp_busy = true; n_stat = (uint32_t)nm; n_dev_members += nm; comp_seen += (uint64_t)r; text_seen += text;
			have += (size_t)text; bytes += text;
		}
		return BMH_OK;
	}
	// the text behind the first k bytes moves to the front: into the other buffer, in stream order
	int consume_dev(size_t k, hipStream_t st)
	{
		if (k >= have) { have = 0; return BMH_OK; }
		if (k == 0) return BMH_OK;
		const size_t rest = have - k;
		dev_buf<uint8_t> &o = dtext[1 - cur];
		if (o.need(rest + 16) != BMH_OK) return BMH_ENOMEM;
		HIPCK(hipMemcpyAsync(o.p, text_dev() + k, rest, hipMemcpyDeviceToDevice, st));
		cur = 1 - cur; have = rest;
		return BMH_OK;
	}
	// the window for the host walker: the rare path
	int mirror(hipStream_t st)
	{
		if (cap < have + 16) {
			uint8_t *nb = (uint8_t *)malloc(have + 16);
			if (!nb) { bmh_set_error("reads file: out of memory (%zu bytes of text)", have + 16); return BMH_ENOMEM; }
			free(buf); buf = nb; cap = have + 16;
		}
		if (comp_busy) { HIPCK(hipStreamSynchronize(st)); const int rc = check_status(); if (rc != BMH_OK) return rc; }
		if (have) { HIPCK(hipMemcpyAsync(buf, text_dev(), have, hipMemcpyDeviceToHost, st)); HIPCK(hipStreamSynchronize(st)); }
		return BMH_OK;
	}
	~stream_t() { if (src) bmh_text_close(src); release(buf); }
	void release(uint8_t *p) { if (!p) return; if (pinned && !on_dev) (void)hipHostFree(p); else free(p); }
	// room for a window of `target` bytes, the text held kept
	int reserve(size_t target)
	{
		if (cap < target + 16) {
			const size_t c = target + 16;
			uint8_t *nb = nullptr;
			if (pinned) { if (hipHostMalloc((void **)&nb, c) != hipSuccess) { (void)hipGetLastError(); nb = nullptr; } }
			else nb = (uint8_t *)malloc(c);
			if (!nb) { bmh_set_error("reads file: out of memory (%zu bytes of text)", c); return BMH_ENOMEM; }
			if (have) memcpy(nb, buf, have);
			release(buf); buf = nb; cap = c;
		}
		return BMH_OK;
	}
	int fill(size_t target)
	{
		if (eof || have >= target) return BMH_OK;
		RCK(reserve(target));
		const int64_t r = bmh_text_read(src, buf + have, target - have);
		if (r < 0) return BMH_EINVAL;
		if ((size_t)r < target - have) eof = true;
		have += (size_t)r; bytes += (uint64_t)r;
		return BMH_OK;
	}
	void consume(size_t k) { if (k >= have) { have = 0; return; } if (k) { memmove(buf, buf + k, have - k); have -= k; } }
};

// final: no further record can join this batch (the file -- with two files the one with fewer records in the window -- has ended)
struct result_t { uint64_t n_reads = 0; bool complete = false, final_ = false; size_t consumed[2] = {0, 0}; int kind[2] = {0, 0}; uint64_t extra[2] = {0, 0}; bool took_all = false; };

struct dev_parser_t {
	hipStream_t st = nullptr;
	static constexpr uint32_t PEEK = 64;
	int stream(hipStream_t *out) { if (!st) HIPCK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking)); *out = st; return BMH_OK; }
	struct per_file_t { dev_buf<uint8_t> b, lid, L, kind, klen, flag, fs, role, rec, seqk, sloff, hdr_line, seq_line, qual_line, rend, rsl, ctl; } D[2];
	dev_buf<uint8_t> tmp, lens, nlen, clen, nstart, cstart, offs, noffs, coffs, ascii, codes, quals, names, cm;
	pin_buf<uint8_t> h_small, h_lens, h_offs, h_noffs, h_coffs, h_rend[2];
	~dev_parser_t() { if (st) (void)hipStreamDestroy(st); }

	// 1: parsed (R; the arrays are in what alloc gave when the batch is delivered), 2: the window is the host's, < 0: error
	int run(stream_t *S, int nf, bool comments, uint64_t want_bases, uint64_t want_reads, bool even, bool take_all, const bmh_batch_alloc_t &alloc,
	        bmh_read_set_t *rs, result_t &R)
	{
		if (!st) HIPCK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
		rp_file_t F[2]; memset(F, 0, sizeof(F));
		// blank[f]: the file ends in this window and the window holds line ends alone ("\n" and "\r": what is left behind the last FASTQ record of a file that
		// ends in blank or CR LF lines).  kseq skips to the next header and finds none, so the bytes are consumed and no kernel runs: as FASTA text the lone CR
		// would raise the flag and the host would walk a window without a record
		bool blank[2] = {false, false};
		if (h_small.need(128 * sizeof(uint32_t)) != BMH_OK) return BMH_ENOMEM;
		uint32_t *hs = h_small.as<uint32_t>();
		uint64_t text = 0;
		for (int f = 0; f < nf; ++f) {
			per_file_t &P = D[f];
			const uint32_t n = (uint32_t)S[f].have;
			F[f].n = n; F[f].eof = S[f].eof; F[f].m = 0;
			text += n;
			if (n == 0) continue;
			if (S[f].on_dev) {
				// the text is in HBM already (inflated there): its first bytes come back with the line count
				if (P.lid.need((size_t)n * 4) != BMH_OK || P.ctl.need(sizeof(rp_ctl_t)) != BMH_OK) return BMH_ENOMEM;
				F[f].b = S[f].text_dev();
				HIPCK(hipMemcpyAsync(hs + 64 + 16 * f, F[f].b, std::min<uint32_t>(n, PEEK), hipMemcpyDeviceToHost, st));
			} else {
				size_t p = 0;
				while (p < n && (S[f].buf[p] == '\n' || S[f].buf[p] == '\r')) ++p;
				if (p < n && S[f].buf[p] != '>' && S[f].buf[p] != '@') return 2;
				F[f].fq = p < n && S[f].buf[p] == '@';
				if (p == n && S[f].eof) { blank[f] = true; continue; }
				if (P.b.need(n + 16) != BMH_OK || P.lid.need((size_t)n * 4) != BMH_OK || P.ctl.need(sizeof(rp_ctl_t)) != BMH_OK) return BMH_ENOMEM;
				HIPCK(hipMemcpyAsync(P.b.p, S[f].buf, n, hipMemcpyHostToDevice, st));
				F[f].b = P.b.as<uint8_t>();
			}
			HIPCK(hipMemsetAsync(P.ctl.p, 0, sizeof(rp_ctl_t), st));
			size_t tb = 0;
			auto in = rocprim::make_transform_iterator(rocprim::counting_iterator<uint32_t>(0), rp_ls_flag{F[f].b});
			HIPCK(rocprim::inclusive_scan(nullptr, tb, in, P.lid.as<uint32_t>(), (size_t)n, rocprim::plus<uint32_t>(), st));
			if (tb > tmp.cap) { HIPCK(hipStreamSynchronize(st)); if (tmp.need(tb) != BMH_OK) return BMH_ENOMEM; }
			HIPCK(rocprim::inclusive_scan(tmp.p, tb, in, P.lid.as<uint32_t>(), (size_t)n, rocprim::plus<uint32_t>(), st));
			HIPCK(hipMemcpyAsync(hs + f, P.lid.as<uint32_t>() + (n - 1), 4, hipMemcpyDeviceToHost, st));
			F[f].lid = P.lid.as<uint32_t>();
		}
		HIPCK(hipStreamSynchronize(st));
		for (int f = 0; f < nf; ++f) {
			if (!S[f].on_dev) continue;
			const int src_rc = S[f].check_status();                    // every member of the window inflated to its size and CRC, or the file is refused
			if (src_rc != BMH_OK) return src_rc;
			if (F[f].n == 0) continue;
			const uint8_t *pk = (const uint8_t *)(hs + 64 + 16 * f);
			const uint32_t np = std::min<uint32_t>(F[f].n, PEEK);
			uint32_t p = 0;
			while (p < np && (pk[p] == '\n' || pk[p] == '\r')) ++p;
			if (p == np ? np < F[f].n : (pk[p] != '>' && pk[p] != '@')) return 2;       // (more blank bytes than the peek holds: the host looks)
			F[f].fq = p < np && pk[p] == '@';
			if (p == np && F[f].eof) blank[f] = true;               // (np == n here)
		}
		for (int f = 0; f < nf; ++f) {
			if (F[f].n == 0 || blank[f]) continue;
			per_file_t &P = D[f];
			const uint32_t n = F[f].n, m = hs[f];
			F[f].m = m;
			const size_t m4 = (size_t)m * 4;
			if (P.L.need(m4) != BMH_OK || P.kind.need(m) != BMH_OK || P.klen.need(m4) != BMH_OK || P.flag.need(m4) != BMH_OK || P.fs.need(m4) != BMH_OK || P.role.need(m) != BMH_OK ||
			    P.rec.need(m4) != BMH_OK || P.seqk.need(m4) != BMH_OK || P.sloff.need(m4) != BMH_OK || P.hdr_line.need(m4 + 4) != BMH_OK || P.seq_line.need(m4 + 4) != BMH_OK ||
			    P.qual_line.need(m4 + 4) != BMH_OK || P.rend.need(m4 + 4) != BMH_OK || P.rsl.need(m4 + 4) != BMH_OK) return BMH_ENOMEM;
			F[f].L = P.L.as<uint32_t>(); F[f].klen = P.klen.as<uint32_t>(); F[f].flag = P.flag.as<uint32_t>(); F[f].fs = P.fs.as<uint32_t>(); F[f].seqk = P.seqk.as<uint32_t>();
			F[f].sloff = P.sloff.as<uint32_t>(); F[f].hdr_line = P.hdr_line.as<uint32_t>(); F[f].seq_line = P.seq_line.as<uint32_t>(); F[f].qual_line = P.qual_line.as<uint32_t>();
			F[f].rec = P.rec.as<uint32_t>(); F[f].role = P.role.as<uint8_t>(); F[f].rend = P.rend.as<uint32_t>(); F[f].rsl = P.rsl.as<uint32_t>();
			rp_ctl_t *ctl = P.ctl.as<rp_ctl_t>();
			const unsigned gb = (n + 255) / 256, gl = (m + 255) / 256;
			hipLaunchKernelGGL(rp_line_starts, dim3(gb), dim3(256), 0, st, F[f].b, n, F[f].lid, P.L.as<uint32_t>());
			hipLaunchKernelGGL(rp_line_kind, dim3(gl), dim3(256), 0, st, F[f].b, n, m, F[f].eof, F[f].fq, F[f].L, P.kind.as<uint8_t>(), P.klen.as<uint32_t>(), P.flag.as<uint32_t>(), ctl);
			size_t tb = 0;
			HIPCK(rocprim::exclusive_scan(nullptr, tb, P.flag.as<uint32_t>(), P.fs.as<uint32_t>(), 0u, (size_t)m, rocprim::plus<uint32_t>(), st));
			if (tb > tmp.cap) { HIPCK(hipStreamSynchronize(st)); if (tmp.need(tb) != BMH_OK) return BMH_ENOMEM; }
			HIPCK(rocprim::exclusive_scan(tmp.p, tb, P.flag.as<uint32_t>(), P.fs.as<uint32_t>(), 0u, (size_t)m, rocprim::plus<uint32_t>(), st));
			hipLaunchKernelGGL(rp_line_role, dim3(gl), dim3(256), 0, st, m, F[f].fq, P.kind.as<uint8_t>(), F[f].klen, F[f].flag, F[f].fs, P.role.as<uint8_t>(), P.rec.as<uint32_t>(),
			                   P.seqk.as<uint32_t>(), P.hdr_line.as<uint32_t>(), P.seq_line.as<uint32_t>(), P.qual_line.as<uint32_t>(), ctl);
			HIPCK(rocprim::exclusive_scan(tmp.p, tb, P.seqk.as<uint32_t>(), P.sloff.as<uint32_t>(), 0u, (size_t)m, rocprim::plus<uint32_t>(), st));
			HIPCK(hipMemcpyAsync(hs + 8 + 4 * f, ctl, sizeof(rp_ctl_t), hipMemcpyDeviceToHost, st));
		}
		HIPCK(hipStreamSynchronize(st));
		uint64_t nrec[2] = {0, 0};
		for (int f = 0; f < nf; ++f) {
			if (F[f].n == 0 || blank[f]) continue;
			const rp_ctl_t *c = (const rp_ctl_t *)(hs + 8 + 4 * f);
			if (c->flag) return 2;
			nrec[f] = F[f].fq ? c->n_flag_lines / 4 : (c->n_flag_lines ? c->n_flag_lines - (F[f].eof ? 0u : 1u) : 0u);
			if (F[f].fq && F[f].eof && (c->n_flag_lines & 3u)) return 2;                     // a truncated last record: the host names it
			R.kind[f] = nrec[f] ? (F[f].fq ? 2 : 1) : 0;
		}
		const uint64_t nuse = nf == 2 ? std::min(nrec[0], nrec[1]) : nrec[0];
		const uint64_t nt = nuse * (uint64_t)nf;
		R.extra[0] = nrec[0] - nuse; R.extra[1] = nf == 2 ? nrec[1] - nuse : 0;
		const bool final_ = nf == 1 ? F[0].eof != 0 : ((F[0].eof && nrec[0] <= nrec[1]) || (F[1].eof && nrec[1] <= nrec[0]));
		R.final_ = final_;
		R.n_reads = 0; R.complete = false; R.took_all = true; R.consumed[0] = R.consumed[1] = 0;
		if (nt == 0) { for (int f = 0; f < nf; ++f) if (F[f].eof && nrec[f] == 0) R.consumed[f] = F[f].n; return 1; }
		if (nt >= 0xFFFFFFF0ull) { bmh_set_error("reads parser: 2^32 records in one window"); return BMH_EINVAL; }
		const size_t t4 = (size_t)nt * 4, t8 = (size_t)(nt + 1) * 8;
		if (lens.need(t4) != BMH_OK || nlen.need(t4) != BMH_OK || clen.need(t4) != BMH_OK || nstart.need(t4) != BMH_OK || cstart.need(t4) != BMH_OK || offs.need(t8) != BMH_OK ||
		    noffs.need(t8) != BMH_OK || coffs.need(t8) != BMH_OK) return BMH_ENOMEM;
		if (ascii.need(text + 16) != BMH_OK || codes.need(text + 16) != BMH_OK || names.need(text + 16) != BMH_OK) return BMH_ENOMEM;
		if ((F[0].fq || F[1].fq) && quals.need(text + 16) != BMH_OK) return BMH_ENOMEM;          // (qualities and comments only where they are produced)
		if (comments && cm.need(text + 16) != BMH_OK) return BMH_ENOMEM;
		if (h_lens.need(t4) != BMH_OK || h_offs.need(t8) != BMH_OK || h_noffs.need(t8) != BMH_OK || h_coffs.need(t8) != BMH_OK) return BMH_ENOMEM;
		for (int f = 0; f < nf; ++f) {
			if (h_rend[f].need((size_t)nuse * 4) != BMH_OK) return BMH_ENOMEM;
			hipLaunchKernelGGL(rp_records, dim3((unsigned)((nuse + 255) / 256)), dim3(256), 0, st, F[f], f, nf, (uint32_t)nuse, comments ? 1 : 0, lens.as<uint32_t>(), nlen.as<uint32_t>(),
			                   clen.as<uint32_t>(), nstart.as<uint32_t>(), cstart.as<uint32_t>(), D[f].ctl.as<rp_ctl_t>());
		}
		{
			size_t tb = 0;
			auto in = rocprim::make_transform_iterator(lens.as<uint32_t>(), rp_to64());
			HIPCK(rocprim::exclusive_scan(nullptr, tb, in, offs.as<uint64_t>(), (uint64_t)0, (size_t)nt, rocprim::plus<uint64_t>(), st));
			if (tb > tmp.cap) { HIPCK(hipStreamSynchronize(st)); if (tmp.need(tb) != BMH_OK) return BMH_ENOMEM; }
			HIPCK(rocprim::exclusive_scan(tmp.p, tb, in, offs.as<uint64_t>(), (uint64_t)0, (size_t)nt, rocprim::plus<uint64_t>(), st));
			auto in2 = rocprim::make_transform_iterator(nlen.as<uint32_t>(), rp_to64());
			HIPCK(rocprim::exclusive_scan(tmp.p, tb, in2, noffs.as<uint64_t>(), (uint64_t)0, (size_t)nt, rocprim::plus<uint64_t>(), st));
			auto in3 = rocprim::make_transform_iterator(clen.as<uint32_t>(), rp_to64());
			HIPCK(rocprim::exclusive_scan(tmp.p, tb, in3, coffs.as<uint64_t>(), (uint64_t)0, (size_t)nt, rocprim::plus<uint64_t>(), st));
		}
		HIPCK(hipMemcpyAsync(h_lens.p, lens.p, t4, hipMemcpyDeviceToHost, st));
		HIPCK(hipMemcpyAsync(h_offs.p, offs.p, (size_t)nt * 8, hipMemcpyDeviceToHost, st));
		HIPCK(hipMemcpyAsync(h_noffs.p, noffs.p, (size_t)nt * 8, hipMemcpyDeviceToHost, st));
		HIPCK(hipMemcpyAsync(h_coffs.p, coffs.p, (size_t)nt * 8, hipMemcpyDeviceToHost, st));
		for (int f = 0; f < nf; ++f) {
			HIPCK(hipMemcpyAsync(h_rend[f].p, D[f].rend.p, (size_t)nuse * 4, hipMemcpyDeviceToHost, st));
			HIPCK(hipMemcpyAsync(hs + 8 + 4 * f, D[f].ctl.p, sizeof(rp_ctl_t), hipMemcpyDeviceToHost, st));
		}
		HIPCK(hipStreamSynchronize(st));
		for (int f = 0; f < nf; ++f) if (((const rp_ctl_t *)(hs + 8 + 4 * f))->flag) return 2;
		const uint32_t *hl = h_lens.as<uint32_t>();
		const uint64_t *ho = h_offs.as<uint64_t>(), *hn = h_noffs.as<uint64_t>(), *hc = h_coffs.as<uint64_t>();
		bool complete = false;
		const uint64_t k = take_all ? nt : bmh_cut_batch(hl, nt, nf, want_bases, want_reads, even, &complete);
		R.complete = complete; R.took_all = k == nt;
		if (!(complete || take_all || final_)) return 1;               // the window is too short for the batch: the pump reads on
		const uint64_t nb = k < nt ? ho[k] : ho[nt - 1] + hl[nt - 1];
		uint64_t nn, nc;
		{   // (the lengths of the last read's name and comment are on the device: from the spans of the next read, or of the whole)
			uint32_t last[2] = {0, 0};
			if (k == nt) {
				HIPCK(hipMemcpyAsync(&hs[32], nlen.as<uint32_t>() + (nt - 1), 4, hipMemcpyDeviceToHost, st));
				HIPCK(hipMemcpyAsync(&hs[33], clen.as<uint32_t>() + (nt - 1), 4, hipMemcpyDeviceToHost, st));
				HIPCK(hipStreamSynchronize(st));
				last[0] = hs[32]; last[1] = hs[33];
			}
			nn = k < nt ? hn[k] : hn[nt - 1] + last[0];
			nc = comments ? (k < nt ? hc[k] : hc[nt - 1] + last[1]) : 0;
		}
		const bool fq = F[0].fq;
		if (nf == 2 && F[0].fq != F[1].fq) { R.n_reads = 0; return 1; }       // (the pump refuses the pair of kinds)
		memset(rs, 0, sizeof(*rs));
		const int arc = alloc(k, nb, nn, nc, fq, rs);
		if (arc != BMH_OK) return arc;
		hipLaunchKernelGGL(rp_names, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, st, F[0].b, F[1].b, nf, (uint32_t)k, comments ? 1 : 0, nlen.as<uint32_t>(), clen.as<uint32_t>(),
		                   nstart.as<uint32_t>(), cstart.as<uint32_t>(), noffs.as<uint64_t>(), coffs.as<uint64_t>(), names.as<uint8_t>(), cm.as<uint8_t>());
		for (int f = 0; f < nf; ++f)
			hipLaunchKernelGGL(rp_scatter, dim3((F[f].n + 255) / 256), dim3(256), 0, st, F[f], f, nf, (uint32_t)(k / (uint64_t)nf), lens.as<uint32_t>(), offs.as<uint64_t>(), ascii.as<uint8_t>(),
			                   codes.as<uint8_t>(), quals.as<uint8_t>());
		HIPCK(hipMemcpyAsync(rs->ascii, ascii.p, nb, hipMemcpyDeviceToHost, st));
		if (rs->codes) HIPCK(hipMemcpyAsync(rs->codes, codes.p, nb, hipMemcpyDeviceToHost, st));
		if (fq && rs->quals) HIPCK(hipMemcpyAsync(rs->quals, quals.p, nb, hipMemcpyDeviceToHost, st));
		HIPCK(hipMemcpyAsync(rs->names, names.p, nn, hipMemcpyDeviceToHost, st));
		if (comments && rs->comments) HIPCK(hipMemcpyAsync(rs->comments, cm.p, nc, hipMemcpyDeviceToHost, st));
		memcpy(rs->offs, ho, k * 8); memcpy(rs->lens, hl, k * 4); memcpy(rs->name_offs, hn, k * 8);
		if (comments && rs->comment_offs) memcpy(rs->comment_offs, hc, k * 8);
		HIPCK(hipStreamSynchronize(st));
		rs->n_reads = k; rs->n_bases = nb; rs->n_name_bytes = nn; rs->n_comment_bytes = nc;
		R.n_reads = k;
		const uint64_t kf = k / (uint64_t)nf;
		for (int f = 0; f < nf; ++f) R.consumed[f] = kf ? h_rend[f].as<uint32_t>()[kf - 1] : 0;
		return 1;
	}
};

// the same contract on the host: records walked alternately from the windows
int host_run(stream_t *S, int nf, bool comments, uint64_t want_bases, uint64_t want_reads, bool even, bool take_all, const bmh_batch_alloc_t &alloc,
             bmh_read_set_t *rs, result_t &R, bmh_hbatch_t &hb)
{
	hb.clear();
	size_t p[2] = {0, 0};
	int kind[2] = {S[0].kind, nf == 2 ? S[1].kind : 0};
	uint64_t acc = 0, cnt = 0; bool complete = false, final_ = false;
	std::vector<size_t> ends[2];
	R = result_t();
	for (;;) {
		size_t p0 = p[0];
		int rc = bmh_walk_record(S[0].buf, S[0].have, S[0].eof, &p0, hb, comments, &kind[0]);
		if (rc < 0) return rc;
		if (rc == 0) {
			if (nf == 2 && S[0].eof) {                         // does the second file go on?
				bmh_hbatch_t t; size_t q = p[1]; int k2 = kind[1];
				const int r2 = bmh_walk_record(S[1].buf, S[1].have, S[1].eof, &q, t, false, &k2);
				if (r2 < 0) return r2;
				if (r2 == 1) R.extra[1] = 1; else if (S[1].eof) p[1] = S[1].have;
			}
			if (S[0].eof) p[0] = S[0].have;
			final_ = S[0].eof;
			break;
		}
		if (nf == 2) {
			size_t p1 = p[1];
			rc = bmh_walk_record(S[1].buf, S[1].have, S[1].eof, &p1, hb, comments, &kind[1]);
			if (rc < 0) return rc;
			if (rc == 0) {                                     // the mate is not there (yet): the first file's record is taken back
				const uint32_t l = hb.lens.back(), nl_ = hb.nlen.back();
				hb.ascii.resize(hb.ascii.size() - l); if (kind[0] == 2) hb.quals.resize(hb.quals.size() - l);
				hb.names.resize(hb.names.size() - nl_); hb.lens.pop_back(); hb.nlen.pop_back();
				if (comments) { hb.comments.resize(hb.comments.size() - hb.clen.back()); hb.clen.pop_back(); }
				if (S[1].eof) { R.extra[0] = 1; p[1] = S[1].have; }
				final_ = S[1].eof;
				break;
			}
			if (kind[0] != kind[1]) { R.kind[0] = kind[0]; R.kind[1] = kind[1]; R.n_reads = 0; return 1; }
			p[1] = p1; ends[1].push_back(p1);
			acc += hb.lens[hb.lens.size() - 2]; ++cnt;
		}
		p[0] = p0; ends[0].push_back(p0);
		acc += hb.lens.back(); ++cnt;
		if (!take_all) {
			const bool full = want_reads ? cnt >= want_reads : acc >= want_bases;
			if (full && (!even || !(cnt & 1))) { complete = true; break; }
		}
	}
	R.kind[0] = cnt ? kind[0] : 0; R.kind[1] = cnt ? kind[1] : 0;
	R.complete = complete; R.took_all = !complete; R.final_ = final_;
	if (!(complete || take_all || final_)) return 1;
	R.consumed[0] = p[0]; R.consumed[1] = p[1];
	if (cnt == 0) return 1;
	const bool fq = kind[0] == 2;
	memset(rs, 0, sizeof(*rs));
	const int arc = alloc(cnt, hb.ascii.size(), hb.names.size(), comments ? hb.comments.size() : 0, fq, rs);
	if (arc != BMH_OK) return arc;
	memcpy(rs->ascii, hb.ascii.data(), hb.ascii.size());
	if (rs->codes) bmh_nt4_codes(hb.ascii.data(), rs->codes, hb.ascii.size());
	if (fq && rs->quals) memcpy(rs->quals, hb.quals.data(), hb.quals.size());
	memcpy(rs->names, hb.names.data(), hb.names.size());
	if (comments && rs->comments) memcpy(rs->comments, hb.comments.data(), hb.comments.size());
	uint64_t o = 0, no = 0, co = 0;
	for (uint64_t r = 0; r < cnt; ++r) {
		rs->offs[r] = o; rs->lens[r] = hb.lens[r]; rs->name_offs[r] = no; o += hb.lens[r]; no += hb.nlen[r];
		if (comments && rs->comment_offs) { rs->comment_offs[r] = co; co += hb.clen[r]; }
	}
	rs->n_reads = cnt; rs->n_bases = o; rs->n_name_bytes = no; rs->n_comment_bytes = comments ? co : 0;
	R.n_reads = cnt;
	return 1;
}

}   // namespace

struct bmh_reads_pump_t {
	stream_t S[2]; int nf = 1; bool comments = false, host_only = false;
	dev_parser_t *dev = nullptr; bmh_hbatch_t hb;
	size_t target = 0, chunk = 0; std::string pending; uint64_t n_dev = 0, n_host = 0, n_records = 0;
	// the third kind: S[0] delivers BAM records (csrc/bam_in_core.h), bs is what its windows share
	bool bam = false; bmh_bam_state_t bs; bmh_bam_dev_t *bdev = nullptr;
	std::vector<uint32_t> chain;                           // the record starts of S[0]'s window found so far; its last entry is where the walk stands
	bool keep_rg = false, markdup = false; bmh_rg_table_t rg;      // a run that keeps the input's read groups: the header's @RG lines (bam_open), their IDs in bs
	~bmh_reads_pump_t() { delete dev; if (bdev) bmh_bam_dev_free(bdev); if (bs.col) bmh_bam_collate_free(bs.col); }
};

namespace {
constexpr size_t MAX_WINDOW = ((size_t)1 << 31) - 4096;

// A BAM file is opened: its header (magic, text, reference table: walked and ignored) is consumed whole, and the first record that gives a read says whether the
// file holds pairs (flag 0x1) -- before a run starts its lanes.  The window grows by the doubling rule until it holds both.
int bam_open(bmh_reads_pump_t *P)
{
	stream_t &S = P->S[0];
	const char *path = S.path.c_str();
	P->bs.path = S.path;
	size_t t = P->chunk ? P->chunk : 65536;
	for (;;) {
		RCK(S.fill(t));
		const int64_t hb = bmh_bam_header_bytes(S.buf, S.have);
		if (hb < 0) { bmh_set_error("reads file: %s: no BAM header behind the magic bytes", path); return BMH_EINVAL; }
		if (hb > 0) {
			if (P->keep_rg) {                                   // the header's text is whole here, before a record is looked at: its @RG lines are the run's read groups
				const std::string what = "reads file: " + S.path;
				RCK(bmh_bam_header_groups(what.c_str(), (const char *)S.buf + 8, (size_t)((uint32_t)S.buf[4] | ((uint32_t)S.buf[5] << 8) | ((uint32_t)S.buf[6] << 16) | ((uint32_t)S.buf[7] << 24)), P->markdup, P->rg));
				P->bs.rg_off.assign(1, 0u);
				for (const std::string &id : P->rg.ids) { P->bs.rg_ids += id; P->bs.rg_off.push_back((uint32_t)P->bs.rg_ids.size()); }
			}
			S.consume((size_t)hb); break;
		}
		if (S.eof) { bmh_set_error("reads file: %s: the file ends inside the BAM header", path); return BMH_EINVAL; }
		if (t >= MAX_WINDOW) { bmh_set_error("reads file: %s: a BAM header of 2^31 bytes or more", path); return BMH_EINVAL; }
		t = std::min(MAX_WINDOW, t * 2);
	}
	for (;;) {
		RCK(S.fill(t));
		uint32_t flag = 0;
		const int k = bmh_bam_first_kept(S.buf, S.have, &flag);
		if (k == 1) P->bs.paired = (int)(flag & 1u);
		if (k != 0 || S.eof || t >= MAX_WINDOW) break;        // (found; damaged, cut or endless: the first parse names it)
		t = std::min(MAX_WINDOW, t * 2);
	}
	return BMH_OK;
}

// The window is filled a piece at a time and the chain of record starts walked behind every piece, while the bytes the inflate has just written are still in
// the loader thread's cache: the walk is one dependent load per record, and over a whole window that has left the cache it costs a memory latency each (31 ms per
// million 150 bp records measured that way).
int bam_fill(bmh_reads_pump_t *P)
{
	constexpr size_t PIECE = (size_t)1 << 20;
	stream_t &S = P->S[0];
	if (P->chain.empty()) P->chain.push_back(0);
	RCK(S.reserve(P->target));
	for (;;) {
		bmh_bam_chain_extend(S.buf, S.have, P->chain);
		if (S.eof || S.have >= P->target) return BMH_OK;
		RCK(S.fill(std::min(P->target, S.have + PIECE)));
	}
}

int bam_next(bmh_reads_pump_t *P, uint64_t want_bases, uint64_t want_reads, bool even, bool take_all, const bmh_batch_alloc_t &alloc, bmh_read_set_t *rs)
{
	stream_t &S = P->S[0];
	for (;;) {
		RCK(bam_fill(P));
		if (S.eof && S.have == 0) return bmh_bam_collate_end(P->bs);      // (BMH_OK is 0: the end; a run that collates refuses the records still open)
		const bmh_bam_win_t w = {S.buf, S.have, S.eof, P->comments, want_bases, want_reads, even, take_all, &P->chain};
		bmh_bam_res_t R;
		int rc = 2;
		if (!P->host_only) rc = bmh_bam_dev_run(P->bdev, P->bs, w, alloc, rs, R);
		if (rc == 2) { rc = bmh_bam_host_run(P->bs, w, alloc, rs, R, P->hb); if (rc >= 0) ++P->n_host; }
		else if (rc >= 0) ++P->n_dev;
		if (rc < 0) return rc;
		if (R.complete || (take_all && R.n_reads > 0) || R.final_) {
			S.consume(R.consumed);
			// (R.consumed is the start of record R.n_recs: the chain behind it stays, moved with the bytes)
			P->chain.erase(P->chain.begin(), P->chain.begin() + (size_t)R.n_recs);
			for (uint32_t &c : P->chain) c -= (uint32_t)R.consumed;
			P->bs.n_recs += R.n_recs; P->bs.n_skipped += R.skipped; P->bs.n_tags_left_out += R.tags_left_out; P->bs.qual = R.qual;
			P->n_records += R.n_reads;
			if (R.n_reads > 0) {
				if (!take_all && !P->chunk) P->target = std::min(MAX_WINDOW, R.consumed + R.consumed / 16 + (1u << 16));
				return 1;
			}
			if (S.eof && S.have == 0) return bmh_bam_collate_end(P->bs);
			if (R.consumed > 0 || (!S.eof && S.have < P->target)) continue;
		}
		// the window holds no complete batch (or not one whole record): a larger one
		if (P->target >= MAX_WINDOW) { bmh_set_error("reads file: a batch (or one record) needs more than 2^31 bytes of BAM records"); return BMH_EINVAL; }
		P->target = std::min(MAX_WINDOW, P->target * 2);
	}
}
}   // namespace

const bmh_rg_table_t *bmh_pump_read_groups(const bmh_reads_pump_t *p) { return p->keep_rg ? &p->rg : nullptr; }

void bmh_pump_collate_counts(const bmh_reads_pump_t *p, uint64_t out[5])
{
	memset(out, 0, 5 * sizeof(uint64_t));
	if (p->bs.col) bmh_bam_collate_counts(p->bs.col, out);
}

bool bmh_pump_collate_ended_open(const bmh_reads_pump_t *p) { return bmh_bam_collate_ended_open(p->bs.col); }

bmh_reads_pump_t *bmh_pump_open(const char *path1, const char *path2, int n_threads, bool comments, bool host_only, size_t chunk_bytes, bool keep_rg, bool markdup, bool collate, uint64_t collate_mem)
{
	bmh_reads_pump_t *P = new bmh_reads_pump_t();
	P->keep_rg = keep_rg; P->markdup = markdup;
	P->nf = path2 ? 2 : 1; P->comments = comments; P->host_only = host_only; P->chunk = chunk_bytes;
	const char *paths[2] = {path1, path2};
	for (int f = 0; f < P->nf; ++f) {
		P->S[f].path = paths[f]; P->S[f].pinned = !host_only;
		P->S[f].src = bmh_text_open(paths[f], n_threads);
		if (!P->S[f].src) { delete P; return nullptr; }
		// BGZF is inflated on the device when asked for (BMH_INFLATE_DEVICE=1: opt-in until its end-to-end rate against the host inflate is on record, DESIGN.md
		// section 4.8); BMH_INFLATE_HOST=1 overrides it (the A/B switch); a plain gzip stream stays with the host
		P->S[f].on_dev = !host_only && bmh_text_kind(P->S[f].src) == 2 && bmh_tune("INFLATE_DEVICE", 0) != 0 && bmh_tune("INFLATE_HOST", 0) == 0;
	}
	for (int f = 0; f < P->nf; ++f) {
		const int b = bmh_text_bam(P->S[f].src);
		if (b == 1 && P->nf == 1) { P->bam = true; continue; }
		if (b == 1) bmh_set_error("reads files: %s is a BAM file, which holds both reads of its pairs: no mates file is taken beside it", paths[f]);
		else if (b == 2) bmh_set_error("reads file: %s holds a BAM in a plain gzip stream: a BAM file is BGZF (what samtools and bgzip write)", paths[f]);
		if (b != 0) { delete P; return nullptr; }
	}
	if (P->bam) {
		// BAM always takes the host inflate, also with BMH_INFLATE_DEVICE=1: the record starts are a chain the host walks over the window it has just inflated
		P->S[0].on_dev = false;
		if (!host_only) P->bdev = bmh_bam_dev_create();
		if (collate) P->bs.col = bmh_bam_collate_create(collate_mem);
		if (bam_open(P) != BMH_OK) { delete P; return nullptr; }
		return P;
	}
	if (keep_rg) { bmh_set_error("reads file: %s: the input's read groups can be kept only when it is a BAM file (text input carries none)", path1); delete P; return nullptr; }
	if (!host_only) P->dev = new dev_parser_t();
	return P;
}

int bmh_pump_bam_paired(const bmh_reads_pump_t *p) { return p->bam ? p->bs.paired : -1; }
void bmh_pump_bam_counts(const bmh_reads_pump_t *p, uint64_t out[2]) { out[0] = p->bs.n_skipped; out[1] = p->bs.n_tags_left_out; }

void bmh_pump_counts(const bmh_reads_pump_t *p, uint64_t out[4])
{
	out[0] = p->n_dev; out[1] = p->n_host; out[2] = p->S[0].bytes + p->S[1].bytes; out[3] = p->n_records;
}

void bmh_pump_inflate_counts(const bmh_reads_pump_t *p, uint64_t out[2])
{
	out[0] = out[1] = 0;
	for (int f = 0; f < p->nf; ++f) { out[0] += p->S[f].n_dev_members; if (p->S[f].src) out[1] += bmh_text_host_members(p->S[f].src); }
}

void bmh_pump_close(bmh_reads_pump_t *p) { delete p; }

int bmh_pump_next(bmh_reads_pump_t *P, uint64_t want_bases, uint64_t want_reads, bool even, bool take_all, const bmh_batch_alloc_t &alloc, bmh_read_set_t *rs)
{
	if (!P->pending.empty()) { bmh_set_error("%s", P->pending.c_str()); return BMH_EINVAL; }
	const int nf = P->nf;
	if (P->target == 0) {
		if (P->chunk) P->target = P->chunk;
		else if (take_all) P->target = (size_t)64 << 20;
		else P->target = (size_t)std::min<uint64_t>(MAX_WINDOW, (want_reads ? want_reads * 400 : want_bases * 5 / 2) / (uint64_t)nf + (1u << 20));
	}
	if (P->bam) return bam_next(P, want_bases, want_reads, even, take_all, alloc, rs);
	for (;;) {
		hipStream_t st = nullptr;
		if (P->dev) { const int src = P->dev->stream(&st); if (src != BMH_OK) return src; }
		for (int f = 0; f < nf; ++f) { const int rc = P->S[f].on_dev ? P->S[f].fill_dev(std::min(P->target, MAX_WINDOW - 65536) /* (it ends on a whole member: up to 64 KiB beyond) */, st) : P->S[f].fill(P->target); if (rc != BMH_OK) return rc; }
		bool all_eof = true, any_eof = false, none_left = true;
		for (int f = 0; f < nf; ++f) { all_eof = all_eof && P->S[f].eof; any_eof = any_eof || P->S[f].eof; none_left = none_left && P->S[f].have == 0; }
		if (all_eof && none_left) {
			for (int f = 0; f < nf; ++f) if (P->S[f].comp_busy) {          // (members without text, the end-of-file marker among them, are checked as well)
				if (hipStreamSynchronize(st) != hipSuccess) { (void)hipGetLastError(); bmh_set_error("reads parser: hipStreamSynchronize failed"); return BMH_ENODEV; }
				const int src = P->S[f].check_status(); if (src != BMH_OK) return src;
			}
			return 0;
		}
		result_t R;
		int rc = 2;
		if (!P->host_only) rc = P->dev->run(P->S, nf, P->comments, want_bases, want_reads, even, take_all, alloc, rs, R);
		if (rc == 2) for (int f = 0; f < nf; ++f) if (P->S[f].on_dev) { const int mrc = P->S[f].mirror(st); if (mrc != BMH_OK) return mrc; }
		if (rc == 2) { rc = host_run(P->S, nf, P->comments, want_bases, want_reads, even, take_all, alloc, rs, R, P->hb); if (rc >= 0) ++P->n_host; }
		else if (rc >= 0) ++P->n_dev;
		if (rc < 0) return rc;
		for (int f = 0; f < nf; ++f) {
			if (R.kind[f] && P->S[f].kind && R.kind[f] != P->S[f].kind) { bmh_set_error("reads file: FASTA and FASTQ records mixed in one file"); return BMH_EINVAL; }
			if (R.kind[f]) P->S[f].kind = R.kind[f];
		}
		if (nf == 2 && P->S[0].kind && P->S[1].kind && P->S[0].kind != P->S[1].kind) {
			bmh_set_error("reads files: %s holds %s records and %s %s records", P->S[0].path.c_str(), P->S[0].kind == 2 ? "FASTQ" : "FASTA", P->S[1].path.c_str(), P->S[1].kind == 2 ? "FASTQ" : "FASTA");
			return BMH_EINVAL;
		}
		const bool deliver = R.complete || (take_all && R.n_reads > 0) || R.final_;
		if (deliver) {
			if (nf == 2) {
				for (uint64_t i = 0; i + 1 < R.n_reads; i += 2) {
					const char *a = (const char *)rs->names + rs->name_offs[i], *b = (const char *)rs->names + rs->name_offs[i + 1];
					if (strcmp(a, b) != 0) { bmh_set_error("reads files: pair %llu has different names in the two files: %s and %s", (unsigned long long)(P->n_records + i) / 2, a, b); return BMH_EINVAL; }
				}
				if (R.took_all && any_eof) {
					const int shorter = (R.extra[0] > 0 && P->S[1].eof) ? 1 : (R.extra[1] > 0 && P->S[0].eof) ? 0 : -1;
					if (shorter >= 0) {
						char msg[1024];
						snprintf(msg, sizeof(msg), "reads files: %s ends before %s (after %llu pairs)", P->S[shorter].path.c_str(), P->S[1 - shorter].path.c_str(), (unsigned long long)(P->n_records + R.n_reads) / 2);
						P->pending = msg;
					}
				}
			}
			for (int f = 0; f < nf; ++f) {
				if (!P->S[f].on_dev) P->S[f].consume(R.consumed[f]);
				else { const int crc = P->S[f].consume_dev(R.consumed[f], st); if (crc != BMH_OK) return crc; }
			}
			P->n_records += R.n_reads;
			if (R.n_reads > 0) {
				if (!take_all && !P->chunk) { size_t c = std::max(R.consumed[0], R.consumed[1]); P->target = std::min(MAX_WINDOW, c + c / 16 + (1u << 16)); }
				return 1;
			}
			if (!P->pending.empty()) { bmh_set_error("%s", P->pending.c_str()); return BMH_EINVAL; }
			if (all_eof) return 0;
			bool progress = false;
			for (int f = 0; f < nf; ++f) progress = progress || R.consumed[f] > 0 || (!P->S[f].eof && P->S[f].have < (P->S[f].on_dev ? std::min(P->target, MAX_WINDOW - 65536) : P->target));
			if (progress) continue;
		}
		// the window holds no complete batch: a larger one
		if (P->target >= MAX_WINDOW) { bmh_set_error("reads file: a batch (or one record) needs more than 2^31 bytes of text"); return BMH_EINVAL; }
		P->target = std::min(MAX_WINDOW, P->target * 2);
	}
}

// ---- the whole of one or two files as a read set
namespace { uint64_t g_last_counts[4] = {0, 0, 0, 0}, g_last_inflate[2] = {0, 0}, g_last_bam[2] = {0, 0}, g_last_collate[5] = {0, 0, 0, 0, 0}; std::mutex g_counts_mu; }

extern "C" int bmh_reads_last_collate_counts(bmh_collate_counts_t *out)
{
	if (!out) return BMH_EINVAL;
	std::lock_guard<std::mutex> lk(g_counts_mu);
	out->pairs = g_last_collate[0]; out->pairs_adjacent = g_last_collate[1]; out->open_records_peak = g_last_collate[2]; out->open_bytes_peak = g_last_collate[3];
	out->windows_to_host_for_hash_runs = g_last_collate[4];
	return BMH_OK;
}
void bmh_reads_note_collate_counts(const uint64_t *c) { std::lock_guard<std::mutex> lk(g_counts_mu); memcpy(g_last_collate, c, sizeof(g_last_collate)); }

extern "C" int bmh_reads_last_bam_counts(uint64_t *out) { if (!out) return BMH_EINVAL; std::lock_guard<std::mutex> lk(g_counts_mu); memcpy(out, g_last_bam, sizeof(g_last_bam)); return BMH_OK; }
void bmh_reads_note_bam_counts(const uint64_t *c) { std::lock_guard<std::mutex> lk(g_counts_mu); memcpy(g_last_bam, c, sizeof(g_last_bam)); }

extern "C" int bmh_reads_last_inflate_counts(uint64_t *out) { if (!out) return BMH_EINVAL; std::lock_guard<std::mutex> lk(g_counts_mu); memcpy(out, g_last_inflate, sizeof(g_last_inflate)); return BMH_OK; }
void bmh_reads_note_inflate_counts(const uint64_t *c) { std::lock_guard<std::mutex> lk(g_counts_mu); memcpy(g_last_inflate, c, sizeof(g_last_inflate)); }

extern "C" int bmh_reads_last_counts(uint64_t *out) { if (!out) return BMH_EINVAL; std::lock_guard<std::mutex> lk(g_counts_mu); memcpy(out, g_last_counts, sizeof(g_last_counts)); return BMH_OK; }
void bmh_reads_note_counts(const uint64_t *c) { std::lock_guard<std::mutex> lk(g_counts_mu); memcpy(g_last_counts, c, sizeof(g_last_counts)); }

extern "C" int bmh_reads_load_files(const char *path1, const char *path2, int n_threads, int flags, bmh_read_set_t *out) { return bmh_reads_load_files_ex(path1, path2, n_threads, flags, 0, out); }

extern "C" int bmh_reads_load_files_ex(const char *path1, const char *path2, int n_threads, int flags, uint64_t collate_mem, bmh_read_set_t *out)
{
	if (!path1 || !out) { bmh_set_error("bmh_reads_load_files: null argument"); return BMH_EINVAL; }
	memset(out, 0, sizeof(*out));
	const bool cm = (flags & BMH_READS_COMMENTS) != 0, host = (flags & BMH_READS_HOST) != 0, collate = (flags & BMH_READS_COLLATE) != 0, keep = (flags & BMH_READS_KEEP_RG) != 0;
	if (collate_mem && !collate) { bmh_set_error("bmh_reads_load_files: a cap of %llu bytes on the collation's open records without BMH_READS_COLLATE", (unsigned long long)collate_mem); return BMH_EINVAL; }
	if (!host) { int nd = 0; if (hipGetDeviceCount(&nd) != hipSuccess || nd == 0) { (void)hipGetLastError(); bmh_set_error("bmh_reads_load_files: no HIP device (BMH_READS_HOST parses on the host)"); return BMH_ENODEV; } }
	bmh_reads_pump_t *P = bmh_pump_open(path1, path2, n_threads, cm, host, (size_t)std::max(0, bmh_tune("READS_CHUNK_BYTES", 0)), keep, false, collate, collate_mem);
	if (!P) return BMH_EINVAL;
	if (collate && bmh_pump_bam_paired(P) < 0) {
		bmh_pump_close(P);
		bmh_set_error("reads file: %s: mates are collated by name (--collate) in BAM input only: text input is taken in the order of its records", path1);
		return BMH_EINVAL;
	}
	std::vector<uint8_t> ascii, codes, quals, names, comments; std::vector<uint64_t> offs, noffs, coffs; std::vector<uint32_t> lens, groups;
	bool fq_any = false;
	uint64_t r0 = 0, b0 = 0, n0 = 0, c0 = 0;
	bmh_batch_alloc_t alloc = [&](uint64_t nr, uint64_t nb, uint64_t nn, uint64_t nc, bool fq, bmh_read_set_t *rs) {
		r0 = lens.size(); b0 = ascii.size(); n0 = names.size(); c0 = comments.size();
		ascii.resize(b0 + nb); codes.resize(b0 + nb); if (fq) quals.resize(b0 + nb); names.resize(n0 + nn); if (cm) { comments.resize(c0 + nc); coffs.resize(r0 + nr); }
		offs.resize(r0 + nr); noffs.resize(r0 + nr); lens.resize(r0 + nr);
		if (keep) { groups.resize(r0 + nr); rs->groups = groups.data() + r0; }
		fq_any = fq_any || fq;
		rs->ascii = ascii.data() + b0; rs->codes = codes.data() + b0; rs->quals = fq ? quals.data() + b0 : nullptr; rs->names = names.data() + n0;
		rs->offs = offs.data() + r0; rs->name_offs = noffs.data() + r0; rs->lens = lens.data() + r0;
		if (cm) { rs->comments = comments.data() + c0; rs->comment_offs = coffs.data() + r0; }
		return (int)BMH_OK;
	};
	int rc;
	for (;;) {
		bmh_read_set_t rs;
		rc = bmh_pump_next(P, 0, 0, false, true, alloc, &rs);
		if (rc <= 0) break;
		for (uint64_t r = r0; r < lens.size(); ++r) { offs[r] += b0; noffs[r] += n0; if (cm) coffs[r] += c0; }
	}
	uint64_t cnt[4]; bmh_pump_counts(P, cnt); bmh_reads_note_counts(cnt);
	uint64_t icnt[2]; bmh_pump_inflate_counts(P, icnt); bmh_reads_note_inflate_counts(icnt);
	uint64_t bcnt[2]; bmh_pump_bam_counts(P, bcnt); bmh_reads_note_bam_counts(bcnt);
	uint64_t ccnt[5]; bmh_pump_collate_counts(P, ccnt); bmh_reads_note_collate_counts(ccnt);
	// the complete pairs come back with the refusal: a file that ends before the other, and with --collate a record that is still open at the file's end
	const bool partial = rc < 0 && (strstr(bmh_last_error(), " ends before ") != nullptr || (!lens.empty() && bmh_pump_collate_ended_open(P)));
	bmh_pump_close(P);
	if (rc < 0 && !partial) return rc;
	const uint64_t nr = lens.size(), nb = ascii.size(), nn = names.size(), nm = comments.size();
	out->n_reads = nr; out->n_bases = nb; out->n_name_bytes = nn;
	out->ascii = (uint8_t *)malloc(nb + 1); out->codes = (uint8_t *)malloc(nb + 1); out->offs = (uint64_t *)malloc(8 * (nr + 1)); out->lens = (uint32_t *)malloc(4 * (nr + 1));
	out->names = (uint8_t *)malloc(nn + 1); out->name_offs = (uint64_t *)malloc(8 * (nr + 1));
	bool ok = out->ascii && out->codes && out->offs && out->lens && out->names && out->name_offs;
	if (fq_any) { out->quals = (uint8_t *)malloc(nb + 1); ok = ok && out->quals; }
	if (cm) { out->n_comment_bytes = nm; out->comments = (uint8_t *)malloc(nm + 1); out->comment_offs = (uint64_t *)malloc(8 * (nr + 1)); ok = ok && out->comments && out->comment_offs; }
	if (keep) { out->groups = (uint32_t *)malloc(4 * (nr + 1)); ok = ok && out->groups; if (out->groups) memcpy(out->groups, groups.data(), 4 * nr); }
	if (!ok) { bmh_reads_free(out); bmh_set_error("bmh_reads_load_files: out of memory"); return BMH_ENOMEM; }
	memcpy(out->ascii, ascii.data(), nb); memcpy(out->codes, codes.data(), nb); out->ascii[nb] = out->codes[nb] = 0;
	memcpy(out->offs, offs.data(), 8 * nr); memcpy(out->lens, lens.data(), 4 * nr); memcpy(out->names, names.data(), nn); out->names[nn] = 0; memcpy(out->name_offs, noffs.data(), 8 * nr);
	if (fq_any) { memcpy(out->quals, quals.data(), nb); out->quals[nb] = 0; }
	if (cm) { memcpy(out->comments, comments.data(), nm); out->comments[nm] = 0; memcpy(out->comment_offs, coffs.data(), 8 * nr); }
	return partial ? BMH_EINVAL : BMH_OK;
}
