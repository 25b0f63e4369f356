// Read files of the host side: the layout the reference's seeding library parses (one '>' header line and one sequence line per
// read, /root/reference/src/GPUSeed/seed_gen.cu:1698-1728; the host takes the same file through kseq / bseq_read, src/bwa.c:48-66)
// into the flat arrays the device path takes: letters back to back (what goes to HBM), nt4 codes (nst_nt4_table: what the host
// tail and the SAM text use), offsets, lengths, names (the header up to the first blank, NUL-terminated, back to back).
// Two passes over the file in memory, both on host threads: count per chunk, then fill at the chunk's offsets.
// FASTQ (bmh_reads_load, bmh_reads_scan, bmh_aligner_run_file): four-line records -- '@' header, one sequence line, a '+' line, one quality line
// of the same length (kseq_read, src/kseq.h:180-220, reads the same files); the qualities land at the letters' offsets.  Comments: the header
// behind the first blank, as kseq cuts it (src/kseq.h:187, its trailing CR dropped at :140 when the comment is longer than that CR).
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <string>
#include <thread>
#include <chrono>
#include <vector>
#include "bmh_internal.h"
#include "bam_in_core.h"
#include "bam_collate_core.h"
#include "../../include/bwamem_hip.h"

namespace {

// a record's name: the header up to the first blank, without a trailing "/<digit>" (kseq's name, then trim_readno: src/bwa.c:27-31,57,62 -- "read/1" and "read/2"
// of an interleaved file are the same QNAME, and mem_sam_pe insists that the two names of a pair are equal, src/bwamem_pair.c:369)
inline size_t name_len(const uint8_t *buf, size_t s, size_t le)
{
	size_t q = s;
	while (q < le && buf[q] != ' ' && buf[q] != '\t') ++q;
	size_t n = q - s;
	if (n > 2 && buf[s + n - 2] == '/' && buf[s + n - 1] >= '0' && buf[s + n - 1] <= '9') n -= 2;
	return n;
}

// bad: 1 headers and sequence lines do not alternate, 2 a line of 2^32 bases, 3 .. 8 FASTQ (bad_msg)
struct counts_t { uint64_t reads = 0, bases = 0, name_bytes = 0, max_len = 0, comment_bytes = 0; int bad = 0; };

const char *bad_msg(int bad)
{
	switch (bad) {
	case 2: return "reads file: a sequence line of 2^32 bases or more";
	case 3: return "FASTQ: a quality line whose length differs from its sequence line";
	case 4: return "FASTQ: a record without its '+' line";
	case 5: return "FASTQ: the last record is truncated";
	case 6: return "FASTQ: a multi-line record (a sequence or quality over several lines)";
	case 7: return "reads file: FASTA and FASTQ records mixed in one file";
	case 8: return "FASTQ: a record with an empty sequence line";
	default: return "reads file: expected alternating '>' header and sequence lines";
	}
}
// (the FASTA-only entry points keep their one message: a '@' line where a '>' header belongs is a line out of place there)
inline const char *bad_msg_fasta(int bad) { return bad == 2 ? bad_msg(2) : bad_msg(1); }

// the comment of the header line [s, raw_le) (s behind the '>' / '@', raw_le at the '\n' or the end; le: raw_le without a trailing CR): kseq's -- the
// rest of the line behind the first blank, its trailing CR dropped only when the comment is longer than it; empty = none
inline void comment_span(const uint8_t *buf, size_t s, size_t le, size_t raw_le, size_t *cb, size_t *cl)
{
	size_t q = s;
	while (q < le && buf[q] != ' ' && buf[q] != '\t') ++q;
	*cb = q + 1; *cl = 0;
	if (q >= le) return;
	size_t l = raw_le - (q + 1);
	if (l > 1 && buf[raw_le - 1] == '\r') --l;
	*cl = l;
}

// nst_nt4_table (src/bntseq.c): A/a 0, C/c 1, G/g 2, T/t 3, everything else 4
struct nt4_table_t {
	uint8_t v[256];
	nt4_table_t() { memset(v, 4, sizeof(v)); v['A'] = v['a'] = 0; v['C'] = v['c'] = 1; v['G'] = v['g'] = 2; v['T'] = v['t'] = 3; }
};
const nt4_table_t NT4;

// walks the lines of buf[b, e): headers and sequence lines must alternate (blank lines, also "\r" alone, are skipped); FILL writes
// cm: the comments too (c.comment_bytes; FILL: o->comments / o->comment_offs from m0)
template <bool FILL, bool CODES = true>
void walk(const uint8_t *buf, size_t b, size_t e, counts_t &c, bmh_read_set_t *o, uint64_t r0, uint64_t b0, uint64_t n0, bool cm = false, uint64_t m0 = 0)
{
	bool want_hdr = true;
	uint64_t r = r0, nb = b0, nn = n0, nm = m0;
	size_t p = b;
	while (p < e) {
		const uint8_t *nl = (const uint8_t *)memchr(buf + p, '\n', e - p);
		size_t le = nl ? (size_t)(nl - buf) : e;
		const size_t raw_le = le;
		const size_t next = nl ? le + 1 : e;
		if (le > p && buf[le - 1] == '\r') --le;
		if (le > p) {
			const bool hdr = buf[p] == '>';
			if (hdr != want_hdr) { c.bad = want_hdr && buf[p] == '@' ? 7 : 1; return; }
			if (hdr) {
				const size_t nl_ = name_len(buf, p + 1, le);
				if (FILL) { memcpy(o->names + nn, buf + p + 1, nl_); o->names[nn + nl_] = 0; o->name_offs[r] = nn; }
				nn += nl_ + 1;
				if (cm) {
					size_t cb, cl; comment_span(buf, p + 1, le, raw_le, &cb, &cl);
					if (FILL) { memcpy(o->comments + nm, buf + cb, cl); o->comments[nm + cl] = 0; o->comment_offs[r] = nm; }
					nm += cl + 1;
				}
			} else {
				const size_t L = le - p;
				if (L >> 32) { c.bad = 2; return; }
				if (FILL) {
					memcpy(o->ascii + nb, buf + p, L);
					if (CODES) { const uint8_t *src = buf + p; uint8_t *dst = o->codes + nb; for (size_t i = 0; i < L; ++i) dst[i] = NT4.v[src[i]]; }
					o->offs[r] = nb; o->lens[r] = (uint32_t)L;
				}
				nb += L; ++r;
				if (!FILL && L > c.max_len) c.max_len = L;
			}
			want_hdr = !hdr;
		}
		p = next;
	}
	if (!want_hdr) { c.bad = 1; return; }                  // a header without its sequence line
	c.reads = r - r0; c.bases = nb - b0; c.name_bytes = nn - n0; c.comment_bytes = nm - m0;
}

// FASTQ: '@' header, sequence, '+' line, quality line of the sequence's length; blank lines (also "\r" alone) between records are skipped.  FILL writes
// the qualities at the letters' offsets (o->quals, if not NULL)
template <bool FILL, bool CODES = true>
void walk_fq(const uint8_t *buf, size_t b, size_t e, counts_t &c, bmh_read_set_t *o, uint64_t r0, uint64_t b0, uint64_t n0, bool cm = false, uint64_t m0 = 0)
{
	int st = 0;                                            // the line the record wants next: 0 header, 1 sequence, 2 '+', 3 quality
	uint64_t r = r0, nb = b0, nn = n0, nm = m0;
	size_t s_beg = 0, s_len = 0;
	size_t p = b;
	while (p < e) {
		const uint8_t *nl = (const uint8_t *)memchr(buf + p, '\n', e - p);
		size_t le = nl ? (size_t)(nl - buf) : e;
		const size_t raw_le = le;
		const size_t next = nl ? le + 1 : e;
		if (le > p && buf[le - 1] == '\r') --le;
		if (st == 0) {
			if (le == p) { p = next; continue; }
			if (buf[p] != '@') { c.bad = buf[p] == '>' ? 7 : 6; return; }
			const size_t nl_ = name_len(buf, p + 1, le);
			if (FILL) { memcpy(o->names + nn, buf + p + 1, nl_); o->names[nn + nl_] = 0; o->name_offs[r] = nn; }
			nn += nl_ + 1;
			if (cm) {
				size_t cb, cl; comment_span(buf, p + 1, le, raw_le, &cb, &cl);
				if (FILL) { memcpy(o->comments + nm, buf + cb, cl); o->comments[nm + cl] = 0; o->comment_offs[r] = nm; }
				nm += cl + 1;
			}
			st = 1;
		} else if (st == 1) {
			if (le == p || buf[p] == '+') { c.bad = 8; return; }
			s_beg = p; s_len = le - p;
			if (s_len >> 32) { c.bad = 2; return; }
			st = 2;
		} else if (st == 2) {
			if (le == p || buf[p] != '+') { c.bad = (le == p || buf[p] == '@' || buf[p] == '>') ? 4 : 6; return; }
			st = 3;
		} else {
			if (le - p != s_len) { c.bad = 3; return; }
			if (FILL) {
				memcpy(o->ascii + nb, buf + s_beg, s_len);
				if (CODES) { const uint8_t *src = buf + s_beg; uint8_t *dst = o->codes + nb; for (size_t i = 0; i < s_len; ++i) dst[i] = NT4.v[src[i]]; }
				if (o->quals) memcpy(o->quals + nb, buf + p, s_len);
				o->offs[r] = nb; o->lens[r] = (uint32_t)s_len;
			}
			nb += s_len; ++r;
			if (!FILL && s_len > c.max_len) c.max_len = s_len;
			st = 0;
		}
		p = next;
	}
	if (st != 0) { c.bad = 5; return; }
	c.reads = r - r0; c.bases = nb - b0; c.name_bytes = nn - n0; c.comment_bytes = nm - m0;
}

// either layout
template <bool FILL, bool CODES = true>
inline void walk_any(bool fq, const uint8_t *buf, size_t b, size_t e, counts_t &c, bmh_read_set_t *o, uint64_t r0, uint64_t b0, uint64_t n0, bool cm, uint64_t m0)
{
	if (fq) walk_fq<FILL, CODES>(buf, b, e, c, o, r0, b0, n0, cm, m0);
	else walk<FILL, CODES>(buf, b, e, c, o, r0, b0, n0, cm, m0);
}

// a FASTQ record starts at p: a '@' line whose line two below starts with '+' (a quality line that starts with '@' has a header and a sequence line below it)
inline bool fq_record_at(const uint8_t *buf, size_t p, size_t sz)
{
	if (p >= sz || buf[p] != '@') return false;
	const uint8_t *a = (const uint8_t *)memchr(buf + p, '\n', sz - p);
	if (!a) return false;
	size_t q = (size_t)(a - buf) + 1;
	if (q >= sz) return false;
	const uint8_t *b = (const uint8_t *)memchr(buf + q, '\n', sz - q);
	if (!b) return false;
	q = (size_t)(b - buf) + 1;
	return q < sz && buf[q] == '+';
}

// first record start at or behind p (FASTA: a '>' at the beginning of a line)
size_t next_record(const uint8_t *buf, size_t p, size_t sz, bool fq = false)
{
	if (p == 0) return 0;
	if (p >= sz) return sz;
	auto at = [&](size_t q) { return fq ? fq_record_at(buf, q, sz) : buf[q] == '>'; };
	if (buf[p - 1] == '\n' && at(p)) return p;
	while (p < sz) {
		const uint8_t *nl = (const uint8_t *)memchr(buf + p, '\n', sz - p);
		if (!nl) return sz;
		p = (size_t)(nl - buf) + 1;
		if (p < sz && at(p)) return p;
	}
	return sz;
}

} // namespace

int bmh_reads_detect(const uint8_t *buf, size_t sz)
{
	size_t p = 0;
	while (p < sz && (buf[p] == '\n' || buf[p] == '\r' || buf[p] == ' ' || buf[p] == '\t')) ++p;
	return p < sz && buf[p] == '@' ? 1 : 0;
}

// the whole file: fq_ok = FASTQ allowed (the first non-blank byte decides), cm = keep the comments; fn: the entry point's name in messages
static int load_reads(const char *fn, const char *path, int n_threads, bool fq_ok, bool cm, bmh_read_set_t *out)
{
	if (!path || !out) { bmh_set_error("%s: null argument", fn); return BMH_EINVAL; }
	memset(out, 0, sizeof(*out));
	const bool prof = getenv("BMH_IO_PROFILE") != nullptr;
	auto now = [] { return std::chrono::steady_clock::now(); };
	auto lap = [&](const char *what, std::chrono::steady_clock::time_point &t) { if (prof) { const auto n = now(); fprintf(stderr, "[reads_io] %s %.1f ms\n", what, std::chrono::duration<double, std::milli>(n - t).count()); t = n; } };
	auto tp = now();
	// the file is mapped, not copied (its pages come straight from the page cache; the two passes below read it on host threads); it has to be
	// a regular file (a FIFO or a process substitution cannot be mapped or cut at headers)
	const int fd = open(path, O_RDONLY);
	if (fd < 0) { bmh_set_error("%s: cannot open %s", fn, path); return BMH_EINVAL; }
	struct stat sb;
	if (fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode)) { close(fd); bmh_set_error("%s: %s is not a regular, seekable file", fn, path); return BMH_EINVAL; }
	const size_t sz = (size_t)sb.st_size;
	const uint8_t *buf = (const uint8_t *)"";
	if (sz) {
		void *m = mmap(nullptr, sz, PROT_READ, MAP_PRIVATE | MAP_POPULATE, fd, 0);
		if (m == MAP_FAILED) { close(fd); bmh_set_error("%s: cannot map %s (%zu bytes)", fn, path, sz); return BMH_ENOMEM; }
		(void)madvise(m, sz, MADV_SEQUENTIAL);
		buf = (const uint8_t *)m;
	}
	close(fd);
	auto unmap = [&]() { if (sz) (void)munmap((void *)buf, sz); };
	lap("read", tp);
	const bool fq = fq_ok && bmh_reads_detect(buf, sz);
	// chunks that begin at a record: the first one that starts a line at or behind the nominal cut
	unsigned T = n_threads > 0 ? (unsigned)n_threads : (unsigned)bmh_effective_cpus();      // (the CPUs the process is granted, not the ones the machine shows)
	if (T == 0) T = 1;
	if (T > 32) T = 32;                                    // (memory-bound beyond a few threads; the host may show hundreds of hardware threads)
	if (sz < (1u << 20)) T = 1;
	std::vector<size_t> cut(T + 1, sz);
	cut[0] = 0;
	for (unsigned t = 1; t < T; ++t) {
		size_t p = sz / T * t;
		if (p < cut[t - 1]) p = cut[t - 1];
		// (the first line start behind p, not p itself: what the loader always did)
		size_t c = sz;
		const uint8_t *nl = p < sz ? (const uint8_t *)memchr(buf + p, '\n', sz - p) : nullptr;
		if (nl) c = next_record(buf, (size_t)(nl - buf) + 1, sz, fq);
		cut[t] = c;
	}
	std::vector<counts_t> cnt(T);
	auto run = [&](auto fn_) {
		if (T == 1) { fn_(0u); return; }
		std::vector<std::thread> th;
		for (unsigned t = 0; t < T; ++t) th.emplace_back(fn_, t);
		for (auto &x : th) x.join();
	};
	run([&](unsigned t) { walk_any<false>(fq, buf, cut[t], cut[t + 1], cnt[t], nullptr, 0, 0, 0, cm, 0); });
	lap("count", tp);
	uint64_t nr = 0, nb = 0, nn = 0, nm = 0;
	std::vector<uint64_t> r0(T), b0(T), n0(T), m0(T);
	for (unsigned t = 0; t < T; ++t) {
		if (cnt[t].bad) {
			unmap();
			if (!fq_ok && cnt[t].bad == 2) bmh_set_error("%s: a sequence line of 2^32 bases or more", fn);
			else bmh_set_error("%s", fq_ok ? bad_msg(cnt[t].bad) : bad_msg_fasta(cnt[t].bad));
			return BMH_EINVAL;
		}
		r0[t] = nr; b0[t] = nb; n0[t] = nn; m0[t] = nm;
		nr += cnt[t].reads; nb += cnt[t].bases; nn += cnt[t].name_bytes; nm += cnt[t].comment_bytes;
	}
	out->n_reads = nr; out->n_bases = nb; out->n_name_bytes = nn;
	// (no MADV_HUGEPAGE on the two large arrays: with the kernel's defrag = madvise the fill pass sometimes stalled for a second in
	// direct compaction -- 60 ms or 1.7 s from one call to the next)
	out->ascii = (uint8_t *)malloc(nb + 1); out->codes = (uint8_t *)malloc(nb + 1);
	out->offs = (uint64_t *)malloc(8 * (nr + 1)); out->lens = (uint32_t *)malloc(4 * (nr + 1));
	out->names = (uint8_t *)malloc(nn + 1); out->name_offs = (uint64_t *)malloc(8 * (nr + 1));
	bool ok = out->ascii && out->codes && out->offs && out->lens && out->names && out->name_offs;
	if (fq) { out->quals = (uint8_t *)malloc(nb + 1); ok = ok && out->quals; }
	if (cm) { out->n_comment_bytes = nm; out->comments = (uint8_t *)malloc(nm + 1); out->comment_offs = (uint64_t *)malloc(8 * (nr + 1)); ok = ok && out->comments && out->comment_offs; }
	if (!ok) {
		unmap(); bmh_reads_free(out);
		bmh_set_error("%s: out of memory", fn); return BMH_ENOMEM;
	}
	out->ascii[nb] = out->codes[nb] = 0; out->names[nn] = 0;
	if (fq) out->quals[nb] = 0;
	if (cm) out->comments[nm] = 0;
	lap("alloc", tp);
	run([&](unsigned t) { counts_t c; walk_any<true>(fq, buf, cut[t], cut[t + 1], c, out, r0[t], b0[t], n0[t], cm, m0[t]); });
	lap("fill", tp);
	unmap();
	return BMH_OK;
}

extern "C" int bmh_reads_load_fasta(const char *path, int n_threads, bmh_read_set_t *out)
{
	return load_reads("bmh_reads_load_fasta", path, n_threads, false, false, out);
}

extern "C" int bmh_reads_load(const char *path, int n_threads, int flags, bmh_read_set_t *out)
{
	return load_reads("bmh_reads_load", path, n_threads, true, (flags & BMH_READS_COMMENTS) != 0, out);
}

extern "C" void bmh_reads_free(bmh_read_set_t *r)
{
	if (!r) return;
	free(r->ascii); free(r->codes); free(r->offs); free(r->lens); free(r->names); free(r->name_offs);
	free(r->quals); free(r->comments); free(r->comment_offs); free(r->groups);
	memset(r, 0, sizeof(*r));
}

// ---- a read file taken batch by batch (csrc/align_pipeline.hip: bmh_aligner_run_fasta).  The reference reads its batches one after the other while the
// previous one is aligned (bseq_read, src/bwa.c:48-66, inside kt_pipeline): reads are added until the batch holds at least chunk bases and an even number
// of reads.  Here the mapped file is cut the same way -- counted on host threads over a window of the expected size, the exact end found by walking the
// chunk in which the count is reached -- and a batch is then filled into the caller's arrays (pinned memory: the letters go to the device from there).
namespace {

// walks records from b until the batch is complete (bases >= want_bases, or reads == want_reads when that is not 0; an even count when `even`) or e is reached;
// reads0 / bases0: what the batch holds before b.  Returns the offset behind the last record taken; bad: the lines do not alternate
size_t walk_until(const uint8_t *buf, size_t b, size_t e, uint64_t reads0, uint64_t bases0, uint64_t want_bases, uint64_t want_reads, bool even, counts_t &c, bool *complete,
                  bool fq = false, bool cm = false)
{
	bool want_hdr = true;
	uint64_t r = reads0, nb = bases0, nn = 0, nm = 0;
	size_t p = b, last = b;
	*complete = false;
	while (p < e) {
		const uint8_t *nl = (const uint8_t *)memchr(buf + p, '\n', e - p);
		size_t le = nl ? (size_t)(nl - buf) : e;
		const size_t raw_le = le;
		const size_t next = nl ? le + 1 : e;
		if (le > p && buf[le - 1] == '\r') --le;
		if (le > p && fq) {                                 // a FASTQ record: its four lines, counted by walk_fq
			size_t q = p;
			for (int k = 0; k < 4 && q < e; ++k) { const uint8_t *x = (const uint8_t *)memchr(buf + q, '\n', e - q); q = x ? (size_t)(x - buf) + 1 : e; }
			counts_t one;
			walk_fq<false>(buf, p, q, one, nullptr, 0, 0, 0, cm, 0);
			if (one.bad) { c.bad = one.bad; return last; }
			nn += one.name_bytes; nm += one.comment_bytes; nb += one.bases; ++r; last = q;
			const bool full = want_reads ? r >= want_reads : nb >= want_bases;
			if (full && (!even || !(r & 1))) { *complete = true; c.reads = r - reads0; c.bases = nb - bases0; c.name_bytes = nn; c.comment_bytes = nm; return last; }
			p = q;
			continue;
		}
		if (le > p) {
			const bool hdr = buf[p] == '>';
			if (hdr != want_hdr) { c.bad = want_hdr && buf[p] == '@' ? 7 : 1; return last; }
			if (hdr) {
				nn += name_len(buf, p + 1, le) + 1;
				if (cm) { size_t cb, cl; comment_span(buf, p + 1, le, raw_le, &cb, &cl); nm += cl + 1; }
			} else {
				nb += le - p; ++r; last = next;
				const bool full = want_reads ? r >= want_reads : nb >= want_bases;
				if (full && (!even || !(r & 1))) { *complete = true; c.reads = r - reads0; c.bases = nb - bases0; c.name_bytes = nn; c.comment_bytes = nm; return last; }
			}
			want_hdr = !hdr;
		}
		p = next;
	}
	if (!want_hdr) { c.bad = 1; return last; }
	c.reads = r - reads0; c.bases = nb - bases0; c.name_bytes = nn; c.comment_bytes = nm;
	return e;
}

}   // namespace

// The end of the batch that starts at offset p of the mapped file (p at a record start): *end, and what it holds.  est_bytes: the caller's guess of its size in
// the file (0: none).  BMH_OK, or BMH_EINVAL (lines that do not alternate).  A batch that ends with the file may be short (and odd).
int bmh_fasta_cut(const uint8_t *buf, size_t sz, size_t p, uint64_t want_bases, uint64_t want_reads, bool even, int n_threads, size_t est_bytes,
                  size_t *end, uint64_t *n_reads, uint64_t *n_bases, uint64_t *n_name_bytes, const bmh_reads_fmt_t &fmt, uint64_t *n_comment_bytes)
{
	unsigned T = n_threads > 0 ? (unsigned)n_threads : 1u;
	if (T > 16) T = 16;
	const bool fq = fmt.fq, cm = fmt.comments;
	uint64_t ncm_dummy = 0;
	uint64_t *ncm = n_comment_bytes ? n_comment_bytes : &ncm_dummy;
	size_t window = est_bytes ? est_bytes + est_bytes / 16 + (1u << 16) : (size_t)(want_reads ? want_reads * (fq ? 400 : 200) : (want_bases + want_bases / 4) * (fq ? 2 : 1)) + (1u << 16);
	for (;;) {
		const size_t q = p + window >= sz ? sz : next_record(buf, p + window, sz, fq);
		const unsigned Tw = (q - p) < (1u << 20) ? 1u : T;
		std::vector<size_t> cut(Tw + 1, q);
		cut[0] = p;
		for (unsigned t = 1; t < Tw; ++t) { size_t c = next_record(buf, p + (q - p) / Tw * t, q, fq); if (c < cut[t - 1]) c = cut[t - 1]; cut[t] = c > q ? q : c; }
		std::vector<counts_t> cnt(Tw);
		if (Tw == 1) walk_any<false>(fq, buf, cut[0], cut[1], cnt[0], nullptr, 0, 0, 0, cm, 0);
		else { std::vector<std::thread> th; for (unsigned t = 0; t < Tw; ++t) th.emplace_back([&, t] { walk_any<false>(fq, buf, cut[t], cut[t + 1], cnt[t], nullptr, 0, 0, 0, cm, 0); }); for (auto &x : th) x.join(); }
		uint64_t r = 0, b = 0, nn = 0, nm = 0;
		for (unsigned t = 0; t < Tw; ++t) {
			if (cnt[t].bad) { bmh_set_error("%s", fmt.either ? bad_msg(cnt[t].bad) : bad_msg_fasta(cnt[t].bad)); return BMH_EINVAL; }
			const bool reached = want_reads ? r + cnt[t].reads >= want_reads : b + cnt[t].bases >= want_bases;
			if (reached) {                                          // the batch ends inside this chunk (or, for an even count, a record into the next ones)
				counts_t c; bool complete = false;
				const size_t e = walk_until(buf, cut[t], q, r, b, want_bases, want_reads, even, c, &complete, fq, cm);
				if (c.bad) { bmh_set_error("%s", fmt.either ? bad_msg(c.bad) : bad_msg_fasta(c.bad)); return BMH_EINVAL; }
				if (complete || q == sz) {
					*end = complete ? e : sz; *n_reads = r + c.reads; *n_bases = b + c.bases; *n_name_bytes = nn + c.name_bytes; *ncm = nm + c.comment_bytes;
					return BMH_OK;
				}
				break;                                               // (ran out of window behind the threshold: a larger window)
			}
			r += cnt[t].reads; b += cnt[t].bases; nn += cnt[t].name_bytes; nm += cnt[t].comment_bytes;
		}
		if (q == sz) { *end = sz; *n_reads = r; *n_bases = b; *n_name_bytes = nn; *ncm = nm; return BMH_OK; }
		window *= 2;
	}
}

// fills the batch [p, end) (bmh_fasta_cut's numbers) into o's arrays -- the caller's, large enough: ascii / codes / quals n_bases + 1, offs / lens / name_offs /
// comment_offs n_reads + 1, names n_name_bytes + 1, comments n_comment_bytes + 1 -- on n_threads host threads; o->codes may be NULL (no nt4 codes wanted),
// o->quals / o->comments too (not kept)
int bmh_fasta_fill(const uint8_t *buf, size_t p, size_t end, uint64_t n_reads, uint64_t n_bases, uint64_t n_name_bytes, int n_threads, bmh_read_set_t *o,
                   const bmh_reads_fmt_t &fmt, uint64_t n_comment_bytes)
{
	unsigned T = n_threads > 0 ? (unsigned)n_threads : 1u;
	if (T > 16) T = 16;
	if (end - p < (1u << 20)) T = 1;
	const bool fq = fmt.fq, cm = fmt.comments;
	std::vector<size_t> cut(T + 1, end);
	cut[0] = p;
	for (unsigned t = 1; t < T; ++t) { size_t c = next_record(buf, p + (end - p) / T * t, end, fq); if (c < cut[t - 1]) c = cut[t - 1]; cut[t] = c > end ? end : c; }
	std::vector<counts_t> cnt(T);
	auto run = [&](auto fn) { if (T == 1) { fn(0u); return; } std::vector<std::thread> th; for (unsigned t = 0; t < T; ++t) th.emplace_back(fn, t); for (auto &x : th) x.join(); };
	run([&](unsigned t) { walk_any<false>(fq, buf, cut[t], cut[t + 1], cnt[t], nullptr, 0, 0, 0, cm, 0); });
	std::vector<uint64_t> r0(T), b0(T), n0(T), m0(T);
	uint64_t nr = 0, nb = 0, nn = 0, nm = 0;
	for (unsigned t = 0; t < T; ++t) {
		if (cnt[t].bad) { bmh_set_error("%s", fmt.either ? bad_msg(cnt[t].bad) : bad_msg_fasta(cnt[t].bad)); return BMH_EINVAL; }
		r0[t] = nr; b0[t] = nb; n0[t] = nn; m0[t] = nm; nr += cnt[t].reads; nb += cnt[t].bases; nn += cnt[t].name_bytes; nm += cnt[t].comment_bytes;
	}
	if (nr != n_reads || nb != n_bases || nn != n_name_bytes || (cm && nm != n_comment_bytes)) { bmh_set_error("reads file: internal error: a batch counted twice gave different sizes"); return BMH_EINVAL; }
	o->n_reads = nr; o->n_bases = nb; o->n_name_bytes = nn; o->n_comment_bytes = cm ? nm : 0;
	uint8_t *codes = o->codes;
	bmh_read_set_t w = *o;
	const bool wcm = cm && o->comments && o->comment_offs;
	if (!wcm) { w.comments = nullptr; w.comment_offs = nullptr; o->comments = nullptr; o->comment_offs = nullptr; o->n_comment_bytes = 0; }
	if (!fq) { w.quals = nullptr; o->quals = nullptr; }
	run([&](unsigned t) { counts_t c; if (codes) walk_any<true, true>(fq, buf, cut[t], cut[t + 1], c, &w, r0[t], b0[t], n0[t], wcm, m0[t]); else walk_any<true, false>(fq, buf, cut[t], cut[t + 1], c, &w, r0[t], b0[t], n0[t], wcm, m0[t]); });
	return BMH_OK;
}

// a regular file mapped for reading from its start to its end: *buf [*sz], the caller's to munmap; an empty file: *sz = 0 and nothing mapped.  fn: the name in messages
int bmh_map_file(const char *fn, const char *path, const uint8_t **buf, size_t *sz)
{
	*buf = nullptr; *sz = 0;
	const int fd = open(path, O_RDONLY);
	if (fd < 0) { bmh_set_error("%s: cannot open %s", fn, path); return BMH_EINVAL; }
	struct stat sb;
	if (fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode)) { close(fd); bmh_set_error("%s: %s is not a regular, seekable file", fn, path); return BMH_EINVAL; }
	const size_t n = (size_t)sb.st_size;
	void *m = n ? mmap(nullptr, n, PROT_READ, MAP_PRIVATE, fd, 0) : nullptr;
	close(fd);
	if (m == MAP_FAILED) { bmh_set_error("%s: cannot map %s (%zu bytes)", fn, path, n); return BMH_ENOMEM; }
	if (n) (void)madvise(m, n, MADV_SEQUENTIAL);
	*buf = (const uint8_t *)m; *sz = n;
	return BMH_OK;
}

// reads, bases, name bytes and the longest read of a read file, without loading it (one counting pass of the mapped file on host threads): out[4]
static int scan_reads(const char *fn, const char *path, int n_threads, bool fq_ok, uint64_t *out)
{
	if (!path || !out) { bmh_set_error("%s: null argument", fn); return BMH_EINVAL; }
	out[0] = out[1] = out[2] = out[3] = 0;
	const uint8_t *buf = nullptr; size_t sz = 0;
	const int mrc = bmh_map_file(fn, path, &buf, &sz);
	if (mrc != BMH_OK || sz == 0) return mrc;
	void *m = (void *)buf;
	const bool fq = fq_ok && bmh_reads_detect(buf, sz);
	unsigned T = n_threads > 0 ? (unsigned)n_threads : (unsigned)bmh_effective_cpus();
	if (T == 0) T = 1;
	if (T > 32) T = 32;
	if (sz < (1u << 20)) T = 1;
	std::vector<size_t> cut(T + 1, sz);
	cut[0] = 0;
	for (unsigned t = 1; t < T; ++t) { size_t c = next_record(buf, sz / T * t, sz, fq); if (c < cut[t - 1]) c = cut[t - 1]; cut[t] = c; }
	std::vector<counts_t> cnt(T);
	if (T == 1) walk_any<false>(fq, buf, cut[0], cut[1], cnt[0], nullptr, 0, 0, 0, false, 0);
	else { std::vector<std::thread> th; for (unsigned t = 0; t < T; ++t) th.emplace_back([&, t] { walk_any<false>(fq, buf, cut[t], cut[t + 1], cnt[t], nullptr, 0, 0, 0, false, 0); }); for (auto &x : th) x.join(); }
	int rc = BMH_OK;
	for (unsigned t = 0; t < T; ++t) {
		if (cnt[t].bad) { bmh_set_error("%s", fq_ok ? bad_msg(cnt[t].bad) : bad_msg_fasta(cnt[t].bad)); rc = BMH_EINVAL; break; }
		out[0] += cnt[t].reads; out[1] += cnt[t].bases; out[2] += cnt[t].name_bytes; if (cnt[t].max_len > out[3]) out[3] = cnt[t].max_len;
	}
	(void)munmap(m, sz);
	return rc;
}

extern "C" int bmh_fasta_scan(const char *path, int n_threads, uint64_t *out) { return scan_reads("bmh_fasta_scan", path, n_threads, false, out); }
extern "C" int bmh_reads_scan(const char *path, int n_threads, uint64_t *out) { return scan_reads("bmh_reads_scan", path, n_threads, true, out); }

// ---- the host walker of bmh_reads_load_files / bmh_aligner_run_files: kseq_read (src/kseq.h:175-215) restated over a window of the text.  A record starts at
// the next '>' or '@' byte; its name runs to the first isspace byte, the comment is the rest of that line (a trailing CR dropped when the comment is longer
// than it); the sequence is every following line until one that starts with '>', '@' or '+' (empty lines skipped; a trailing CR dropped unless it is the
// record's first sequence byte or a one-byte last line of the file); behind a '+' line the qualities are lines until their total length reaches the
// sequence's.  It is what the device parser (csrc/reads_parse.hip) must equal, its fallback, and the form that runs without a device.  Where kseq_read
// gives up silently (-2: bseq_read ends the run there) this refuses with a message, and so for an empty sequence and for FASTA and FASTQ records in one file.
void bmh_nt4_codes(const uint8_t *src, uint8_t *dst, size_t n) { for (size_t i = 0; i < n; ++i) dst[i] = NT4.v[src[i]]; }

static inline bool c_isspace(uint8_t c) { return c == ' ' || (c >= '\t' && c <= '\r'); }

// One record from b[*p, n) appended to o.  1: done, *p behind it; 0: none -- *p = n when the window ends the file (eof), else *p is where the unfinished
// record starts (more text is needed); < 0: refused (message set).  *kind: 0 at first, then 1 (FASTA) or 2 (FASTQ): what the file's records are
int bmh_walk_record(const uint8_t *b, size_t n, bool eof, size_t *pp, bmh_hbatch_t &o, bool comments, int *kind)
{
	size_t p = *pp;
	while (p < n && b[p] != '>' && b[p] != '@') ++p;
	*pp = p;
	if (p >= n) return 0;
	const size_t a0 = o.ascii.size(), q0 = o.quals.size(), n0 = o.names.size(), c0 = o.comments.size();
	auto more = [&]() { o.ascii.resize(a0); o.quals.resize(q0); o.names.resize(n0); o.comments.resize(c0); return 0; };
	auto line_end = [&](size_t q) { const uint8_t *x = q < n ? (const uint8_t *)memchr(b + q, '\n', n - q) : nullptr; return x ? (size_t)(x - b) : n; };
	size_t q = p + 1;
	while (q < n && !c_isspace(b[q])) ++q;
	if (q >= n) {
		if (!eof) return more();
		if (q == p + 1) { *pp = n; return 0; }                  // (a header byte that ends the file makes no record)
	}
	size_t nl_ = q - (p + 1);
	size_t cb = q, cl = 0;
	if (q < n && b[q] != '\n') {
		const size_t le = line_end(q + 1);
		if (le >= n && !eof) return more();
		cb = q + 1; cl = le - cb;
		if (cl > 1 && b[cb + cl - 1] == '\r') --cl;
		q = le < n ? le + 1 : n;
	} else if (q < n) ++q;
	int c = -1;
	for (;;) {
		if (q >= n) { if (!eof) return more(); c = -1; break; }
		c = b[q];
		if (c == '>' || c == '@' || c == '+') break;
		if (c == '\n') { ++q; continue; }
		const size_t le = line_end(q);
		if (le >= n && !eof) return more();
		o.ascii.insert(o.ascii.end(), b + q, b + le);
		const bool lone_last = le >= n && le - q == 1;           // (kseq: the rest of the line is empty and the file ends -- nothing is trimmed)
		if (!lone_last && o.ascii.size() - a0 > 1 && o.ascii.back() == '\r') o.ascii.pop_back();
		q = le < n ? le + 1 : n;
	}
	const size_t L = o.ascii.size() - a0;
	const int k = c == '+' ? 2 : 1;
	if (c == '+') {
		size_t le = line_end(q);
		if (le >= n) { if (!eof) return more(); bmh_set_error("%s", bad_msg(5)); return BMH_EINVAL; }
		q = le + 1;
		bool ended = false;
		do {
			if (q >= n) { if (!eof) return more(); ended = true; break; }
			le = line_end(q);
			if (le >= n && !eof) return more();
			o.quals.insert(o.quals.end(), b + q, b + le);
			if (o.quals.size() - q0 > 1 && o.quals.back() == '\r') o.quals.pop_back();
			q = le < n ? le + 1 : n;
		} while (o.quals.size() - q0 < L);
		if (o.quals.size() - q0 != L) { bmh_set_error("%s", bad_msg(ended ? 5 : 3)); return BMH_EINVAL; }
	}
	if (*kind && *kind != k) { bmh_set_error("%s", bad_msg(7)); return BMH_EINVAL; }
	*kind = k;
	if (L == 0) { bmh_set_error("%s", k == 2 ? bad_msg(8) : "reads file: a record with an empty sequence"); return BMH_EINVAL; }
	if (L > 0x7fffffffu) { bmh_set_error("%s", bad_msg(2)); return BMH_EINVAL; }
	if (nl_ > 2 && b[p + nl_ - 1] == '/' && b[p + nl_] >= '0' && b[p + nl_] <= '9') nl_ -= 2;         // trim_readno (src/bwa.c:27-31)
	o.names.insert(o.names.end(), b + p + 1, b + p + 1 + nl_); o.names.push_back(0);
	if (comments) { o.comments.insert(o.comments.end(), b + cb, b + cb + cl); o.comments.push_back(0); o.clen.push_back((uint32_t)cl + 1); }
	o.lens.push_back((uint32_t)L); o.nlen.push_back((uint32_t)nl_ + 1);
	*pp = q;
	return 1;
}

// ---- BAM records as reads, the host form (csrc/bam_in_core.h has the rules): the definition the device kernels (csrc/bam_in_kernels.hip) must equal, the fallback
// that words their refusals -- every one names the record's index in the file -- and what BMH_READS_HOST runs without a device.
int64_t bmh_bam_header_bytes(const uint8_t *b, size_t n)
{
	if (n >= 4 && memcmp(b, "BAM\1", 4) != 0) return -1;
	if (n < 12) return 0;
	size_t p = 8 + (size_t)bi_u32(b + 4);                  // magic, l_text, text: walked and ignored
	if (n < p + 4 || p + 4 < p) return 0;
	const uint32_t n_ref = bi_u32(b + p);
	p += 4;
	for (uint32_t i = 0; i < n_ref; ++i) {                 // l_name, name, l_ref
		if (n < p + 4) return 0;
		p += 8 + (size_t)bi_u32(b + p);
		if (n < p) return 0;
	}
	return (int64_t)p;
}

void bmh_bam_chain_extend(const uint8_t *b, size_t n, std::vector<uint32_t> &starts)
{
	for (size_t p = starts.back(); n - p >= 4;) {
		const size_t e = p + 4 + (size_t)bi_u32(b + p);
		if (e > n) break;
		starts.push_back((uint32_t)e);
		p = e;
	}
}

void bmh_bam_chain(const uint8_t *b, size_t n, std::vector<uint32_t> &starts)
{
	starts.assign(1, 0u);
	bmh_bam_chain_extend(b, n, starts);
}

// for scripts/reads_input_rate.py, not part of the public interface: the chain walk alone over records in memory -- *n_records whole records, *end where they end
extern "C" int bmh_bam_chain_count(const uint8_t *records, uint64_t n_bytes, uint64_t *n_records, uint64_t *end)
{
	if ((!records && n_bytes) || !n_records || !end || n_bytes >= ((uint64_t)1 << 31)) { bmh_set_error("bmh_bam_chain_count: null argument, or 2^31 bytes or more"); return BMH_EINVAL; }
	std::vector<uint32_t> starts;
	bmh_bam_chain(records, (size_t)n_bytes, starts);
	*n_records = starts.size() - 1; *end = starts.back();
	return BMH_OK;
}

int bmh_bam_first_kept(const uint8_t *b, size_t n, uint32_t *flag)
{
	for (size_t p = 0; n - p >= 4;) {
		const size_t e = p + 4 + (size_t)bi_u32(b + p);
		if (e > n) return 0;
		if (e - p < 36) return -1;                           // (damaged: the parse names it)
		const uint32_t f = bi_u16(b + p + 18);
		if (!(f & BI_SKIP_FLAGS)) { *flag = f; return 1; }
		p = e;
	}
	return 0;
}

// ---- the pool of a run that collates mates by name (csrc/bam_collate_core.h)
bcl_pool_t *bmh_bam_collate_create(uint64_t mem_bytes)
{
	bcl_pool_t *p = new bcl_pool_t();
	if (mem_bytes) p->cap = mem_bytes;
	p->hash_bits = std::min(64, std::max(1, bmh_tune("COLLATE_HASH_BITS", 64)));
	return p;
}
void bmh_bam_collate_free(bcl_pool_t *p) { delete p; }
bool bmh_bam_collate_ended_open(const bcl_pool_t *p) { return p && p->ended_open; }
void bmh_bam_collate_counts(const bcl_pool_t *p, uint64_t out[5])
{
	out[0] = p->cnt.pairs; out[1] = p->cnt.pairs_adjacent; out[2] = p->cnt.open_records_peak; out[3] = p->cnt.open_bytes_peak; out[4] = p->cnt.windows_to_host_for_hash_runs;
}
int bmh_bam_collate_end(const bmh_bam_state_t &st)
{
	if (!st.collate() || st.col->n == 0) return BMH_OK;
	const uint32_t s = (uint32_t)st.col->smallest();
	st.col->ended_open = true;
	bmh_set_error("reads file: %s: BAM record %llu (%s): flag 0x1 and no partner", st.path.c_str(), (unsigned long long)st.col->slots[s].index, st.col->name(s));
	return BMH_EINVAL;
}

int bmh_bam_host_run(const bmh_bam_state_t &st, const bmh_bam_win_t &w, const bmh_batch_alloc_t &alloc, bmh_read_set_t *rs, bmh_bam_res_t &R, bmh_hbatch_t &hb)
{
	hb.clear();
	R = bmh_bam_res_t(); R.qual = st.qual;
	std::vector<uint32_t> walked;
	if (!w.chain) bmh_bam_chain(w.buf, w.have, walked);
	const std::vector<uint32_t> &starts = w.chain ? *w.chain : walked;
	const size_t nrec = starts.size() - 1, chain_end = starts.back();
	const char *path = st.path.c_str();
	auto idx = [&](size_t i) { return (unsigned long long)(st.n_recs + i); };
	auto name = [&](size_t i) { return (const char *)w.buf + starts[i] + BI_NAME_OFF; };
	int qual = st.qual;
	uint64_t acc = 0, cnt = 0, skipped = 0, left_out = 0;
	bool complete = false;
	size_t pend = (size_t)-1, i = 0; bi_rec_t pend_rec; uint32_t pend_hq = 0, pend_g = 0;
	const bool keep = st.keep_rg();
	const bi_groups_t G = {(const uint8_t *)st.rg_ids.data(), st.rg_off.data(), keep ? (uint32_t)st.rg_off.size() - 1 : 0u};
	auto gid = [&](uint32_t g) { return st.rg_ids.substr(st.rg_off[g], st.rg_off[g + 1] - st.rg_off[g]); };
	auto append_rec = [&](const uint8_t *r, const bi_rec_t &B, uint32_t hq, uint32_t g) {
		for (uint32_t t = 0; t < B.l_seq; ++t) hb.ascii.push_back(bi_base(r, B, t));
		if (hq) for (uint32_t t = 0; t < B.l_seq; ++t) hb.quals.push_back(bi_qual(r, B, t));
		hb.names.insert(hb.names.end(), r + BI_NAME_OFF, r + BI_NAME_OFF + B.l_name);
		hb.lens.push_back(B.l_seq); hb.nlen.push_back(B.l_name);
		if (keep) hb.grp.push_back(g);
		uint32_t lo = 0;
		const uint32_t cl = bi_comment(r, B, nullptr, 0, &lo);
		left_out += lo;
		if (w.comments) {
			const size_t c0 = hb.comments.size();
			hb.comments.resize(c0 + cl + 1);
			(void)bi_comment(r, B, hb.comments.data() + c0, cl, &lo);
			hb.comments[c0 + cl] = 0; hb.clen.push_back(cl + 1);
		}
		acc += B.l_seq; ++cnt;
	};
	auto append = [&](size_t k, const bi_rec_t &B, uint32_t hq, uint32_t g) { append_rec(w.buf + starts[k], B, hq, g); };
	// mates collated by name (csrc/bam_collate_core.h): the walk below asks `cw` what a kept record does -- it opens its name, or closes the record that did
	bcl_pool_t *col = st.collate() ? st.col : nullptr;
	bcl_pool_t no_pool;
	bcl_walk_t cw(col ? *col : no_pool, w.buf, starts.data(), st.n_recs);
	auto commit = [&](size_t k) {
		R.consumed = starts[k + 1]; R.n_recs = k + 1; R.skipped = skipped; R.tags_left_out = left_out; R.qual = qual;
		if (!w.take_all) {
			const bool full = w.want_reads ? cnt >= w.want_reads : acc >= w.want_bases;
			if (full && (!w.even || !(cnt & 1))) complete = true;
		}
	};
	for (; i < nrec && !complete; ++i) {
		const uint8_t *r = w.buf + starts[i];
		bi_rec_t B;
		int s = bi_check(r, starts[i + 1] - starts[i], &B);
		if (s != BI_OK) { bmh_set_error("reads file: %s: BAM record %llu: %s", path, idx(i), bi_status_text(s)); return BMH_EINVAL; }
		const uint32_t role = bi_role(B.flag);
		if (role == 0) { ++skipped; continue; }
		uint32_t hq = 0;
		s = bi_check_kept(r, B, &hq);
		if (s != BI_OK) { bmh_set_error("reads file: %s: BAM record %llu (%s): %s", path, idx(i), name(i), bi_status_text(s)); return BMH_EINVAL; }
		if ((int)(B.flag & 1u) != st.paired) { bmh_set_error("reads file: %s: BAM record %llu (%s): the file mixes records with and without flag 0x1", path, idx(i), name(i)); return BMH_EINVAL; }
		if (qual && qual != (hq ? 1 : 2)) {
			bmh_set_error("reads file: %s: BAM record %llu (%s) has %s base qualities and the records before it have %s: a file mixes both", path, idx(i), name(i), hq ? "its" : "no", hq ? "none" : "theirs");
			return BMH_EINVAL;
		}
		qual = hq ? 1 : 2;
		uint32_t g = 0;
		if (keep) {                                          // (kept records only: a record skipped by its flag is never inspected for its group)
			s = bi_read_group(r, B, G, &g);
			if (s != BI_OK) { bmh_set_error("reads file: %s: BAM record %llu (%s): %s", path, idx(i), name(i), bi_status_text(s)); return BMH_EINVAL; }
		}
		if (!st.paired) { append(i, B, hq, g); commit(i); continue; }
		if (role == 3) { bmh_set_error("reads file: %s: BAM record %llu (%s): flag 0x1 with neither or both of 0x40 and 0x80", path, idx(i), name(i)); return BMH_EINVAL; }
		if (col) {
			bcl_partner_t pt;
			const int ev = cw.step((uint32_t)i, role, &pt);
			if (ev == BCL_OPENED) continue;
			if (ev == BCL_OVER_CAP) {
				bmh_set_error("reads file: %s: BAM record %llu: the open records (first mates that wait for their partners) hold more than --collate-mem %llu bytes", path, (unsigned long long)pt.index, (unsigned long long)col->cap);
				return BMH_EINVAL;
			}
			if (ev == BCL_SAME_ROLE) { bmh_set_error("reads file: %s: BAM records %llu and %llu (%s) both carry flag %s", path, (unsigned long long)pt.index, idx(i), name(i), role == 1 ? "0x40" : "0x80"); return BMH_EINVAL; }
			// the partner was checked when it was walked (in this window, or in the one it came to the pool from): its fields are read again, not refused again
			bi_rec_t PB; uint32_t phq = 0, pg = 0;
			(void)bi_check(pt.bytes, pt.size, &PB); (void)bi_check_kept(pt.bytes, PB, &phq);
			if (keep) {
				(void)bi_read_group(pt.bytes, PB, G, &pg);
				if (pg != g) {
					bmh_set_error("reads file: %s: BAM records %llu and %llu (%s) name different read groups (%s and %s): the two reads of a pair are of one", path, (unsigned long long)pt.index, idx(i), name(i), gid(pg).c_str(), gid(g).c_str());
					return BMH_EINVAL;
				}
			}
			if (role == 2) { append_rec(pt.bytes, PB, phq, pg); append(i, B, hq, g); }
			else { append(i, B, hq, g); append_rec(pt.bytes, PB, phq, pg); }
			cw.commit((uint32_t)i);
			commit(i);
			continue;
		}
		if (pend == (size_t)-1) { pend = i; pend_rec = B; pend_hq = hq; pend_g = g; continue; }
		if (strcmp(name(pend), name(i)) != 0) {
			bmh_set_error("reads file: %s: BAM records %llu and %llu carry different names (%s and %s): is the file grouped by read name?", path, idx(pend), idx(i), name(pend), name(i));
			return BMH_EINVAL;
		}
		if (bi_role(pend_rec.flag) == role) { bmh_set_error("reads file: %s: BAM records %llu and %llu (%s) both carry flag %s", path, idx(pend), idx(i), name(i), role == 1 ? "0x40" : "0x80"); return BMH_EINVAL; }
		if (keep && pend_g != g) {
			bmh_set_error("reads file: %s: BAM records %llu and %llu (%s) name different read groups (%s and %s): the two reads of a pair are of one", path, idx(pend), idx(i), name(i), gid(pend_g).c_str(), gid(g).c_str());
			return BMH_EINVAL;
		}
		if (role == 2) { append(pend, pend_rec, pend_hq, pend_g); append(i, B, hq, g); }
		else { append(i, B, hq, g); append(pend, pend_rec, pend_hq, pend_g); }
		pend = (size_t)-1;
		commit(i);
	}
	R.complete = complete;
	R.final_ = w.eof && !complete;
	if (R.final_) {
		// what the file's end leaves over is refused once the reads before it have been delivered
		if (cnt == 0 && chain_end < w.have) { bmh_set_error("reads file: %s: the file ends inside BAM record %llu", path, idx(nrec)); return BMH_EINVAL; }
		if (cnt == 0 && pend != (size_t)-1) { bmh_set_error("reads file: %s: BAM record %llu (%s): flag 0x1 and no partner", path, idx(pend), name(pend)); return BMH_EINVAL; }
		if (col && cnt == 0) {                               // every pair is delivered: what is open now stays open
			if (col->n) return bmh_bam_collate_end(st);
			const int64_t fo = cw.first_open();
			if (fo >= 0) { col->ended_open = true; bmh_set_error("reads file: %s: BAM record %llu (%s): flag 0x1 and no partner", path, idx((size_t)fo), name((size_t)fo)); return BMH_EINVAL; }
		}
		if (chain_end == w.have && pend == (size_t)-1 && !(col && cw.open_behind_commit())) { R.consumed = chain_end; R.n_recs = nrec; R.skipped = skipped; R.tags_left_out = left_out; R.qual = qual; }
	}
	if (!(complete || w.take_all || R.final_) || cnt == 0) { hb.clear(); return 1; }
	if (col) cw.deliver();
	// (the records behind the last commit -- a first record whose partner the window does not hold -- were not appended: append runs at the commit only)
	const bool fq = qual == 1;
	memset(rs, 0, sizeof(*rs));
	const int arc = alloc(cnt, hb.ascii.size(), hb.names.size(), w.comments ? hb.comments.size() : 0, fq, rs);
	if (arc != BMH_OK) return arc;
	memcpy(rs->ascii, hb.ascii.data(), hb.ascii.size());
	if (rs->codes) bmh_nt4_codes(hb.ascii.data(), rs->codes, hb.ascii.size());
	if (fq && rs->quals) memcpy(rs->quals, hb.quals.data(), hb.quals.size());
	memcpy(rs->names, hb.names.data(), hb.names.size());
	if (w.comments && rs->comments) memcpy(rs->comments, hb.comments.data(), hb.comments.size());
	if (keep && rs->groups) memcpy(rs->groups, hb.grp.data(), 4 * (size_t)cnt);
	uint64_t o = 0, no = 0, co = 0;
	for (uint64_t r = 0; r < cnt; ++r) {
		rs->offs[r] = o; rs->lens[r] = hb.lens[r]; rs->name_offs[r] = no; o += hb.lens[r]; no += hb.nlen[r];
		if (w.comments && rs->comment_offs) { rs->comment_offs[r] = co; co += hb.clen[r]; }
	}
	rs->n_reads = cnt; rs->n_bases = o; rs->n_name_bytes = no; rs->n_comment_bytes = w.comments ? co : 0;
	R.n_reads = cnt;
	return 1;
}

// ---- the read groups of a BAM header's text (declared in csrc/bmh_internal.h with its rules)
int bmh_bam_header_groups(const char *what, const char *text, size_t n, bool markdup, bmh_rg_table_t &T)
{
	T.clear();
	const void *nul = n ? memchr(text, 0, n) : nullptr;
	if (nul) n = (size_t)((const char *)nul - text);
	int n_line = 0;
	for (size_t p = 0; p < n;) {
		const char *nl = (const char *)memchr(text + p, '\n', n - p);
		size_t le = nl ? (size_t)(nl - text) : n;
		const size_t next = nl ? le + 1 : n;
		if (nl && le > p && text[le - 1] == '\r') --le;
		const std::string line(text + p, le - p);
		p = next;
		if (line.compare(0, 3, "@RG") != 0 || (line.size() > 3 && line[3] != '\t')) continue;
		++n_line;
		auto refuse = [&](const char *why) {
			bmh_set_error("%s: BAM header: @RG line %d ('%.120s'): %s", what, n_line, line.c_str(), why);
			T.clear();
			return (int)BMH_EINVAL;
		};
		std::string id, lb; bool has_id = false;
		for (size_t q = 3; q < line.size();) {                  // (line[q] is the tab in front of a field)
			const size_t e = std::min(line.find('\t', q + 1), line.size());
			const std::string f = line.substr(q + 1, e - q - 1);
			if (f.size() < 3 || f[2] != ':') return refuse("a field that is not XX:value");
			if (f.compare(0, 3, "ID:") == 0 && !has_id) { id = f.substr(3); has_id = true; }
			if (f.compare(0, 3, "LB:") == 0 && f.size() > 3) lb = f.substr(3);
			q = e;
		}
		if (!has_id || id.empty()) return refuse("no ID field, or an empty one");
		if (id.size() > 255) return refuse("an ID longer than 255 bytes");
		for (const std::string &o : T.ids) if (o == id) return refuse("its ID names an earlier @RG line's read group");
		if (T.ids.size() >= 65535) return refuse("more than 65535 read groups");
		if (lb.empty()) lb = "Unknown Library";
		size_t l = 0;
		while (l < T.lib_names.size() && T.lib_names[l] != lb) ++l;
		if (l == T.lib_names.size()) {
			if (markdup && l >= 255) return refuse("its library is the run's 256th: duplicate marking holds at most 255 (the library is a byte of the duplicate key)");
			T.lib_names.push_back(lb);
		}
		T.lines.push_back(line); T.ids.push_back(id); T.lib.push_back((int32_t)l);
	}
	if (T.ids.empty()) { bmh_set_error("%s: BAM header: no @RG line: the run keeps the input's read groups and the header names none", what); return BMH_EINVAL; }
	return BMH_OK;
}

// the table as one malloc'd blob for a caller without C++: every line with a '\n' behind it (*lines, *lines_bytes), and lib [*n_groups]; bmh_free both
extern "C" int bmh_bam_header_read_groups(const char *text, uint64_t n_bytes, int markdup, char **lines, uint64_t *lines_bytes, int32_t **lib, int32_t *n_groups)
{
	if ((!text && n_bytes) || !lines || !lines_bytes || !lib || !n_groups) { bmh_set_error("bmh_bam_header_read_groups: null argument"); return BMH_EINVAL; }
	*lines = nullptr; *lib = nullptr; *lines_bytes = 0; *n_groups = 0;
	bmh_rg_table_t T;
	const int rc = bmh_bam_header_groups("bmh_bam_header_read_groups", text ? text : "", (size_t)n_bytes, markdup != 0, T);
	if (rc != BMH_OK) return rc;
	std::string all;
	for (const std::string &l : T.lines) { all += l; all += '\n'; }
	*lines = (char *)malloc(all.size() + 1); *lib = (int32_t *)malloc(4 * T.lib.size());
	if (!*lines || !*lib) { free(*lines); free(*lib); *lines = nullptr; *lib = nullptr; bmh_set_error("bmh_bam_header_read_groups: out of memory"); return BMH_ENOMEM; }
	memcpy(*lines, all.data(), all.size()); (*lines)[all.size()] = 0; memcpy(*lib, T.lib.data(), 4 * T.lib.size());
	*lines_bytes = all.size(); *n_groups = (int32_t)T.lib.size();
	return BMH_OK;
}

// bmh_bam_reads_device / bmh_bam_reads_host: the records are one window that ends the file, and every read of it is taken.  d: the device form, or NULL
int bmh_bam_reads_run(const char *fn, bmh_bam_dev_t *d, const uint8_t *records, uint64_t n_bytes, int flags, bmh_read_set_t *out, const char *const *rg_ids, int n_groups, uint64_t collate_mem)
{
	memset(out, 0, sizeof(*out));
	const bool keep = rg_ids != nullptr;
	if (keep && (n_groups < 1 || n_groups > 65535)) { bmh_set_error("%s: %d read groups (1 .. 65535)", fn, n_groups); return BMH_EINVAL; }
	if (n_bytes >= ((uint64_t)1 << 31) - 4096) { bmh_set_error("%s: 2^31 bytes of records or more (offsets inside a window are 32-bit)", fn); return BMH_EINVAL; }
	const bool cm = (flags & BMH_READS_COMMENTS) != 0;
	bmh_bam_state_t st;
	struct pool_guard_t { bcl_pool_t *p = nullptr; ~pool_guard_t() { if (p) bmh_bam_collate_free(p); } } pool;
	if (collate_mem && !(flags & BMH_READS_COLLATE)) { bmh_set_error("%s: a cap of %llu bytes on the collation's open records without BMH_READS_COLLATE", fn, (unsigned long long)collate_mem); return BMH_EINVAL; }
	if (flags & BMH_READS_COLLATE) st.col = pool.p = bmh_bam_collate_create(collate_mem);
	st.path = "(records in memory)";
	if (keep) {
		st.rg_off.push_back(0);
		for (int g = 0; g < n_groups; ++g) {
			const size_t l = rg_ids[g] ? strlen(rg_ids[g]) : 0;
			if (l == 0 || l > 255) { bmh_set_error("%s: read group %d: an ID of %zu bytes (1 .. 255)", fn, g, l); return BMH_EINVAL; }
			for (int o = 0; o < g; ++o) if (strcmp(rg_ids[o], rg_ids[g]) == 0) { bmh_set_error("%s: read groups %d and %d share the ID '%s'", fn, o, g, rg_ids[g]); return BMH_EINVAL; }
			st.rg_ids += rg_ids[g]; st.rg_off.push_back((uint32_t)st.rg_ids.size());
		}
	}
	uint32_t flag = 0;
	if (bmh_bam_first_kept(records, (size_t)n_bytes, &flag) == 1) st.paired = (int)(flag & 1u);
	const bmh_batch_alloc_t alloc = [&](uint64_t nr, uint64_t nb, uint64_t nn, uint64_t nc, bool fq, bmh_read_set_t *rs) {
		out->ascii = (uint8_t *)malloc(nb + 1); out->codes = (uint8_t *)malloc(nb + 1); out->offs = (uint64_t *)malloc(8 * (nr + 1)); out->lens = (uint32_t *)malloc(4 * (nr + 1));
		out->names = (uint8_t *)malloc(nn + 1); out->name_offs = (uint64_t *)malloc(8 * (nr + 1));
		bool ok = out->ascii && out->codes && out->offs && out->lens && out->names && out->name_offs;
		if (fq) { out->quals = (uint8_t *)malloc(nb + 1); ok = ok && out->quals; }
		if (cm) { out->comments = (uint8_t *)malloc(nc + 1); out->comment_offs = (uint64_t *)malloc(8 * (nr + 1)); ok = ok && out->comments && out->comment_offs; }
		if (keep) { out->groups = (uint32_t *)malloc(4 * (nr + 1)); ok = ok && out->groups; }
		if (!ok) { bmh_set_error("%s: out of memory", fn); return (int)BMH_ENOMEM; }
		out->ascii[nb] = out->codes[nb] = 0; out->names[nn] = 0;
		if (fq) out->quals[nb] = 0;
		if (cm) out->comments[nc] = 0;
		*rs = *out;
		return (int)BMH_OK;
	};
	const bmh_batch_alloc_t none = [&](uint64_t, uint64_t, uint64_t, uint64_t, bool, bmh_read_set_t *) { bmh_set_error("%s: internal error: reads behind the end of the records", fn); return (int)BMH_EINVAL; };
	bmh_bam_win_t w = {records, (size_t)n_bytes, true, cm, 0, 0, false, true, nullptr};
	bmh_bam_res_t R; bmh_hbatch_t hb; bmh_read_set_t rs;
	memset(&rs, 0, sizeof(rs));
	int rc = 2;
	if (d) rc = bmh_bam_dev_run(d, st, w, alloc, &rs, R);
	if (rc == 2) rc = bmh_bam_host_run(st, w, alloc, &rs, R, hb);
	uint64_t skipped_behind = 0;
	if (rc >= 0 && R.consumed < n_bytes) {                  // what the end leaves over (a cut record, a record without its partner) is refused by name
		st.n_recs = R.n_recs; st.qual = R.qual;
		w.buf = records + R.consumed; w.have = (size_t)n_bytes - R.consumed;
		bmh_bam_res_t R2;
		rc = bmh_bam_host_run(st, w, none, &rs, R2, hb);
		// (a run that collates stops at the record that completes its last pair: records skipped by their flag may follow it)
		if (rc >= 0 && st.collate() && R2.consumed == w.have) skipped_behind = R2.skipped;
		else if (rc >= 0) { bmh_set_error("%s: internal error: the bytes behind the last read were not refused", fn); rc = BMH_EINVAL; }
	}
	if (rc >= 0) rc = bmh_bam_collate_end(st) == BMH_OK ? rc : BMH_EINVAL;
	{ uint64_t cc[5] = {0, 0, 0, 0, 0}; if (st.col) bmh_bam_collate_counts(st.col, cc); bmh_reads_note_collate_counts(cc); }      // (zeros after a call that did not collate)
	if (rc < 0 && !(R.n_reads && bmh_bam_collate_ended_open(st.col))) { bmh_reads_free(out); return rc; }
	if (R.n_reads) { out->n_reads = rs.n_reads; out->n_bases = rs.n_bases; out->n_name_bytes = rs.n_name_bytes; out->n_comment_bytes = rs.n_comment_bytes; }
	const uint64_t bc[2] = {R.skipped + skipped_behind, R.tags_left_out};
	bmh_reads_note_bam_counts(bc);
	return rc < 0 ? rc : BMH_OK;                            // (< 0: an open record at the end of a run that collates -- *out holds the complete pairs before it)
}

extern "C" int bmh_bam_reads_groups_host(const uint8_t *records, uint64_t n_bytes, int flags, const char *const *rg_ids, int n_groups, bmh_read_set_t *out)
{
	if ((!records && n_bytes) || !out || !rg_ids) { bmh_set_error("bmh_bam_reads_groups_host: null argument"); return BMH_EINVAL; }
	return bmh_bam_reads_run("bmh_bam_reads_groups_host", nullptr, records, n_bytes, flags, out, rg_ids, n_groups);
}

extern "C" int bmh_bam_reads_host(const uint8_t *records, uint64_t n_bytes, int flags, bmh_read_set_t *out)
{
	if ((!records && n_bytes) || !out) { bmh_set_error("bmh_bam_reads_host: null argument"); return BMH_EINVAL; }
	return bmh_bam_reads_run("bmh_bam_reads_host", nullptr, records, n_bytes, flags, out);
}
