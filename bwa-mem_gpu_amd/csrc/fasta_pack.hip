// `bwa index` from a FASTA (or .fa.gz) file on the MI355X: the file is packed into the 2-bit forward strand on the device,
// then bmh_index_build (csrc/index_build.hip) builds the FMD index from it, and the five files are written.
//
// What is reproduced: bns_fasta2bntseq + add1 (bwa_index/bntseq.c:233-330) over kseq_read (bwa_index/kseq.h:95-215), i.e.
// the .pac / .ann / .amb of the forward-only pass (bwtindex.c:340), with ambiguous bases replaced by lrand48() & 3 after
// srand48(11).  The rules, applied to every byte of the file:
//   - bytes before the first '>' or '@' are skipped; that byte starts the first header.  Afterwards a line whose first byte
//     is '>' or '@' is a header, '+' makes the file FASTQ (refused), '\n' is an empty line (skipped), anything else is a
//     sequence line: every byte but its '\n' is sequence, except a trailing '\r', which is dropped unless it is the first
//     sequence byte of its record (a lone "\r" first line) or a lone "\r" line at the end of the file;
//   - header: name up to the first isspace byte; if that byte is not '\n' the rest of the line is the comment (a trailing
//     '\r' dropped when the comment is longer than one byte).  A '>' that is the last byte of the file makes no record;
//   - hole: an ambiguous byte (nst_nt4_table >= 4) that differs from the record's previous sequence byte (0 at a record's
//     start) starts a hole; every ambiguous byte belongs to the hole started last, so a hole's length is the difference of
//     the ranks (among ambiguous bytes) of its start and of the next hole's start;
//   - the k-th ambiguous byte of the file becomes (X_{k+1} >> 17) & 3 with X_{j+1} = a X_j + c mod 2^48 from
//     X_0 = (11 << 16) | 0x330E: glibc's lrand48 after srand48(11), reached for any k by jumping ahead through the affine map.
// A sequence byte that is 0 or >= 128 is refused: the reference indexes its table with a signed char there.
//
// Device mapping, per chunk (chunk-local offsets are 32-bit, file / text offsets 64-bit):
//   1 line ids: inclusive scan of "byte i starts a segment" (i = 0, or byte i-1 is '\n') -> lid[i]; segment starts L[]
//   2 segments (lines, the first possibly continuing one of the previous chunk): kind from the first byte; a segmented scan
//     gives each its ordinal among the sequence lines of its record (saturated at 2: only "first" matters)
//   3 kept length of every segment (the '\n' and a dropped '\r' at its end are the only bytes of a sequence line not kept);
//     their scan is each segment's offset in the packed text, so kept bytes are scattered without a byte-level select
//   4 per kept byte: ambiguous flag, hole start flag; scan of the ambiguous flags = rank = index of the lrand48 draw
//   5 pack: one thread per output .pac byte, four bases each, ambiguous ones drawn by jump-ahead
//   6 hole starts and header segments selected (rocPRIM) and copied back; headers' text is read from the pinned chunk
// The file is read (or inflated by zlib, loaded with dlopen) by a host thread into pinned double buffers while the previous
// chunk is copied and packed.  The last byte of a chunk is held back and processed with the next one, so every byte has
// its successor at hand (the '\r' rule).
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include <dlfcn.h>
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <chrono>
#include <future>
#include <string>
#include <vector>
#define BMH_CK_PREFIX "index_fasta: "
#include "bmh_internal.h"
#include "devmem.h"

namespace {

enum { K_SEQ = 0, K_HDR = 1, K_EMPTY = 2, K_PLUS = 3 };
enum { ERR_FASTQ = 1, ERR_BYTE = 2 };

// bwa_index/bntseq.c:47 nst_nt4_table: A C G T (either case) -> 0..3, '-' -> 5, everything else 4
__device__ __forceinline__ int fp_nt4(unsigned c)
{
	switch (c | 32u) {
	case 'a': return (c == 'A' || c == 'a') ? 0 : 4;
	case 'c': return (c == 'C' || c == 'c') ? 1 : 4;
	case 'g': return (c == 'G' || c == 'g') ? 2 : 4;
	case 't': return (c == 'T' || c == 't') ? 3 : 4;
	default: return c == '-' ? 5 : 4;
	}
}

struct seg_t { uint32_t start, klen, loff; uint8_t kind, recfirst, real, pad; };
struct ord_t { uint32_t hdr, seq; };
struct ord_op {
	__host__ __device__ ord_t operator()(const ord_t &a, const ord_t &b) const
	{
		ord_t r;
		r.hdr = a.hdr | b.hdr;
		r.seq = b.hdr ? b.seq : (a.seq + b.seq > 2u ? 2u : a.seq + b.seq);
		return r;
	}
};
// "byte i starts a segment": i == 0 or byte i-1 is '\n'
struct ls_flag {
	const uint8_t *b;
	__host__ __device__ uint32_t operator()(uint32_t i) const { return (i == 0 || b[i - 1] == '\n') ? 1u : 0u; }
};

// what a chunk's kernels tell the host (one copy back at the end of a chunk)
struct ctl_t {
	uint32_t m, n_kept, n_amb, n_holes, n_hdr, err;
	uint32_t last_kind, last_ord, last_prev;
};
struct hole_dev_t { uint64_t off, rank; uint32_t ch, pad; };
struct hdr_dev_t { uint32_t start, loff; };

// lrand48 jump-ahead: jt[2j] = a^(2^j), jt[2j+1] = the additive term of 2^j steps (mod 2^48)
__constant__ uint64_t fp_jump[96];
constexpr uint64_t LR_MASK = (1ull << 48) - 1, LR_A = 0x5DEECE66Dull, LR_C = 0xB, LR_X0 = (11ull << 16) | 0x330E;

__device__ __forceinline__ int fp_draw(uint64_t k)    // (lrand48() & 3) of the k-th draw (0-based) after srand48(11)
{
	uint64_t s = (k + 1) & LR_MASK, x = LR_X0;
	for (int j = 0; s; ++j, s >>= 1)
		if (s & 1) x = (fp_jump[2 * j] * x + fp_jump[2 * j + 1]) & LR_MASK;
	return (int)(x >> 17) & 3;
}

__global__ void __launch_bounds__(256) fp_seg_starts(const uint8_t *__restrict__ b, uint32_t n, const uint32_t *__restrict__ lid, uint32_t *__restrict__ L)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	if (i == 0 || b[i - 1] == '\n') L[lid[i] - 1] = i;
}

__global__ void __launch_bounds__(256) fp_seg_kind(const uint8_t *__restrict__ b, uint32_t m, const uint32_t *__restrict__ L, int at_ls, int carry_kind,
                                                   seg_t *__restrict__ seg, ord_t *__restrict__ ord, uint8_t *__restrict__ hdr_flag, ctl_t *ctl)
{
	const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= m) return;
	const uint32_t s = L[j];
	const bool real = j > 0 || at_ls;
	int kind = carry_kind;
	if (real) {
		const uint8_t c = b[s];
		kind = (c == '>' || c == '@') ? K_HDR : c == '+' ? K_PLUS : c == '\n' ? K_EMPTY : K_SEQ;
	}
	if (kind == K_PLUS) ctl->err = ERR_FASTQ;
	seg_t g;
	g.start = s; g.klen = 0; g.loff = 0; g.kind = (uint8_t)kind; g.recfirst = 0; g.real = real; g.pad = 0;
	seg[j] = g;
	ord_t o; o.hdr = kind == K_HDR; o.seq = (kind == K_SEQ && real) ? 1u : 0u;
	ord[j] = o;
	hdr_flag[j] = kind == K_HDR && real;
}

// kept length of every segment; eof: the chunk ends the file (else byte n is the next chunk's first byte)
__global__ void __launch_bounds__(256) fp_seg_klen(const uint8_t *__restrict__ b, uint32_t n, uint32_t m, int eof, uint32_t carry_ord,
                                                   const uint32_t *__restrict__ L, seg_t *__restrict__ seg, const ord_t *__restrict__ ord, uint32_t *__restrict__ klen, ctl_t *ctl)
{
	const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= m) return;
	seg_t g = seg[j];
	const ord_t o = ord[j];
	uint32_t ordinal = o.hdr ? o.seq : (carry_ord + o.seq > 2u ? 2u : carry_ord + o.seq);
	if (j == m - 1) { ctl->last_kind = g.kind; ctl->last_ord = ordinal; }
	uint32_t k = 0;
	if (g.kind == K_SEQ) {
		const uint32_t s = g.start, e = j + 1 < m ? L[j + 1] : n;
		const bool nl = b[e - 1] == '\n';
		k = e - s - (nl ? 1u : 0u);
		if (k > 0) {
			const uint32_t p = s + k - 1;                   // the last byte before the line's end
			const bool first = p == s && g.real;            // ... is the line's first byte
			int next = nl ? '\n' : (eof ? -1 : b[n]);       // what follows it
			if (b[p] == '\r' && ((next == '\n' && !(first && ordinal == 1)) || (next == -1 && !first))) --k;
		}
		g.recfirst = g.real && ordinal == 1 && k > 0;
	}
	g.klen = k;
	seg[j] = g;
	klen[j] = k;
}

__global__ void __launch_bounds__(256) fp_seg_loff(uint32_t m, seg_t *__restrict__ seg, const uint32_t *__restrict__ lend, ctl_t *ctl)
{
	const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= m) return;
	seg[j].loff = lend[j] - seg[j].klen;
	if (j == m - 1) ctl->n_kept = lend[j];
}

// kept bytes -> the chunk's text (raw byte | 256 if it is its record's first sequence byte)
__global__ void __launch_bounds__(256) fp_scatter(const uint8_t *__restrict__ b, uint32_t n, const uint32_t *__restrict__ lid, const seg_t *__restrict__ seg,
                                                  uint16_t *__restrict__ t, ctl_t *ctl)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const seg_t g = seg[lid[i] - 1];
	if (g.kind != K_SEQ) return;
	const uint32_t r = i - g.start;
	if (r >= g.klen) return;
	const uint8_t c = b[i];
	if (c == 0 || c >= 128) ctl->err = ERR_BYTE;
	t[g.loff + r] = (uint16_t)(c | ((r == 0 && g.recfirst) ? 256u : 0u));
}

__global__ void __launch_bounds__(256) fp_flags(const uint16_t *__restrict__ t, uint32_t nk, uint32_t carry_prev, uint32_t *__restrict__ amb,
                                                uint8_t *__restrict__ hole, ctl_t *ctl)
{
	const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= nk) return;
	const uint32_t v = t[k], raw = v & 255u;
	const uint32_t prev = (v >> 8) ? 0u : k ? (t[k - 1] & 255u) : carry_prev;
	const bool a = fp_nt4(raw) >= 4;
	amb[k] = a;
	hole[k] = a && prev != raw;
	if (k == nk - 1) ctl->last_prev = raw;
}

__global__ void __launch_bounds__(256) fp_pack(const uint16_t *__restrict__ t, const uint32_t *__restrict__ arank, uint32_t nk, uint64_t P0, uint64_t amb0,
                                               uint8_t *__restrict__ pac)
{
	const uint64_t q = (P0 >> 2) + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (q > (P0 + nk - 1) >> 2) return;
	uint32_t v = (q == (P0 >> 2) && (P0 & 3)) ? pac[q] : 0u;     // the first byte is shared with the previous chunk
	for (int r = 0; r < 4; ++r) {
		const uint64_t P = q * 4 + (uint64_t)r;
		if (P < P0 || P >= P0 + nk) continue;
		const uint32_t k = (uint32_t)(P - P0);
		int c = fp_nt4(t[k] & 255u);
		if (c >= 4) c = fp_draw(amb0 + arank[k] - 1);
		v |= (uint32_t)c << ((3 - r) * 2);
	}
	pac[q] = (uint8_t)v;
}

__global__ void __launch_bounds__(256) fp_gather(const uint16_t *__restrict__ t, const uint32_t *__restrict__ arank, const uint32_t *__restrict__ hpos,
                                                 const seg_t *__restrict__ seg, const uint32_t *__restrict__ hseg, const ctl_t *ctl,
                                                 uint64_t P0, uint64_t amb0, hole_dev_t *__restrict__ holes, hdr_dev_t *__restrict__ hdrs)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < ctl->n_holes) {
		const uint32_t k = hpos[i];
		hole_dev_t h; h.off = P0 + k; h.rank = amb0 + arank[k] - 1; h.ch = t[k] & 255u; h.pad = 0;
		holes[i] = h;
	}
	if (i < ctl->n_hdr) {
		const seg_t g = seg[hseg[i]];
		hdr_dev_t h; h.start = g.start; h.loff = g.loff;
		hdrs[i] = h;
	}
}

// ---------------------------------------------------------------- host side

typedef void *(*gzopen_f)(const char *, const char *);
typedef int (*gzread_f)(void *, void *, unsigned);
typedef int (*gzclose_f)(void *);
typedef int (*gzbuffer_f)(void *, unsigned);

// a plain or gzip file (by its magic bytes, as xzopen does), read in pieces
struct source_t {
	FILE *f = nullptr;
	void *gz = nullptr, *zlib = nullptr;
	gzread_f gzread = nullptr; gzclose_f gzclose = nullptr;
	bool is_gz = false;
	~source_t() { close(); }
	void close()
	{
		if (f) fclose(f);
		if (gz) gzclose(gz);
		if (zlib) dlclose(zlib);
		f = nullptr; gz = nullptr; zlib = nullptr;
	}
	int open(const char *path)
	{
		FILE *p = fopen(path, "rb");
		if (!p) { bmh_set_error("index_fasta: cannot open %s: %s", path, strerror(errno)); return BMH_EINVAL; }
		unsigned char mg[2] = {0, 0};
		size_t got = fread(mg, 1, 2, p);
		is_gz = got == 2 && mg[0] == 0x1f && mg[1] == 0x8b;
		if (!is_gz) { rewind(p); f = p; return 0; }
		fclose(p);
		zlib = dlopen("libz.so.1", RTLD_NOW | RTLD_LOCAL);
		if (!zlib) { bmh_set_error("index_fasta: %s is gzip-compressed and zlib (libz.so.1) could not be loaded: %s", path, dlerror()); return BMH_EINVAL; }
		gzopen_f gzo = (gzopen_f)dlsym(zlib, "gzopen");
		gzread = (gzread_f)dlsym(zlib, "gzread");
		gzclose = (gzclose_f)dlsym(zlib, "gzclose");
		gzbuffer_f gzb = (gzbuffer_f)dlsym(zlib, "gzbuffer");
		if (!gzo || !gzread || !gzclose) { bmh_set_error("index_fasta: libz.so.1 lacks gzopen/gzread/gzclose"); return BMH_EINVAL; }
		gz = gzo(path, "rb");
		if (!gz) { bmh_set_error("index_fasta: gzopen %s failed", path); return BMH_EINVAL; }
		if (gzb) gzb(gz, 1u << 20);
		return 0;
	}
	// fills up to n bytes; returns the count, or -1 on a read / inflate error
	int64_t read(uint8_t *dst, size_t n)
	{
		size_t done = 0;
		while (done < n) {
			if (!is_gz) {
				size_t r = fread(dst + done, 1, n - done, f);
				done += r;
				if (r == 0) return ferror(f) ? -1 : (int64_t)done;
			} else {
				size_t want = n - done < (1u << 30) ? n - done : (1u << 30);
				int r = gzread(gz, dst + done, (unsigned)want);
				if (r < 0) return -1;
				if (r == 0) break;
				done += (size_t)r;
			}
		}
		return (int64_t)done;
	}
};

struct header_t { std::string text; uint64_t offset = 0; };
struct record_t { std::string name, comment; uint64_t offset; };

double secs(std::chrono::steady_clock::time_point a) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - a).count(); }

// a failed HIP call / a non-OK code ends bmh_fasta_pack through its `done:` label
#define FCK(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) { rc = bmh_hip_failed(BMH_CK_PREFIX, e_, #x); goto done; } } while (0)
#define FRC(x) do { if ((rc = (x)) != BMH_OK) goto done; } while (0)

struct packer_t {
	// device
	dev_buf<uint8_t> d_b; dev_buf<uint32_t> lid, L, klen, lend, amb, arank, hpos, hseg;
	dev_buf<seg_t> seg; dev_buf<ord_t> ord, ord2; dev_buf<uint8_t> hdr_flag, hole_flag; dev_buf<uint16_t> t;
	dev_buf<hole_dev_t> holes; dev_buf<hdr_dev_t> hdrs; dev_buf<ctl_t> ctl; dev_buf<uint8_t> tmp;
	uint8_t *d_pac = nullptr; uint64_t pac_cap = 0;      // (a plain pointer: it is handed to the caller at the end)
	// host
	pin_buf<uint8_t> h_buf[2]; pin_buf<ctl_t> h_ctl; pin_buf<hole_dev_t> h_holes; pin_buf<hdr_dev_t> h_hdrs;
	hipStream_t st = nullptr;
	size_t cap = 0;     // bytes per chunk buffer (one held-back byte + chunk_bytes)

	void free_work()
	{
		d_b.drop(); lid.drop(); L.drop(); klen.drop(); lend.drop(); amb.drop(); arank.drop(); hpos.drop(); hseg.drop(); seg.drop(); ord.drop(); ord2.drop();
		hdr_flag.drop(); hole_flag.drop(); t.drop(); holes.drop(); hdrs.drop(); ctl.drop(); tmp.drop();
		h_buf[0].drop(); h_buf[1].drop(); h_ctl.drop(); h_holes.drop(); h_hdrs.drop();
		if (st) (void)hipStreamDestroy(st);
		st = nullptr;
	}
	~packer_t() { free_work(); if (d_pac) (void)hipFree(d_pac); }
};

// the isspace of the C locale
inline bool c_isspace(unsigned char c) { return c == ' ' || (c >= '\t' && c <= '\r'); }

record_t parse_header(const header_t &h)
{
	record_t r;
	r.offset = h.offset;
	size_t i = 0;
	while (i < h.text.size() && !c_isspace((unsigned char)h.text[i])) ++i;
	r.name = h.text.substr(0, i);
	// the text holds no '\n': a name that runs to the line's end (or the file's) has no comment
	if (i < h.text.size()) {
		r.comment = h.text.substr(i + 1);
		if (r.comment.size() > 1 && r.comment.back() == '\r') r.comment.pop_back();
	}
	return r;
}

} // namespace

extern "C" int bmh_fasta_pack(const char *fa_path, size_t chunk_bytes, bmh_fasta_packed_t *out, bmh_index_fasta_stats_t *stats)
{
	int rc = 0;
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { bmh_set_error("bmh_fasta_pack: no HIP device"); return BMH_ENODEV; }
	if (!fa_path || !out) { bmh_set_error("bmh_fasta_pack: NULL argument"); return BMH_EINVAL; }
	memset(out, 0, sizeof(*out));
	if (chunk_bytes == 0) chunk_bytes = (size_t)256 << 20;
	if (chunk_bytes < 64 || chunk_bytes > ((size_t)1 << 31)) { bmh_set_error("bmh_fasta_pack: chunk_bytes %zu outside [64, 2^31]", chunk_bytes); return BMH_EINVAL; }
	bmh_index_fasta_stats_t S;
	memset(&S, 0, sizeof(S));
	const auto t_all = std::chrono::steady_clock::now();
	source_t src;
	packer_t P;
	std::vector<record_t> recs;
	std::vector<uint64_t> hole_off, hole_rank;
	std::vector<uint8_t> hole_ch;
	header_t hdr;
	bool hdr_open = false, started = false, at_ls = true, eof = false;
	uint32_t carry_kind = K_SEQ, carry_ord = 0, carry_prev = 0;
	uint64_t l_pac = 0, n_amb = 0, file_bytes = 0;
	size_t hold = 0;          // bytes at the front of the next buffer (the held-back byte)
	int cur = 0;
	std::future<int64_t> pending;
	size_t tb = 0;
	uint64_t jt[96];
	{
		uint64_t a = LR_A, c = LR_C;
		for (int j = 0; j < 48; ++j) { jt[2 * j] = a; jt[2 * j + 1] = c; c = (a * c + c) & LR_MASK; a = (a * a) & LR_MASK; }
	}
	if ((rc = src.open(fa_path)) != 0) return rc;
	P.cap = chunk_bytes + 1;
	FCK(hipStreamCreateWithFlags(&P.st, hipStreamNonBlocking));
	FCK(hipMemcpyToSymbol(HIP_SYMBOL(fp_jump), jt, sizeof(jt)));
	FRC(P.h_buf[0].resize(P.cap)); FRC(P.h_buf[1].resize(P.cap));
	FRC(P.h_ctl.resize(1));
	FRC(P.d_b.resize(P.cap + 8));
	FRC(P.lid.resize(P.cap)); FRC(P.L.resize(P.cap));
	FRC(P.klen.resize(P.cap)); FRC(P.lend.resize(P.cap));
	FRC(P.amb.resize(P.cap)); FRC(P.arank.resize(P.cap));
	FRC(P.hpos.resize(P.cap)); FRC(P.hseg.resize(P.cap));
	FRC(P.seg.resize(P.cap)); FRC(P.ord.resize(P.cap)); FRC(P.ord2.resize(P.cap));
	FRC(P.hdr_flag.resize(P.cap)); FRC(P.hole_flag.resize(P.cap)); FRC(P.t.resize(P.cap));
	FRC(P.ctl.resize(1));
	{   // one temporary buffer for every scan and select of a chunk
		size_t b1 = 0, b2 = 0, b3 = 0, b4 = 0;
		const uint32_t N = (uint32_t)P.cap;
		FCK(rocprim::inclusive_scan(nullptr, b1, rocprim::make_transform_iterator(rocprim::counting_iterator<uint32_t>(0), ls_flag{P.d_b.p}), P.lid.p, (size_t)N, rocprim::plus<uint32_t>(), P.st));
		FCK(rocprim::inclusive_scan(nullptr, b2, P.ord.p, P.ord2.p, (size_t)N, ord_op(), P.st));
		FCK(rocprim::inclusive_scan(nullptr, b3, P.klen.p, P.lend.p, (size_t)N, rocprim::plus<uint32_t>(), P.st));
		FCK(rocprim::select(nullptr, b4, rocprim::counting_iterator<uint32_t>(0), P.hole_flag.p, P.hpos.p, &P.ctl.p->n_holes, (size_t)N, P.st));
		tb = std::max(std::max(b1, b2), std::max(b3, b4));
		FRC(P.tmp.resize(tb));
	}
	{   // the .pac grows as needed; a plain file bounds it
		FILE *p = fopen(fa_path, "rb");
		uint64_t fsz = 0;
		if (p) { fseek(p, 0, SEEK_END); fsz = (uint64_t)ftell(p); fclose(p); }
		P.pac_cap = (src.is_gz ? 4 * fsz : fsz) / 4 + 64 + 1024;
		FCK(hipMalloc((void **)&P.d_pac, P.pac_cap));
		FCK(hipMemsetAsync(P.d_pac, 0, P.pac_cap, P.st));
	}
	{
		auto t0 = std::chrono::steady_clock::now();
		int64_t r = src.read(P.h_buf[0].p, chunk_bytes);
		S.read_seconds += secs(t0);
		if (r < 0) { bmh_set_error("index_fasta: read error in %s", fa_path); rc = BMH_EINVAL; goto done; }
		file_bytes += (uint64_t)r;
		hold = (size_t)r;          // bytes valid in buffer 0
		eof = (size_t)r < chunk_bytes;
	}
	for (;;) {
		uint8_t *hb = P.h_buf[cur].p;
		const size_t len = hold;
		// the next chunk is read while this one is packed; it starts with this one's last byte
		bool next_eof = true;
		if (!eof) {
			uint8_t *nb = P.h_buf[cur ^ 1].p;
			nb[0] = hb[len - 1];
			pending = std::async(std::launch::async, [&src, nb, chunk_bytes]() { return src.read(nb + 1, chunk_bytes); });
			next_eof = false;
		}
		const size_t n = eof ? len : len - 1;         // bytes processed now
		size_t off = 0;
		if (!started) {
			while (off < n && hb[off] != '>' && hb[off] != '@') ++off;
			if (off < n) { started = true; at_ls = true; }
		}
		if (started && off < n) {
			const uint32_t nn = (uint32_t)(n - off);
			const uint8_t *db = P.d_b.p + off;
			const uint64_t P0 = l_pac, A0 = n_amb;
			auto t0 = std::chrono::steady_clock::now();
			FCK(hipMemcpyAsync(P.d_b.p, hb, len, hipMemcpyHostToDevice, P.st));
			FCK(hipStreamSynchronize(P.st));
			S.h2d_seconds += secs(t0);
			t0 = std::chrono::steady_clock::now();
			FCK(hipMemsetAsync(P.ctl.p, 0, sizeof(ctl_t), P.st));
			size_t b = tb;
			FCK(rocprim::inclusive_scan(P.tmp.p, b, rocprim::make_transform_iterator(rocprim::counting_iterator<uint32_t>(0), ls_flag{db}), P.lid.p, (size_t)nn, rocprim::plus<uint32_t>(), P.st));
			const uint32_t g_n = (nn + 255) / 256;
			fp_seg_starts<<<g_n, 256, 0, P.st>>>(db, nn, P.lid.p, P.L.p);
			FCK(hipMemcpyAsync(&P.h_ctl.p->m, P.lid.p + nn - 1, 4, hipMemcpyDeviceToHost, P.st));
			FCK(hipStreamSynchronize(P.st));
			const uint32_t m = P.h_ctl.p->m, g_m = (m + 255) / 256;
			fp_seg_kind<<<g_m, 256, 0, P.st>>>(db, m, P.L.p, at_ls, (int)carry_kind, P.seg.p, P.ord.p, P.hdr_flag.p, P.ctl.p);
			b = tb;
			FCK(rocprim::inclusive_scan(P.tmp.p, b, P.ord.p, P.ord2.p, (size_t)m, ord_op(), P.st));
			fp_seg_klen<<<g_m, 256, 0, P.st>>>(db, nn, m, eof ? 1 : 0, carry_ord, P.L.p, P.seg.p, P.ord2.p, P.klen.p, P.ctl.p);
			b = tb;
			FCK(rocprim::inclusive_scan(P.tmp.p, b, P.klen.p, P.lend.p, (size_t)m, rocprim::plus<uint32_t>(), P.st));
			fp_seg_loff<<<g_m, 256, 0, P.st>>>(m, P.seg.p, P.lend.p, P.ctl.p);
			fp_scatter<<<g_n, 256, 0, P.st>>>(db, nn, P.lid.p, P.seg.p, P.t.p, P.ctl.p);
			b = tb;
			FCK(rocprim::select(P.tmp.p, b, rocprim::counting_iterator<uint32_t>(0), P.hdr_flag.p, P.hseg.p, &P.ctl.p->n_hdr, (size_t)m, P.st));
			FCK(hipMemcpyAsync(P.h_ctl.p, P.ctl.p, sizeof(ctl_t), hipMemcpyDeviceToHost, P.st));
			FCK(hipStreamSynchronize(P.st));
			const uint32_t nk = P.h_ctl.p->n_kept;
			if (P.h_ctl.p->err & ERR_FASTQ) { bmh_set_error("index_fasta: %s has a '+' line: FASTQ references are not indexed", fa_path); rc = BMH_EINVAL; goto done; }
			if (P.h_ctl.p->err & ERR_BYTE) { bmh_set_error("index_fasta: %s has a sequence byte 0 or >= 128", fa_path); rc = BMH_EINVAL; goto done; }
			if (nk) {
				const uint64_t need = (P0 + nk + 3) / 4 + 64;
				if (need > P.pac_cap) {
					uint64_t nc = std::max(need, 2 * P.pac_cap);
					uint8_t *np = nullptr;
					FCK(hipMalloc((void **)&np, nc));
					FCK(hipMemsetAsync(np, 0, nc, P.st));
					FCK(hipMemcpyAsync(np, P.d_pac, P.pac_cap, hipMemcpyDeviceToDevice, P.st));
					FCK(hipStreamSynchronize(P.st));
					(void)hipFree(P.d_pac);
					P.d_pac = np; P.pac_cap = nc;
				}
				const uint32_t g_k = (nk + 255) / 256;
				fp_flags<<<g_k, 256, 0, P.st>>>(P.t.p, nk, carry_prev, P.amb.p, P.hole_flag.p, P.ctl.p);
				b = tb;
				FCK(rocprim::inclusive_scan(P.tmp.p, b, P.amb.p, P.arank.p, (size_t)nk, rocprim::plus<uint32_t>(), P.st));
				const uint64_t nq = ((P0 + nk - 1) >> 2) - (P0 >> 2) + 1;
				fp_pack<<<(uint32_t)((nq + 255) / 256), 256, 0, P.st>>>(P.t.p, P.arank.p, nk, P0, A0, P.d_pac);
				b = tb;
				FCK(rocprim::select(P.tmp.p, b, rocprim::counting_iterator<uint32_t>(0), P.hole_flag.p, P.hpos.p, &P.ctl.p->n_holes, (size_t)nk, P.st));
				FCK(hipMemcpyAsync(&P.ctl.p->n_amb, P.arank.p + nk - 1, 4, hipMemcpyDeviceToDevice, P.st));
			}
			FCK(hipMemcpyAsync(P.h_ctl.p, P.ctl.p, sizeof(ctl_t), hipMemcpyDeviceToHost, P.st));
			FCK(hipStreamSynchronize(P.st));
			{
				const ctl_t c = *P.h_ctl.p;
				const uint32_t nh = std::max(c.n_holes, c.n_hdr);
				if (nh) {
					// small tables (holes and headers are few): they grow with the largest count seen
					if (nh > P.h_hdrs.cap) {              // (the last of the four to grow)
						const size_t tab_cap = std::max<size_t>(nh, 2 * P.h_hdrs.cap);
						P.holes.drop(); P.hdrs.drop(); P.h_holes.drop(); P.h_hdrs.drop();
						FRC(P.holes.resize(tab_cap)); FRC(P.hdrs.resize(tab_cap));
						FRC(P.h_holes.resize(tab_cap)); FRC(P.h_hdrs.resize(tab_cap));
					}
					fp_gather<<<(nh + 255) / 256, 256, 0, P.st>>>(P.t.p, P.arank.p, P.hpos.p, P.seg.p, P.hseg.p, P.ctl.p, P0, A0, P.holes.p, P.hdrs.p);
					if (c.n_holes) FCK(hipMemcpyAsync(P.h_holes.p, P.holes.p, (size_t)c.n_holes * sizeof(hole_dev_t), hipMemcpyDeviceToHost, P.st));
					if (c.n_hdr) FCK(hipMemcpyAsync(P.h_hdrs.p, P.hdrs.p, (size_t)c.n_hdr * sizeof(hdr_dev_t), hipMemcpyDeviceToHost, P.st));
					FCK(hipStreamSynchronize(P.st));
				}
				S.pack_seconds += secs(t0);
				for (uint32_t h = 0; h < c.n_holes; ++h) { hole_off.push_back(P.h_holes.p[h].off); hole_rank.push_back(P.h_holes.p[h].rank); hole_ch.push_back((uint8_t)P.h_holes.p[h].ch); }
				// header text from the pinned chunk: an open one continues at the chunk's start
				const uint8_t *cb = hb + off;
				auto take = [&](uint32_t from) {
					const uint8_t *e = (const uint8_t *)memchr(cb + from, '\n', nn - from);
					const uint32_t to = e ? (uint32_t)(e - cb) : nn;
					hdr.text.append((const char *)cb + from, to - from);
					if (e) { recs.push_back(parse_header(hdr)); hdr_open = false; }
				};
				if (hdr_open) take(0);
				for (uint32_t h = 0; h < c.n_hdr; ++h) {
					hdr = header_t();
					hdr.offset = P0 + P.h_hdrs.p[h].loff;
					hdr_open = true;
					take(P.h_hdrs.p[h].start + 1);
				}
				if (m) { carry_kind = c.last_kind; carry_ord = c.last_ord; }
				if (nk) carry_prev = c.last_prev;
				l_pac += nk;
				n_amb += c.n_amb;
				at_ls = cb[nn - 1] == '\n';
			}
		}
		if (eof) break;
		{
			auto t0 = std::chrono::steady_clock::now();
			int64_t r = pending.get();
			S.read_seconds += secs(t0);
			if (r < 0) { bmh_set_error("index_fasta: read error in %s", fa_path); rc = BMH_EINVAL; goto done; }
			file_bytes += (uint64_t)r;
			hold = 1 + (size_t)r;
			eof = next_eof || (size_t)r < chunk_bytes;
			cur ^= 1;
		}
	}
	if (hdr_open) {
		// the file ends inside a header line; a '>' as the file's last byte makes no record (kseq_read returns -1)
		if (!hdr.text.empty()) recs.push_back(parse_header(hdr));
		hdr_open = false;
	}
	if (recs.empty()) { bmh_set_error("index_fasta: %s holds no FASTA record", fa_path); rc = BMH_EINVAL; goto done; }
	if (l_pac == 0) { bmh_set_error("index_fasta: every sequence of %s is empty", fa_path); rc = BMH_EINVAL; goto done; }
	if (l_pac >= ((uint64_t)1 << 32)) { bmh_set_error("index_fasta: %llu bases: the index builder takes fewer than 2^32", (unsigned long long)l_pac); rc = BMH_ECAPACITY; goto done; }
	{
		const size_t nr = recs.size(), nh = hole_off.size();
		out->n_contigs = (int32_t)nr;
		out->n_holes = (int64_t)nh;
		out->l_pac = l_pac;
		out->n_ambig = n_amb;
		size_t name_bytes = 0, comment_bytes = 0;
		for (auto &r : recs) { name_bytes += r.name.size() + 1; comment_bytes += r.comment.size() + 1; }
		out->names = (char *)malloc(name_bytes); out->comments = (char *)malloc(comment_bytes);
		out->name_off = (uint64_t *)malloc(nr * 8); out->comment_off = (uint64_t *)malloc(nr * 8);
		out->offsets = (int64_t *)malloc(nr * 8); out->lens = (int64_t *)malloc(nr * 8); out->n_ambs = (int32_t *)malloc(nr * 4);
		out->hole_off = (int64_t *)malloc(nh * 8 + 8); out->hole_len = (int64_t *)malloc(nh * 8 + 8); out->hole_char = (uint8_t *)malloc(nh + 1);
		if (!out->names || !out->comments || !out->name_off || !out->comment_off || !out->offsets || !out->lens || !out->n_ambs || !out->hole_off || !out->hole_len || !out->hole_char) {
			bmh_set_error("index_fasta: out of host memory"); rc = BMH_ENOMEM; goto done;
		}
		size_t pn = 0, pc = 0;
		for (size_t i = 0; i < nr; ++i) {
			const record_t &r = recs[i];
			out->name_off[i] = pn; memcpy(out->names + pn, r.name.c_str(), r.name.size() + 1); pn += r.name.size() + 1;
			out->comment_off[i] = pc; memcpy(out->comments + pc, r.comment.c_str(), r.comment.size() + 1); pc += r.comment.size() + 1;
			out->offsets[i] = (int64_t)r.offset;
			out->lens[i] = (int64_t)((i + 1 < nr ? recs[i + 1].offset : l_pac) - r.offset);
			out->n_ambs[i] = 0;
			if (out->lens[i] > INT32_MAX) { bmh_set_error("index_fasta: sequence %s is longer than 2^31 - 1 bases", r.name.c_str()); rc = BMH_ECAPACITY; goto done; }
		}
		size_t ci = 0;       // holes and contigs both ascend: the contig that holds a hole's first base
		for (size_t h = 0; h < nh; ++h) {
			out->hole_off[h] = (int64_t)hole_off[h];
			out->hole_len[h] = (int64_t)((h + 1 < nh ? hole_rank[h + 1] : n_amb) - hole_rank[h]);
			out->hole_char[h] = hole_ch[h];
			while (ci < nr && hole_off[h] >= (uint64_t)(out->offsets[ci] + out->lens[ci])) ++ci;
			if (ci == nr) { bmh_set_error("index_fasta: internal: hole at %llu outside every contig", (unsigned long long)hole_off[h]); rc = BMH_EINVAL; goto done; }
			++out->n_ambs[ci];
		}
		(void)file_bytes;
	}
	// the packer's buffers go before the index is built (the builder needs ~24 B of HBM per symbol)
	P.free_work();
	out->d_pac = P.d_pac;
	out->pac_bytes = P.pac_cap;
	P.d_pac = nullptr;
	S.n_contigs = (uint64_t)out->n_contigs; S.n_holes = (uint64_t)out->n_holes; S.l_pac = l_pac; S.n_ambig = n_amb;
	S.file_bytes = file_bytes;
done:
	if (pending.valid()) pending.wait();
	S.total_seconds = secs(t_all);
	if (stats) *stats = S;
	if (rc) bmh_fasta_packed_free(out);
	return rc;
}

extern "C" void bmh_fasta_packed_free(bmh_fasta_packed_t *p)
{
	if (!p) return;
	if (p->d_pac) (void)hipFree(p->d_pac);
	void *h[] = {p->names, p->comments, p->name_off, p->comment_off, p->offsets, p->lens, p->n_ambs, p->hole_off, p->hole_len, p->hole_char};
	for (void *x : h) free(x);
	memset(p, 0, sizeof(*p));
}

namespace {

bool write_all(FILE *f, const void *p, size_t n) { return fwrite(p, 1, n, f) == n; }

// .pac / .ann / .amb as bns_fasta2bntseq (forward only, bntseq.c:311-323) and bns_dump (:66-95) write them
int write_bns_files(const std::string &pfx, const bmh_fasta_packed_t *pk, const uint8_t *h_pac)
{
	const uint64_t l_pac = pk->l_pac;
	FILE *f = fopen((pfx + ".pac").c_str(), "wb");
	if (!f) return -1;
	bool ok = write_all(f, h_pac, (l_pac >> 2) + ((l_pac & 3) ? 1 : 0));
	uint8_t ct = 0;
	if (l_pac % 4 == 0) ok = ok && write_all(f, &ct, 1);
	ct = (uint8_t)(l_pac % 4);
	ok = ok && write_all(f, &ct, 1);
	ok = (fclose(f) == 0) && ok;
	if (!ok) return -1;
	f = fopen((pfx + ".ann").c_str(), "w");
	if (!f) return -1;
	fprintf(f, "%lld %d %u\n", (long long)l_pac, pk->n_contigs, 11u);
	for (int i = 0; i < pk->n_contigs; ++i) {
		const char *name = pk->names + pk->name_off[i], *cm = pk->comments + pk->comment_off[i];
		const char *anno = cm[0] ? cm : "(null)";
		fprintf(f, "0 %s", name);
		if (anno[0]) fprintf(f, " %s\n", anno); else fprintf(f, "\n");
		fprintf(f, "%lld %d %d\n", (long long)pk->offsets[i], (int)pk->lens[i], pk->n_ambs[i]);
	}
	ok = !ferror(f);
	ok = (fclose(f) == 0) && ok;
	if (!ok) return -1;
	f = fopen((pfx + ".amb").c_str(), "w");
	if (!f) return -1;
	fprintf(f, "%lld %d %u\n", (long long)l_pac, pk->n_contigs, (unsigned)pk->n_holes);
	for (int64_t h = 0; h < pk->n_holes; ++h) fprintf(f, "%lld %d %c\n", (long long)pk->hole_off[h], (int)pk->hole_len[h], pk->hole_char[h]);
	ok = !ferror(f);
	ok = (fclose(f) == 0) && ok;
	return ok ? 0 : -1;
}

// .bwt / .sa as fmindex.write_index writes them (the reference's files: bwtindex.c:174-197, bwt.c:472-487)
int write_bwt_sa(const std::string &pfx, uint64_t n, uint64_t primary, const uint64_t L2[5], int sa_intv,
                 const std::vector<uint32_t> &bwt, std::vector<uint32_t> &sa, std::vector<uint32_t> &bits)
{
	const uint64_t nblk = (n + 63) / 64, n16 = (n + 15) / 16, n_words_last = n16 - (nblk - 1) * 4;
	const uint64_t body = (nblk - 1) * 8 + 4 + n_words_last, n_sa = (n + sa_intv) / sa_intv;
	uint64_t hdr[5] = {primary, L2[1], L2[2], L2[3], L2[4]};
	uint32_t tot[4];
	for (int c = 0; c < 4; ++c) tot[c] = (uint32_t)(L2[c + 1] - L2[c]);
	FILE *f = fopen((pfx + ".bwt").c_str(), "wb");
	if (!f) return -1;
	bool ok = write_all(f, hdr, sizeof(hdr)) && write_all(f, bwt.data(), body * 4) && write_all(f, tot, sizeof(tot));
	ok = (fclose(f) == 0) && ok;
	if (!ok) return -1;
	const uint64_t nbits = n_sa / 32 + 1;
	if (n >> 32) {      // the high bit of every sample row below n_sa; the rest of the last word cleared
		const uint64_t tail = n_sa & 31;
		bits[n_sa / 32] &= tail ? (uint32_t)((1ull << tail) - 1) : 0u;
	} else {
		std::fill(bits.begin(), bits.end(), 0u);
	}
	uint64_t h2[7] = {primary, L2[1], L2[2], L2[3], L2[4], (uint64_t)sa_intv, n};
	uint8_t pack_size = 1;
	f = fopen((pfx + ".sa").c_str(), "wb");
	if (!f) return -1;
	ok = write_all(f, h2, sizeof(h2)) && write_all(f, sa.data() + 1, (n_sa - 1) * 4) && write_all(f, &pack_size, 1) && write_all(f, bits.data(), nbits * 4);
	ok = (fclose(f) == 0) && ok;
	return ok ? 0 : -1;
}

} // namespace

extern "C" int bmh_index_fasta(const char *fa_path, const char *prefix, int sa_intv, int flags, size_t chunk_bytes, bmh_index_fasta_stats_t *stats)
{
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { bmh_set_error("bmh_index_fasta: no HIP device"); return BMH_ENODEV; }
	if (!fa_path || !prefix) { bmh_set_error("bmh_index_fasta: NULL argument"); return BMH_EINVAL; }
	if (sa_intv <= 0 || (sa_intv & (sa_intv - 1))) { bmh_set_error("bmh_index_fasta: -r %d: the SA interval must be a power of two", sa_intv); return BMH_EINVAL; }
	const auto t_all = std::chrono::steady_clock::now();
	bmh_fasta_packed_t pk;
	bmh_index_fasta_stats_t S;
	memset(&S, 0, sizeof(S));
	int rc = bmh_fasta_pack(fa_path, chunk_bytes, &pk, &S);
	if (rc) { if (stats) *stats = S; return rc; }
	static const char *exts[5] = {".bwt", ".sa", ".pac", ".ann", ".amb"};
	const std::string pfx(prefix), tpfx = pfx + ".tmp" + std::to_string((long)getpid());
	const uint64_t l_pac = pk.l_pac, n = 2 * l_pac, nblk = (n + 63) / 64, n_sa = (n + sa_intv) / sa_intv;
	std::vector<uint32_t> bwt((nblk + 1) * 8), sa(n_sa), bits(n_sa / 32 + 1);
	std::vector<uint8_t> h_pac((l_pac + 3) / 4);
	uint32_t *d_bwt = nullptr, *d_sa = nullptr, *d_bits = nullptr;
	uint64_t primary = 0, L2[5] = {0, 0, 0, 0, 0};
	bmh_build_stats_t bs;
	auto t0 = std::chrono::steady_clock::now();
	hipError_t e = hipMemcpy(h_pac.data(), pk.d_pac, h_pac.size(), hipMemcpyDeviceToHost);
	if (e == hipSuccess) e = hipMalloc((void **)&d_bwt, bwt.size() * 4);
	if (e == hipSuccess) e = hipMalloc((void **)&d_sa, sa.size() * 4);
	if (e == hipSuccess) e = hipMalloc((void **)&d_bits, bits.size() * 4);
	if (e != hipSuccess) { bmh_set_error("bmh_index_fasta: %s", hipGetErrorString(e)); rc = BMH_ENODEV; goto out; }
	rc = bmh_index_build(pk.d_pac, l_pac, sa_intv, d_bwt, d_sa, d_bits, &primary, L2, flags & BMH_BUILD_VERIFY, &bs);
	if (rc) goto out;
	e = hipMemcpy(bwt.data(), d_bwt, bwt.size() * 4, hipMemcpyDeviceToHost);
	if (e == hipSuccess) e = hipMemcpy(sa.data(), d_sa, sa.size() * 4, hipMemcpyDeviceToHost);
	if (e == hipSuccess) e = hipMemcpy(bits.data(), d_bits, bits.size() * 4, hipMemcpyDeviceToHost);
	if (e != hipSuccess) { bmh_set_error("bmh_index_fasta: %s", hipGetErrorString(e)); rc = BMH_ENODEV; goto out; }
	S.build_seconds = secs(t0);
	S.verified = bs.verified;
	t0 = std::chrono::steady_clock::now();
	if (write_bwt_sa(tpfx, n, primary, L2, sa_intv, bwt, sa, bits) || write_bns_files(tpfx, &pk, h_pac.data())) {
		bmh_set_error("bmh_index_fasta: cannot write %s.*: %s", pfx.c_str(), strerror(errno));
		rc = BMH_EINVAL;
		goto out;
	}
	for (int i = 0; i < 5; ++i)
		if (rename((tpfx + exts[i]).c_str(), (pfx + exts[i]).c_str()) != 0) {
			bmh_set_error("bmh_index_fasta: cannot rename to %s%s: %s", pfx.c_str(), exts[i], strerror(errno));
			rc = BMH_EINVAL;
			goto out;
		}
	S.write_seconds = secs(t0);
out:
	if (rc) for (int i = 0; i < 5; ++i) unlink((tpfx + exts[i]).c_str());
	if (d_bwt) (void)hipFree(d_bwt);
	if (d_sa) (void)hipFree(d_sa);
	if (d_bits) (void)hipFree(d_bits);
	bmh_fasta_packed_free(&pk);
	S.total_seconds = secs(t_all);
	if (stats) *stats = S;
	return rc;
}
