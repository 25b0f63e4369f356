// The text of a read file, in order, whatever it is wrapped in (bmh_reads_load_files, bmh_aligner_run_files): a plain file or pipe, a gzip stream
// (recognised by its magic bytes 1f 8b, concatenated members read as one stream, as gzread does) or BGZF (gzip members of at most 64 KiB whose extra field
// "BC" carries the member's size: what bgzip and the sequencers' converters write) -- BGZF members are independent, so they are inflated on several host
// threads, in order; a plain gzip stream is one dependent bit stream and stays on one thread.  A BGZF file whose text begins with "BAM\1" holds BAM records, not
// text: it is recognised here from those bytes (peek_bam), never from the file's name, and the pump (csrc/reads_parse.hip) takes it as its third kind.  zlib is loaded at run time (dlopen("libz.so.1"), as
// csrc/fasta_pack.hip does): no link dependency, and a clear message when it is missing.  Nothing is mapped and nothing is sought: every form reads its
// descriptor front to back.
#include <dlfcn.h>
#include <errno.h>
#include <fcntl.h>
#include <unistd.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>
#include "bmh_internal.h"

namespace {

// zlib's z_stream (its layout is part of zlib's ABI: inflateInit2_ checks sizeof)
struct zs_t {
	const uint8_t *next_in; unsigned avail_in; unsigned long total_in;
	uint8_t *next_out; unsigned avail_out; unsigned long total_out;
	const char *msg; void *state; void *zalloc, *zfree, *opaque;
	int data_type; unsigned long adler, reserved;
};
typedef int (*inflate_init2_f)(zs_t *, int, const char *, int);
typedef int (*inflate_f)(zs_t *, int);
typedef int (*inflate_end_f)(zs_t *);
typedef unsigned long (*crc32_f)(unsigned long, const uint8_t *, unsigned);
typedef const char *(*zversion_f)(void);
enum { Z_OK_ = 0, Z_STREAM_END_ = 1, Z_BUF_ERROR_ = -5 };

struct zlib_t {
	void *h = nullptr;
	inflate_init2_f init2 = nullptr; inflate_f inflate = nullptr; inflate_end_f end = nullptr, reset = nullptr; crc32_f crc32 = nullptr; const char *ver = nullptr;
	~zlib_t() { if (h) dlclose(h); }
	bool load(const char *path)
	{
		h = dlopen("libz.so.1", RTLD_NOW | RTLD_LOCAL);
		if (!h) { bmh_set_error("reads file: %s is gzip-compressed and zlib (libz.so.1) could not be loaded: %s", path, dlerror()); return false; }
		init2 = (inflate_init2_f)dlsym(h, "inflateInit2_"); inflate = (inflate_f)dlsym(h, "inflate"); end = (inflate_end_f)dlsym(h, "inflateEnd");
		reset = (inflate_end_f)dlsym(h, "inflateReset"); crc32 = (crc32_f)dlsym(h, "crc32");
		zversion_f zv = (zversion_f)dlsym(h, "zlibVersion");
		if (!init2 || !inflate || !end || !reset || !crc32 || !zv) { bmh_set_error("reads file: libz.so.1 lacks inflateInit2_ / inflate / inflateEnd / inflateReset / crc32"); return false; }
		ver = zv();
		return true;
	}
};

enum { SRC_PLAIN = 0, SRC_GZIP = 1, SRC_BGZF = 2 };
constexpr size_t IN_CAP = 4u << 20;          // compressed bytes held (many BGZF members, or a piece of a gzip stream)
constexpr size_t BGZF_MAX = 65536;

// size of the BGZF member whose header starts at p: 0 if it is not one, (size_t)-1 if its header is not complete in the avail bytes; *data_off: where its deflate data begin
inline size_t bgzf_size(const uint8_t *p, size_t avail, size_t *data_off)
{
	if (avail < 12) return (size_t)-1;
	if (p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || !(p[3] & 4)) return 0;
	const size_t xlen = p[10] | ((size_t)p[11] << 8);
	if (avail < 12 + xlen) return (size_t)-1;
	for (size_t q = 12; q + 4 <= 12 + xlen;) {
		const size_t sl = p[q + 2] | ((size_t)p[q + 3] << 8);
		if (p[q] == 'B' && p[q + 1] == 'C' && sl == 2 && q + 6 <= 12 + xlen) { *data_off = 12 + xlen; return (size_t)(p[q + 4] | (p[q + 5] << 8)) + 1; }
		q += 4 + sl;
	}
	return 0;
}

}   // namespace

struct bmh_text_src_t {
	std::string path;
	int fd = -1, kind = SRC_PLAIN, n_threads = 1;
	std::vector<uint8_t> in; size_t in_pos = 0, in_len = 0; bool in_eof = false;
	zlib_t z; zs_t zs; bool zs_live = false, member_done = false, tail_ignored = false;
	// BGZF: the members inflated last, served in order
	std::vector<uint8_t> slots; std::vector<uint32_t> slot_len; size_t slot_cur = 0, slot_pos = 0;
	uint64_t n_host_members = 0;
	~bmh_text_src_t() { if (zs_live) z.end(&zs); if (fd >= 0) close(fd); }

	// more compressed bytes behind the ones not yet used (moved to the front); false at the end of the file
	bool refill(size_t enough = 65536 + 18)
	{
		if (in_pos) { memmove(in.data(), in.data() + in_pos, in_len - in_pos); in_len -= in_pos; in_pos = 0; }
		while (!in_eof && in_len < in.size()) {
			const ssize_t r = ::read(fd, in.data() + in_len, in.size() - in_len);
			if (r < 0) { if (errno == EINTR) continue; bmh_set_error("reads file: read error in %s: %s", path.c_str(), strerror(errno)); return false; }
			if (r == 0) { in_eof = true; break; }
			in_len += (size_t)r;
			if (in_len >= enough) break;                 // (a pipe gives what it has: read on until the next step has what it needs)
		}
		return true;
	}

	int64_t read_plain(uint8_t *dst, size_t n)
	{
		size_t done = 0;
		if (in_pos < in_len) { done = std::min(n, in_len - in_pos); memcpy(dst, in.data() + in_pos, done); in_pos += done; }
		while (done < n && !in_eof) {
			const ssize_t r = ::read(fd, dst + done, n - done);
			if (r < 0) { if (errno == EINTR) continue; bmh_set_error("reads file: read error in %s: %s", path.c_str(), strerror(errno)); return -1; }
			if (r == 0) { in_eof = true; break; }
			done += (size_t)r;
		}
		return (int64_t)done;
	}

	int64_t read_gzip(uint8_t *dst, size_t n)
	{
		size_t done = 0;
		while (done < n && !tail_ignored) {
			if (member_done && in_len - in_pos < 2 && !in_eof && !refill()) return -1;
			if (member_done && in_pos < in_len && (in_len - in_pos < 2 || in.data()[in_pos] != 0x1f || in.data()[in_pos + 1] != 0x8b)) {
				tail_ignored = true; break;             // bytes behind the last member that begin no member (padding): ignored, as gzread ignores them
			}
			if (in_pos == in_len) {
				if (!refill()) return -1;
				if (in_pos == in_len) {                     // the file has ended: fine between members, an error inside one
					if (member_done) break;
					bmh_set_error("reads file: %s: the gzip stream is truncated", path.c_str()); return -1;
				}
			}
			if (member_done) { z.reset(&zs); member_done = false; }      // a further member: the same stream
			zs.next_in = in.data() + in_pos; zs.avail_in = (unsigned)(in_len - in_pos);
			const size_t want = std::min(n - done, (size_t)1 << 30);
			zs.next_out = dst + done; zs.avail_out = (unsigned)want;
			const int rc = z.inflate(&zs, 0);
			in_pos = in_len - zs.avail_in; done += want - zs.avail_out;
			if (rc == Z_STREAM_END_) member_done = true;
			else if (rc != Z_OK_ && rc != Z_BUF_ERROR_) { bmh_set_error("reads file: %s: damaged gzip data (%s)", path.c_str(), zs.msg ? zs.msg : "inflate failed"); return -1; }
		}
		return (int64_t)done;
	}

	// inflates the next members (as many as are in `in`, at most 16 per thread) into the slots; false: error
	bool bgzf_round()
	{
		slot_len.clear(); slot_cur = slot_pos = 0;
		struct blk_t { size_t off, size, data; };
		std::vector<blk_t> blk;
		const size_t max_blk = (size_t)n_threads * 16;
		// (as many members as the buffer holds, from a pipe too: the round's threads need members to share)
		if (!in_eof && in_len - in_pos < in.size() / 2 && !refill(in.size())) return false;
		for (size_t p = in_pos; blk.size() < max_blk && p < in_len;) {
			size_t data = 0;
			const size_t bs = bgzf_size(in.data() + p, in_len - p, &data);
			if (bs == (size_t)-1) break;                                 // (its header is cut: the file is truncated, or the rest comes with the next round)
			if (bs == 0 || bs < data + 8) {
				if (!blk.empty()) break;
				bmh_set_error("reads file: %s: a gzip member without the BGZF size field behind BGZF members", path.c_str()); return false;
			}
			if (in_len - p < bs) break;
			blk.push_back({p, bs, data}); p += bs;
		}
		if (blk.empty()) {
			if (in_pos == in_len && in_eof) return true;                  // the end
			bmh_set_error("reads file: %s: the gzip stream is truncated", path.c_str()); return false;
		}
		slots.resize(blk.size() * BGZF_MAX); slot_len.assign(blk.size(), 0);
		const unsigned T = (unsigned)std::min<size_t>((size_t)n_threads, blk.size());
		std::vector<int> bad(T, 0);
		auto work = [&](unsigned t) {
			zs_t s; memset(&s, 0, sizeof(s));
			if (z.init2(&s, -15, z.ver, (int)sizeof(zs_t)) != Z_OK_) { bad[t] = 1; return; }
			for (size_t i = t; i < blk.size(); i += T) {
				const uint8_t *m = in.data() + blk[i].off;
				if (i != t) z.reset(&s);
				s.next_in = m + blk[i].data; s.avail_in = (unsigned)(blk[i].size - blk[i].data - 8);
				s.next_out = slots.data() + i * BGZF_MAX; s.avail_out = (unsigned)BGZF_MAX;
				const int rc = z.inflate(&s, 4 /* Z_FINISH */);
				const uint32_t got = (uint32_t)(BGZF_MAX - s.avail_out);
				const uint8_t *tr = m + blk[i].size - 8;
				const uint32_t crc = tr[0] | (tr[1] << 8) | (tr[2] << 16) | ((uint32_t)tr[3] << 24), isz = tr[4] | (tr[5] << 8) | (tr[6] << 16) | ((uint32_t)tr[7] << 24);
				if (rc != Z_STREAM_END_ || got != isz || (uint32_t)z.crc32(0, slots.data() + i * BGZF_MAX, got) != crc) { bad[t] = 1; break; }
				slot_len[i] = got;
			}
			z.end(&s);
		};
		if (T == 1) work(0);
		else { std::vector<std::thread> th; for (unsigned t = 0; t < T; ++t) th.emplace_back(work, t); for (auto &x : th) x.join(); }
		for (int b : bad) if (b) { bmh_set_error("reads file: %s: damaged BGZF member (inflate, length or CRC)", path.c_str()); return false; }
		in_pos = blk.back().off + blk.back().size;
		n_host_members += blk.size();
		return true;
	}

	// for the device inflate: the bytes not yet used and then the file's next bytes go to dst [cap] until the whole members at its front hold want_text bytes of
	// text (or the file ends, or dst is full); tab: those members, offsets into dst and into their text; returns the bytes they cover (the rest waits in `in` for
	// the next call: a member cut at the end of dst, or one more member than wanted), -1: refused.  cap >= the unused bytes + 1 MiB.
	int64_t members(uint8_t *dst, size_t cap, size_t want_text, std::vector<bmh_inflate_member_t> &tab, uint64_t *text, bool *end)
	{
		tab.clear(); *text = 0; *end = false;
		size_t n = in_len - in_pos, p = 0;
		if (n + (1u << 20) > cap) { bmh_set_error("reads file: %s: the buffer of compressed bytes is too small (%zu for %zu held)", path.c_str(), cap, n); return -1; }
		memcpy(dst, in.data() + in_pos, n); in_pos = in_len = 0;
		for (;;) {
			bool foreign = false;
			while (*text < want_text) {
				size_t data = 0;
				const size_t bs = bgzf_size(dst + p, n - p, &data);
				if (bs == (size_t)-1) break;                               // (its header is cut)
				if (bs == 0 || bs < data + 8) {
					if (!tab.empty() || p > 0) { foreign = true; break; }    // (refused by the next call: what lies before it is delivered first)
					bmh_set_error("reads file: %s: a gzip member without the BGZF size field behind BGZF members", path.c_str()); return -1;
				}
				if (n - p < bs) break;
				const uint8_t *tr = dst + p + bs - 8;
				bmh_inflate_member_t e;
				e.in_off = p + data; e.out_off = *text; e.in_len = (uint32_t)(bs - data - 8); e.reserved = 0;
				e.crc32 = tr[0] | (tr[1] << 8) | (tr[2] << 16) | ((uint32_t)tr[3] << 24); e.isize = tr[4] | (tr[5] << 8) | (tr[6] << 16) | ((uint32_t)tr[7] << 24);
				tab.push_back(e); *text += e.isize; p += bs;
			}
			if (foreign || *text >= want_text || n == cap) break;
			if (in_eof) {
				if (p < n && tab.empty()) { bmh_set_error("reads file: %s: the gzip stream is truncated", path.c_str()); return -1; }
				break;
			}
			// as many bytes as the text still wanted is likely to take, by the ratio seen so far
			const double ratio = *text ? (double)p / (double)*text : 0.3;
			const size_t guess = (size_t)((double)(want_text - *text) * ratio * 1.05) + (128u << 10);
			const size_t want = std::min(cap - n, guess > n - p ? guess - (n - p) : (size_t)65536);
			const ssize_t r = ::read(fd, dst + n, want);
			if (r < 0) { if (errno == EINTR) continue; bmh_set_error("reads file: read error in %s: %s", path.c_str(), strerror(errno)); return -1; }
			if (r == 0) in_eof = true; else n += (size_t)r;
		}
		if (p == 0 && n > 0 && !in_eof && n == cap) { bmh_set_error("reads file: %s: a BGZF member larger than the buffer of compressed bytes", path.c_str()); return -1; }
		if (n - p > in.size()) in.resize(n - p);
		memcpy(in.data(), dst + p, n - p); in_len = n - p;
		*end = in_eof && in_len == 0;
		return (int64_t)p;
	}

	// Does the text begin with "BAM\1"?  Looked at without taking a byte: the first members are inflated into a buffer of their own (BGZF), or the stream's first
	// bytes with a z_stream of its own (gzip).  0 no, 1 a BGZF file that does, 2 a plain gzip stream that does, -1 a read error.  A damaged first member is no
	// BAM here: the reader meets it again and words the refusal.
	int peek_bam()
	{
		uint8_t head[4]; size_t got = 0;
		if (kind == SRC_BGZF) {
			std::vector<uint8_t> tmp(BGZF_MAX);
			size_t rel = 0;
			for (int m = 0; got < 4 && m < 16; ++m) {                 // (empty members in front of the text are legal)
				if (in_len - in_pos - rel < BGZF_MAX + 18 && !in_eof && !refill(rel + 2 * (BGZF_MAX + 18))) return -1;
				const uint8_t *mp = in.data() + in_pos + rel;
				const size_t avail = in_len - in_pos - rel;
				size_t data = 0;
				const size_t bs = bgzf_size(mp, avail, &data);
				if (bs == (size_t)-1 || bs == 0 || bs < data + 8 || avail < bs) break;
				zs_t s; memset(&s, 0, sizeof(s));
				if (z.init2(&s, -15, z.ver, (int)sizeof(zs_t)) != Z_OK_) break;
				s.next_in = mp + data; s.avail_in = (unsigned)(bs - data - 8); s.next_out = tmp.data(); s.avail_out = (unsigned)BGZF_MAX;
				const int rc = z.inflate(&s, 4 /* Z_FINISH */);
				const size_t n = BGZF_MAX - s.avail_out;
				z.end(&s);
				if (rc != Z_STREAM_END_) break;
				for (size_t k = 0; k < n && got < 4; ++k) head[got++] = tmp[k];
				rel += bs;
			}
		} else if (kind == SRC_GZIP) {
			if (in_len - in_pos < 4096 && !in_eof && !refill(4096)) return -1;
			zs_t s; memset(&s, 0, sizeof(s));
			if (z.init2(&s, 15 + 16, z.ver, (int)sizeof(zs_t)) != Z_OK_) return 0;
			s.next_in = in.data() + in_pos; s.avail_in = (unsigned)(in_len - in_pos); s.next_out = head; s.avail_out = 4;
			(void)z.inflate(&s, 0);
			got = 4 - s.avail_out;
			z.end(&s);
		}
		return got == 4 && memcmp(head, "BAM\1", 4) == 0 ? (kind == SRC_BGZF ? 1 : 2) : 0;
	}

	int64_t read_bgzf(uint8_t *dst, size_t n)
	{
		size_t done = 0;
		while (done < n) {
			if (slot_cur == slot_len.size()) {
				if (!bgzf_round()) return -1;
				if (slot_len.empty()) break;
			}
			const size_t k = std::min(n - done, (size_t)slot_len[slot_cur] - slot_pos);
			memcpy(dst + done, slots.data() + slot_cur * BGZF_MAX + slot_pos, k);
			done += k; slot_pos += k;
			if (slot_pos == slot_len[slot_cur]) { ++slot_cur; slot_pos = 0; }
		}
		return (int64_t)done;
	}
};

bmh_text_src_t *bmh_text_open(const char *path, int n_threads)
{
	bmh_text_src_t *s = new bmh_text_src_t();
	s->path = path;
	s->n_threads = n_threads > 0 ? std::min(n_threads, 64) : std::max(1, bmh_effective_cpus());
	s->fd = open(path, O_RDONLY);
	if (s->fd < 0) { bmh_set_error("reads file: cannot open %s: %s", path, strerror(errno)); delete s; return nullptr; }
	s->in.resize(IN_CAP);
	while (s->in_len < 18 && !s->in_eof) {
		const ssize_t r = ::read(s->fd, s->in.data() + s->in_len, 18 - s->in_len);
		if (r < 0) { if (errno == EINTR) continue; bmh_set_error("reads file: read error in %s: %s", path, strerror(errno)); delete s; return nullptr; }
		if (r == 0) s->in_eof = true; else s->in_len += (size_t)r;
	}
	if (s->in_len >= 2 && s->in[0] == 0x1f && s->in[1] == 0x8b) {
		if (!s->z.load(path)) { delete s; return nullptr; }
		// BGZF or gzip: decided when the whole extra field of the first member is there
		size_t data = 0, bs = bgzf_size(s->in.data(), s->in_len, &data);
		if (bs == (size_t)-1 && !s->in_eof && s->refill(12 + 65536)) bs = bgzf_size(s->in.data(), s->in_len, &data);
		if (bs != 0 && bs != (size_t)-1) s->kind = SRC_BGZF;
		else {
			s->kind = SRC_GZIP;
			memset(&s->zs, 0, sizeof(s->zs));
			if (s->z.init2(&s->zs, 15 + 16, s->z.ver, (int)sizeof(zs_t)) != Z_OK_) { bmh_set_error("reads file: inflateInit2 failed (zlib %s)", s->z.ver); delete s; return nullptr; }
			s->zs_live = true;
		}
	}
	return s;
}

int64_t bmh_text_read(bmh_text_src_t *s, uint8_t *dst, size_t n)
{
	return s->kind == SRC_PLAIN ? s->read_plain(dst, n) : s->kind == SRC_GZIP ? s->read_gzip(dst, n) : s->read_bgzf(dst, n);
}

int bmh_text_kind(const bmh_text_src_t *s) { return s->kind; }
int bmh_text_bam(bmh_text_src_t *s) { return s->peek_bam(); }
size_t bmh_text_pending(const bmh_text_src_t *s) { return s->in_len - s->in_pos; }
uint64_t bmh_text_host_members(const bmh_text_src_t *s) { return s->n_host_members; }
int64_t bmh_text_members(bmh_text_src_t *s, uint8_t *dst, size_t cap, size_t want_text, std::vector<bmh_inflate_member_t> &tab, uint64_t *text_bytes, bool *end)
{
	return s->members(dst, cap, want_text, tab, text_bytes, end);
}

extern "C" int bmh_bgzf_scan(const uint8_t *data, uint64_t n_bytes, bmh_inflate_member_t *tab, uint64_t tab_cap, uint64_t *n_members, uint64_t *used, uint64_t *text_bytes)
{
	if ((!data && n_bytes) || !n_members || !used || !text_bytes) { bmh_set_error("bmh_bgzf_scan: null argument"); return BMH_EINVAL; }
	uint64_t nm = 0, p = 0, text = 0;
	while (p < n_bytes && (!tab || nm < tab_cap)) {
		size_t data_off = 0;
		const size_t bs = bgzf_size(data + p, (size_t)(n_bytes - p), &data_off);
		if (bs == (size_t)-1) break;
		if (bs == 0 || bs < data_off + 8) { bmh_set_error("bmh_bgzf_scan: the bytes at %llu begin no BGZF member (a gzip member with the size field BC)", (unsigned long long)p); return BMH_EINVAL; }
		if (n_bytes - p < bs) break;
		const uint8_t *tr = data + p + bs - 8;
		const uint32_t isize = tr[4] | (tr[5] << 8) | (tr[6] << 16) | ((uint32_t)tr[7] << 24);
		if (tab) {
			bmh_inflate_member_t &e = tab[nm];
			e.in_off = p + data_off; e.out_off = text; e.in_len = (uint32_t)(bs - data_off - 8); e.isize = isize; e.reserved = 0;
			e.crc32 = tr[0] | (tr[1] << 8) | (tr[2] << 16) | ((uint32_t)tr[3] << 24);
		}
		++nm; text += isize; p += bs;
	}
	*n_members = nm; *used = p; *text_bytes = text;
	return BMH_OK;
}
void bmh_text_close(bmh_text_src_t *s) { delete s; }
