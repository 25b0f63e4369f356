// One BGZF member written by one wave of 64 lanes: the compressor of csrc/deflate_kernels.hip and, compiled as plain C++ with a loop over the 64 "lanes" of
// every phase, of bmh_deflate_blocks_host and tests/deflate_core_host.cpp (under the sanitizers).  The same source runs in both places and gives the same bytes.
//
// A member: the 18-byte gzip header with the BC subfield (BSIZE = the member's bytes - 1), one deflate block, CRC32 and ISIZE.  Level 0: a stored block.
// Level 1: LZ77 tokens in a dynamic-Huffman block (BTYPE 2), or the stored block when that is not smaller -- so a member of a piece of at most 0xff00
// bytes has at most 0xff00 + 31 bytes and BSIZE fits 16 bits.
//
// LZ77, 64 positions a step: every lane hashes the four bytes at its position and looks the hash up in the position table AS IT WAS BEFORE THE STEP
// (so a candidate always lies before the step: no lane depends on another lane of its step), compares forward (at most 258 bytes, never past the piece's
// end) and keeps a match of 4 bytes or more at a distance of at most 32 768; then all 64 positions are inserted with an atomic maximum (the highest
// position wins a slot, whatever the order); then ONE lane walks the step left to right and picks the tokens greedily (a match where the lane at the
// position has one, else a literal).  A step that lies wholly inside a match is skipped (nothing is inserted).  The tokens are not stored: a first pass
// counts them (literal / length and distance histograms, atomic adds), one lane builds the code lengths (Moffat and Katajainen's in-place minimum-
// redundancy lengths on the symbols ranked by count, then the Kraft-sum repair that limits them to 15 bits; the code-length code to 7 bits, written
// without the run symbols 16-18), the exact size is compared with the stored form, and a second pass finds the same tokens again and writes their bits:
// the one lane's walk gives every token its bit offset (a running sum), every lane ORs its token's bits (at most 48) into the zeroed output words with
// atomic ORs -- commutative, so no result depends on which lane comes first.  The distance code always has two codes of one bit at least (as zlib writes
// it), so a block without matches, or with one distance, is a complete code for every inflater.
// CRC32: every lane takes a 64th of the piece with the byte table, one lane joins the 64 registers (crc(A B) = crc(A) x^(8 |B|) + crc(B) in GF(2)[x] / P).
//
// Shared state (LDS on the device): the position table of 8192 32-bit entries (32 KiB; 32-bit because the insert is an atomic maximum), the CRC table
// (1 KiB), histograms, codes and the step's arrays: about 38 KiB, four waves in a CU's 160 KiB.  The builder's scratch lies in the position table, which is
// cleared before the second pass anyway.
#pragma once
#include <stdint.h>
#include <string.h>
#include "inflate_core.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DFL_FN __host__ __device__ inline
#else
#define DFL_FN inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define DFL_LANES(lane) for (uint32_t lane = threadIdx.x, dfl_once_ = 1; dfl_once_; dfl_once_ = 0)
#define DFL_SYNC() __syncthreads()
#define DFL_MAX(p, v) ((void)atomicMax((p), (v)))
#define DFL_ADD(p, v) ((void)atomicAdd((p), (v)))
#define DFL_OR(p, v) ((void)atomicOr((p), (v)))
#else
#define DFL_LANES(lane) for (uint32_t lane = 0; lane < 64; ++lane)
#define DFL_SYNC() ((void)0)
#define DFL_MAX(p, v) do { if (*(p) < (v)) *(p) = (v); } while (0)
#define DFL_ADD(p, v) (*(p) += (v))
#define DFL_OR(p, v) (*(p) |= (v))
#endif
// (inside DFL_LANES only `continue` leaves a lane's turn: on the host a `break` would end the other lanes' too)

#define DFL_PIECE 0xff00u            // the bytes of a piece at most
#define DFL_HBITS 13
#define DFL_SLOT 65536u              // the device's output slot per member
#define DFL_MIN_MATCH 4u
#define DFL_MAX_MATCH 258u
#define DFL_MAX_DIST 32768u
#define DFL_NONE 0xffffffffu

// the bytes a member of n bytes needs at most (the stored form), rounded up to whole 32-bit words; the output is that many ZERO bytes, 4-byte aligned
DFL_FN uint32_t dfl_bound(uint32_t n) { return (n + 31u + 3u) & ~3u; }

struct dfl_state_t {
	uint32_t htab[1u << DFL_HBITS];
	uint32_t crc[256];
	uint32_t lfreq[288], dfreq[32], clfreq[20];
	uint32_t lcode[288], dcode[32], clcode[20];      // length << 16 | the code, bit-reversed (as it goes into the stream)
	uint8_t llen[288], dlen[32], cllen[20];
	uint32_t hh[64], off[64], nb[64], lanecrc[64];
	uint16_t mlen[64], mdist[64];
	uint64_t tokv[64];
	uint64_t starts;
	uint32_t extra, carry, bitpos, u0, u1;
};

DFL_FN uint32_t dfl_ld32(const uint8_t *p) { uint32_t v; memcpy(&v, p, 4); return v; }

// a x b mod P, reflected (bit 31 is x^0): zlib's multmodp
DFL_FN uint32_t dfl_mulmod(uint32_t a, uint32_t b)
{
	uint32_t m = 1u << 31, p = 0;
	for (;;) {
		if (a & m) { p ^= b; if ((a & (m - 1)) == 0) break; }
		m >>= 1;
		b = (b & 1u) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
	}
	return p;
}

DFL_FN void dfl_len_sym(uint32_t len, uint32_t *sym, uint32_t *eb, uint32_t *ev)
{
	if (len == 258) { *sym = 285; *eb = 0; *ev = 0; return; }
	const uint32_t l = len - 3;
	if (l < 8) { *sym = 257 + l; *eb = 0; *ev = 0; return; }
	const uint32_t e = (31u - (uint32_t)__builtin_clz(l)) - 2;
	*sym = 257 + 4 * (e + 1) + ((l >> e) & 3u); *eb = e; *ev = l & ((1u << e) - 1);
}

DFL_FN void dfl_dist_sym(uint32_t dist, uint32_t *sym, uint32_t *eb, uint32_t *ev)
{
	const uint32_t d = dist - 1;
	if (d < 4) { *sym = d; *eb = 0; *ev = 0; return; }
	const uint32_t e = (31u - (uint32_t)__builtin_clz(d)) - 1;
	*sym = 2 * (e + 1) + ((d >> e) & 1u); *eb = e; *ev = d & ((1u << e) - 1);
}

// v (at most 48 bits) ORed into the words at bit offset `at`
DFL_FN void dfl_or_bits(uint32_t *w, uint32_t at, uint64_t v)
{
	const uint32_t i = at >> 5, s = at & 31u;
	const uint64_t a = v << s;
	const uint32_t w0 = (uint32_t)a, w1 = (uint32_t)(a >> 32), w2 = s ? (uint32_t)(v >> (64 - s)) : 0u;
	if (w0) DFL_OR(w + i, w0);
	if (w1) DFL_OR(w + i + 1, w1);
	if (w2) DFL_OR(w + i + 2, w2);
}

// Code lengths of at most maxbits bits for the nsym counts freq[] (a symbol that does not occur gets 0; fewer than two that do: the first symbols that
// do not are built in as place-holders with a count of one, so that the code is complete -- freq[] itself stays what the tokens counted, and what the
// caller sizes the block from).  Scratch: sh.htab, sh.u0, sh.u1.  All lanes call it.
DFL_FN void dfl_build(dfl_state_t &sh, const uint32_t *freq, uint32_t nsym, uint32_t maxbits, uint8_t *len)
{
	uint32_t *key = sh.htab, *srt = sh.htab + 512, *A = sh.htab + 1024;
	DFL_LANES(lane) {
		if (lane != 0) continue;
		uint32_t used = 0, ph = 0xffffffffu;                                // the place-holders: two symbols of 16 bits, 0xffff for none
		for (uint32_t i = 0; i < nsym; ++i) used += freq[i] != 0;
		for (uint32_t i = 0; i < nsym && used < 2; ++i) if (!freq[i]) { ph = ph << 16 | i; ++used; }
		sh.u0 = used; sh.u1 = ph;
	}
	DFL_SYNC();
	DFL_LANES(lane) {
		const uint32_t ph = sh.u1;
		for (uint32_t i = lane; i < nsym; i += 64) {
			const uint32_t f = freq[i] ? freq[i] : (i == (ph & 0xffffu) || i == ph >> 16) ? 1u : 0u;
			key[i] = f ? (f << 9 | i) : DFL_NONE; len[i] = 0;
		}
	}
	DFL_SYNC();
	DFL_LANES(lane) {
		for (uint32_t i = lane; i < nsym; i += 64) {
			const uint32_t k = key[i];
			if (k == DFL_NONE) continue;
			uint32_t r = 0;
			for (uint32_t j = 0; j < nsym; ++j) r += key[j] < k;
			srt[r] = k;
		}
	}
	DFL_SYNC();
	DFL_LANES(lane) {
		if (lane != 0) continue;
		const int n = (int)sh.u0;
		for (int i = 0; i < n; ++i) A[i] = srt[i] >> 9;
		// minimum-redundancy code lengths in place (Moffat and Katajainen 1995): A ascending counts -> A depths (A[0] the deepest)
		if (n == 1) A[0] = 1;
		else {
			A[0] += A[1];
			int root = 0, leaf = 2, next;
			for (next = 1; next < n - 1; ++next) {
				if (leaf >= n || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = (uint32_t)next; } else A[next] = A[leaf++];
				if (leaf >= n || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = (uint32_t)next; } else A[next] += A[leaf++];
			}
			A[n - 2] = 0;
			for (next = n - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
			int avbl = 1, used = 0, dpth = 0;
			root = n - 2; next = n - 1;
			while (avbl > 0) {
				while (root >= 0 && (int)A[root] == dpth) { ++used; --root; }
				while (avbl > used) { A[next--] = (uint32_t)dpth; --avbl; }
				avbl = 2 * used; ++dpth; used = 0;
			}
		}
		// at most maxbits: the deeper codes move up to maxbits, then the Kraft sum is brought back to one (a code of maxbits leaves, the deepest shorter code splits)
		uint32_t num[33];
		for (int i = 0; i <= 32; ++i) num[i] = 0;
		for (int i = 0; i < n; ++i) ++num[A[i] > 32 ? 32 : A[i]];
		for (uint32_t i = maxbits + 1; i <= 32; ++i) { num[maxbits] += num[i]; num[i] = 0; }
		uint32_t total = 0;
		for (uint32_t i = maxbits; i > 0; --i) total += num[i] << (maxbits - i);
		while (total > (1u << maxbits)) {
			--num[maxbits];
			for (uint32_t i = maxbits - 1; i > 0; --i) if (num[i]) { --num[i]; num[i + 1] += 2; break; }
			--total;
		}
		int j = n;
		for (uint32_t l = 1; l <= maxbits; ++l) for (uint32_t k = num[l]; k > 0; --k) len[srt[--j] & 511u] = (uint8_t)l;
	}
	DFL_SYNC();
}

// canonical codes of the lengths (RFC 1951 3.2.2), bit-reversed; one lane
DFL_FN void dfl_codes(const uint8_t *len, uint32_t nsym, uint32_t *code)
{
	uint32_t cnt[16], next[16];
	for (int l = 0; l < 16; ++l) cnt[l] = 0;
	for (uint32_t i = 0; i < nsym; ++i) ++cnt[len[i]];
	cnt[0] = 0;
	uint32_t c = 0;
	for (int l = 1; l < 16; ++l) { c = (c + cnt[l - 1]) << 1; next[l] = c; }
	for (uint32_t i = 0; i < nsym; ++i) {
		const uint32_t l = len[i];
		if (!l) { code[i] = 0; continue; }
		const uint32_t v = next[l]++;
		uint32_t r = 0;
		for (uint32_t b = 0; b < l; ++b) r |= ((v >> b) & 1u) << (l - 1 - b);
		code[i] = l << 16 | r;
	}
}

// One pass over the piece: the tokens counted (EMIT false) or written from bit `bitpos` on (EMIT true; returns the bit behind the last token).  All lanes call it.
template <bool EMIT>
DFL_FN uint32_t dfl_pass(dfl_state_t &sh, const uint8_t *in, uint32_t n, uint32_t *out32, uint32_t bitpos)
{
	DFL_LANES(lane) {
		for (uint32_t i = lane; i < (1u << DFL_HBITS); i += 64) sh.htab[i] = 0;
		if (lane == 0) { sh.carry = 0; sh.bitpos = bitpos; }
	}
	DFL_SYNC();
	for (uint32_t b = 0; b < n; b += 64) {
		const uint32_t carry = sh.carry;
		if (carry >= 64) {                                                 // the step lies inside a match
			DFL_SYNC();
			DFL_LANES(lane) { if (lane == 0) sh.carry = carry - 64; }
			DFL_SYNC();
			continue;
		}
		DFL_LANES(lane) {
			const uint32_t p = b + lane;
			uint32_t h = DFL_NONE, ml = 0, md = 0;
			if (p + 4 <= n) {
				h = (dfl_ld32(in + p) * 2654435761u) >> (32 - DFL_HBITS);
				const uint32_t c = sh.htab[h];
				if (c && p - (c - 1) <= DFL_MAX_DIST) {
					const uint32_t cand = c - 1, maxl = n - p < DFL_MAX_MATCH ? n - p : DFL_MAX_MATCH;
					uint32_t k = 0;
					while (k + 4 <= maxl && dfl_ld32(in + cand + k) == dfl_ld32(in + p + k)) k += 4;
					while (k < maxl && in[cand + k] == in[p + k]) ++k;
					if (k >= DFL_MIN_MATCH) { ml = k; md = p - cand; }
				}
			}
			sh.hh[lane] = h; sh.mlen[lane] = (uint16_t)ml; sh.mdist[lane] = (uint16_t)(md - 1);
			if (EMIT && p < n) {
				uint64_t v; uint32_t nb;
				if (ml) {
					uint32_t ls, le, lv, ds, de, dv;
					dfl_len_sym(ml, &ls, &le, &lv); dfl_dist_sym(md, &ds, &de, &dv);
					const uint32_t lc = sh.lcode[ls], dc = sh.dcode[ds];
					v = lc & 0xffffu; nb = lc >> 16;
					v |= (uint64_t)lv << nb; nb += le;
					v |= (uint64_t)(dc & 0xffffu) << nb; nb += dc >> 16;
					v |= (uint64_t)dv << nb; nb += de;
				} else { const uint32_t lc = sh.lcode[in[p]]; v = lc & 0xffffu; nb = lc >> 16; }
				sh.tokv[lane] = v; sh.nb[lane] = nb;
			}
		}
		DFL_SYNC();
		DFL_LANES(lane) {
			const uint32_t h = sh.hh[lane];
			if (h != DFL_NONE) DFL_MAX(&sh.htab[h], b + lane + 1);
			if (lane == 0) {                                                // the greedy walk
				const uint32_t lim = n - b < 64 ? n - b : 64;
				uint32_t q = carry, bp = sh.bitpos; uint64_t st = 0;
				while (q < lim) {
					st |= 1ull << q;
					if (EMIT) { sh.off[q] = bp; bp += sh.nb[q]; }
					q += sh.mlen[q] ? sh.mlen[q] : 1u;
				}
				sh.starts = st; sh.carry = q >= 64 ? q - 64 : 0; sh.bitpos = bp;
			}
		}
		DFL_SYNC();
		DFL_LANES(lane) {
			if (!((sh.starts >> lane) & 1ull)) continue;
			if (EMIT) dfl_or_bits(out32, sh.off[lane], sh.tokv[lane]);
			else {
				const uint32_t ml = sh.mlen[lane];
				if (ml) {
					uint32_t ls, le, lv, ds, de, dv;
					dfl_len_sym(ml, &ls, &le, &lv); dfl_dist_sym((uint32_t)sh.mdist[lane] + 1, &ds, &de, &dv);
					DFL_ADD(&sh.lfreq[ls], 1u); DFL_ADD(&sh.dfreq[ds], 1u); DFL_ADD(&sh.extra, le + de);
				} else DFL_ADD(&sh.lfreq[in[b + lane]], 1u);
			}
		}
		DFL_SYNC();
	}
	return sh.bitpos;
}

// The member of the piece in[0, n), 1 <= n <= DFL_PIECE, at level 0 or 1 -> out32[0, dfl_bound(n) / 4), which the caller has zeroed.  Returns its bytes.
// All 64 lanes of the wave call it (the host: once).
DFL_FN uint32_t dfl_member(dfl_state_t &sh, const uint8_t *in, uint32_t n, uint32_t *out32, int level)
{
	uint8_t *out = (uint8_t *)out32;
	// ---- CRC32
	const uint32_t C = (n + 63) / 64;
	DFL_LANES(lane) { for (uint32_t i = lane; i < 256; i += 64) sh.crc[i] = inf_crc_entry(i); }
	DFL_SYNC();
	DFL_LANES(lane) {
		const uint32_t a = lane * C < n ? lane * C : n, e = a + C < n ? a + C : n;
		uint32_t r = 0;
		for (uint32_t k = a; k < e; ++k) r = sh.crc[(r ^ in[k]) & 0xffu] ^ (r >> 8);
		sh.lanecrc[lane] = r;
	}
	DFL_SYNC();
	DFL_LANES(lane) {
		if (lane != 0) continue;
		uint32_t xc = 1u << 31, xl = 1u << 31, total = 0xffffffffu;
		const uint32_t full = n / C, last = n - full * C;                  // `full` parts of C bytes, then one of `last` (or none)
		for (uint32_t k = 0; k < C; ++k) xc = sh.crc[xc & 0xffu] ^ (xc >> 8);
		for (uint32_t k = 0; k < last; ++k) xl = sh.crc[xl & 0xffu] ^ (xl >> 8);
		for (uint32_t l = 0; l < full; ++l) total = dfl_mulmod(xc, total) ^ sh.lanecrc[l];
		if (last) total = dfl_mulmod(xl, total) ^ sh.lanecrc[full];
		sh.u1 = total ^ 0xffffffffu;
	}
	DFL_SYNC();
	const uint32_t crc = sh.u1;
	// ---- level 1: count, build, size
	bool dynamic = false;
	uint32_t nlen = 257, ndist = 1, ncode = 4;
	if (level >= 1) {
		DFL_LANES(lane) {
			for (uint32_t i = lane; i < 288; i += 64) sh.lfreq[i] = 0;
			if (lane < 32) sh.dfreq[lane] = 0;
			if (lane < 20) sh.clfreq[lane] = 0;
			if (lane == 0) sh.extra = 0;
		}
		DFL_SYNC();
		dfl_pass<false>(sh, in, n, out32, 0);
		DFL_LANES(lane) { if (lane == 0) sh.lfreq[256] = 1; }
		DFL_SYNC();
		// (the builder leaves the counts as they are: the block is sized below from what the tokens cost, without the builder's place-holders)
		dfl_build(sh, sh.lfreq, 286, 15, sh.llen);
		dfl_build(sh, sh.dfreq, 30, 15, sh.dlen);
		DFL_LANES(lane) {
			if (lane != 0) continue;
			uint32_t nl = 286, nd = 30;
			while (nl > 257 && !sh.llen[nl - 1]) --nl;
			while (nd > 1 && !sh.dlen[nd - 1]) --nd;
			for (uint32_t i = 0; i < nl; ++i) ++sh.clfreq[sh.llen[i]];
			for (uint32_t i = 0; i < nd; ++i) ++sh.clfreq[sh.dlen[i]];
			sh.u0 = nl; sh.u1 = nd;
		}
		DFL_SYNC();
		nlen = sh.u0; ndist = sh.u1;
		DFL_SYNC();
		dfl_build(sh, sh.clfreq, 16, 7, sh.cllen);
		DFL_LANES(lane) {
			if (lane != 0) continue;
			sh.cllen[16] = sh.cllen[17] = sh.cllen[18] = 0;
			dfl_codes(sh.llen, 286, sh.lcode); dfl_codes(sh.dlen, 30, sh.dcode); dfl_codes(sh.cllen, 19, sh.clcode);
			uint32_t nc = 19;
			while (nc > 4) { const uint32_t i = nc - 1, ord = i < 3 ? 16 + i : i == 3 ? 0u : (i & 1u) ? 8u - (i - 3) / 2 : 8u + (i - 4) / 2; if (sh.cllen[ord]) break; --nc; }
			uint32_t bits = 3 + 14 + 3 * nc + sh.extra;
			for (uint32_t i = 0; i < nlen; ++i) bits += sh.cllen[sh.llen[i]] + sh.lfreq[i] * sh.llen[i];
			for (uint32_t i = 0; i < ndist; ++i) bits += sh.cllen[sh.dlen[i]] + sh.dfreq[i] * sh.dlen[i];
			sh.u0 = nc; sh.u1 = bits;                                       // (u1 keeps the bits to the end of the call: the trace of tests/deflate_core_host.cpp reads them)
		}
		DFL_SYNC();
		ncode = sh.u0;
		dynamic = 18 + (sh.u1 + 7) / 8 + 8 < n + 31;
		DFL_SYNC();
	}
	// ---- the gzip header's first 16 bytes: whole words of their own
	DFL_LANES(lane) {
		if (lane != 0) continue;
		out32[0] = 0x04088b1fu; out32[1] = 0; out32[2] = 0x0006ff00u; out32[3] = 0x00024342u;
	}
	uint32_t total;
	if (!dynamic) {
		total = n + 31;
		DFL_LANES(lane) {
			if (lane == 0) {
				out[16] = (uint8_t)(total - 1); out[17] = (uint8_t)((total - 1) >> 8);
				out[18] = 1; out[19] = (uint8_t)n; out[20] = (uint8_t)(n >> 8); out[21] = (uint8_t)~n; out[22] = (uint8_t)(~n >> 8);
				uint8_t *t = out + 23 + n;
				for (int k = 0; k < 4; ++k) { t[k] = (uint8_t)(crc >> (8 * k)); t[4 + k] = (uint8_t)(n >> (8 * k)); }
			}
			for (uint32_t k = lane; k < n; k += 64) out[23 + k] = in[k];
		}
		DFL_SYNC();
		return total;
	}
	// ---- the dynamic block: its header by one lane, the tokens by all, the end-of-block code and the trailer
	DFL_LANES(lane) {
		if (lane != 0) continue;
		uint32_t at = 144;
		dfl_or_bits(out32, at, 1u | 2u << 1 | (uint64_t)(nlen - 257) << 3 | (uint64_t)(ndist - 1) << 8 | (uint64_t)(ncode - 4) << 13); at += 17;
		for (uint32_t i = 0; i < ncode; ++i) {
			const uint32_t ord = i < 3 ? 16 + i : i == 3 ? 0u : (i & 1u) ? 8u - (i - 3) / 2 : 8u + (i - 4) / 2;
			dfl_or_bits(out32, at, sh.cllen[ord]); at += 3;
		}
		for (uint32_t i = 0; i < nlen + ndist; ++i) {
			const uint32_t c = sh.clcode[i < nlen ? sh.llen[i] : sh.dlen[i - nlen]];
			dfl_or_bits(out32, at, c & 0xffffu); at += c >> 16;
		}
		sh.u0 = at;
	}
	DFL_SYNC();
	const uint32_t at0 = sh.u0;
	DFL_SYNC();
	const uint32_t at1 = dfl_pass<true>(sh, in, n, out32, at0);
	const uint32_t eob = sh.lcode[256], end = at1 + (eob >> 16), tb = (end + 7) / 8;
	total = tb + 8;
	DFL_LANES(lane) {
		if (lane != 0) continue;
		dfl_or_bits(out32, at1, eob & 0xffffu);
		dfl_or_bits(out32, 128, (uint64_t)(total - 1));
		dfl_or_bits(out32, 8 * tb, (uint64_t)crc);
		dfl_or_bits(out32, 8 * tb + 32, (uint64_t)n);
	}
	DFL_SYNC();
	return total;
}
