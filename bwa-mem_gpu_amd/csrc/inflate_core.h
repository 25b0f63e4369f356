// One DEFLATE stream (RFC 1951) inflated by one thread: the decoder of csrc/inflate_kernels.hip (one lane per BGZF member) and, compiled as plain
// C++, of bmh_bgzf_inflate's host mode and of tests/inflate_core_host.cpp (under the sanitizers).  The same source runs in both places.
//
// It cannot read or write out of bounds whatever the bytes are: the bit reader delivers zeros behind in[in_len) and the member then ends with
// INF_ETRUNC; every output byte goes through put(), which refuses byte `cap`; every distance is compared with the bytes produced so far; the
// code-length sets are checked the way zlib's inflate_table checks them (over-subscribed: refused; incomplete: refused unless it is a single
// one-bit code, whose unused half then decodes to no symbol), so what zlib takes is taken and gives the same bytes.
//
// Symbol decoding: a 9-bit lookup table for the literal / length codes of up to 9 bits, the canonical walk (count per length, symbols sorted by
// code: Mark Adler's puff restated) for longer ones and for the distance codes.  The tables live where WS puts them: the kernel keeps the
// lookup table, the counts and the distance symbols in LDS and the rest in the lane's private memory; the host build uses plain arrays.
//   WS: uint16_t &fast(i) [512], &lcnt(i) [16], &dcnt(i) [16], &dsym(i) [32], &lsym(i) [288]; uint8_t &len(i) [320]; uint32_t crc_tab(i) [256]
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define INF_FN __host__ __device__ __forceinline__
#else
#define INF_FN inline
#endif

enum {
	INF_OK = 0,
	INF_EBTYPE = 1,      // block type 3
	INF_ESTORED = 2,     // a stored block whose LEN and NLEN disagree
	INF_ECODES = 3,      // an over-subscribed or incomplete code-length set, a repeat without a length before it or beyond the set, no end-of-block code
	INF_ESYMBOL = 4,     // a bit pattern that is no code, or a length / distance symbol outside the alphabet (286, 287; 30, 31)
	INF_EDIST = 5,       // a distance beyond the start of the member's output
	INF_ETRUNC = 6,      // the deflate bytes end before the last block does
	INF_ESIZE = 7,       // more or fewer bytes than ISIZE (or an ISIZE above 65536)
	INF_ECRC = 8,        // the CRC32 of the bytes produced is not the trailer's
	INF_ETABLE = 9       // the member table points outside the buffers (device entry point)
};
#define INF_FAST_BITS 9
#define INF_MAX_OUT 65536u

// CRC-32 (IEEE 802.3, reflected, as zlib's crc32): entry i of the byte table
INF_FN uint32_t inf_crc_entry(uint32_t i)
{
	uint32_t c = i;
	for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
	return c;
}

struct inf_bits_t {
	const uint8_t *in; uint32_t len, pos; uint64_t buf; uint32_t cnt;
	INF_FN void init(const uint8_t *p, uint32_t n) { in = p; len = n; pos = 0; buf = 0; cnt = 0; }
	INF_FN void refill() { while (cnt <= 56) { const uint64_t b = pos < len ? in[pos] : 0u; ++pos; buf |= b << cnt; cnt += 8; } }
	INF_FN uint32_t peek(uint32_t n) const { return (uint32_t)(buf & ((1ull << n) - 1)); }
	INF_FN void drop(uint32_t n) { buf >>= n; cnt -= n; }
	// n <= 32 bits; the caller has refilled (a refill holds at least 57)
	INF_FN uint32_t take(uint32_t n) { const uint32_t v = peek(n); drop(n); return v; }
	// bits taken so far lie beyond the member's bytes
	INF_FN bool over() const { return (uint64_t)pos * 8 - cnt > (uint64_t)len * 8; }
};

struct inf_out_t {
	uint8_t *out; uint32_t n, cap, crc;
};

// counts, sorted symbols of the lengths len(base .. base + n); 0 or INF_ECODES by zlib's rules (lit: the literal / length set, which needs its end-of-block code)
template <class WS, bool LIT>
INF_FN int inf_build(WS &ws, uint32_t base, uint32_t n)
{
	uint16_t offs[16];
	for (int l = 0; l < 16; ++l) { if (LIT) ws.lcnt(l) = 0; else ws.dcnt(l) = 0; }
	for (uint32_t s = 0; s < n; ++s) { const uint32_t l = ws.len(base + s); if (LIT) ++ws.lcnt(l); else ++ws.dcnt(l); }
	int left = 1; uint32_t maxl = 0;
	for (int l = 1; l < 16; ++l) {
		const int c = LIT ? ws.lcnt(l) : ws.dcnt(l);
		left = (left << 1) - c;
		if (left < 0) return INF_ECODES;                                 // over-subscribed
		if (c) maxl = (uint32_t)l;
	}
	if (left > 0 && maxl > 1) return INF_ECODES;                          // incomplete (a single one-bit code, or no code at all, is taken as zlib takes it)
	if (LIT && ws.len(base + 256) == 0) return INF_ECODES;                // no end-of-block code
	offs[1] = 0;
	for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + (LIT ? ws.lcnt(l) : ws.dcnt(l)));
	for (uint32_t s = 0; s < n; ++s) {
		const uint32_t l = ws.len(base + s);
		if (l) { if (LIT) ws.lsym(offs[l]++) = (uint16_t)s; else ws.dsym(offs[l]++) = (uint16_t)s; }
	}
	if (LIT) {
		for (uint32_t i = 0; i < (1u << INF_FAST_BITS); ++i) ws.fast(i) = 0;
		uint32_t code = 0, idx = 0;
		for (uint32_t l = 1; l <= INF_FAST_BITS; ++l) {
			const uint32_t c = ws.lcnt(l);
			for (uint32_t k = 0; k < c; ++k, ++idx, ++code) {
				uint32_t r = 0;
				for (uint32_t b = 0; b < l; ++b) r |= ((code >> b) & 1u) << (l - 1 - b);
				const uint16_t e = (uint16_t)((ws.lsym(idx) << 4) | l);
				for (uint32_t j = r; j < (1u << INF_FAST_BITS); j += 1u << l) ws.fast(j) = e;
			}
			code <<= 1;
		}
	}
	return INF_OK;
}

// the canonical walk: the symbol of the code at the front of the bits (taken), or -1 when the bits are no code
template <class WS, bool LIT>
INF_FN int inf_walk(WS &ws, inf_bits_t &br)
{
	int code = 0, first = 0, index = 0;
	uint64_t b = br.buf;
	for (int l = 1; l <= 15; ++l) {
		code |= (int)(b & 1u); b >>= 1;
		const int c = LIT ? ws.lcnt(l) : ws.dcnt(l);
		if (code - c < first) { br.drop((uint32_t)l); return LIT ? ws.lsym(index + (code - first)) : ws.dsym(index + (code - first)); }
		index += c; first += c; first <<= 1; code <<= 1;
	}
	return -1;
}

template <class WS>
INF_FN bool inf_put(WS &ws, inf_out_t &o, uint32_t b)
{
	if (o.n >= o.cap) return false;
	o.out[o.n++] = (uint8_t)b;
	o.crc = ws.crc_tab((o.crc ^ b) & 0xffu) ^ (o.crc >> 8);
	return true;
}

// the dynamic block's header: code lengths into len(0 .. nlen + ndist)
template <class WS>
INF_FN int inf_dynamic_header(WS &ws, inf_bits_t &br, uint32_t *nlen_, uint32_t *ndist_)
{
	br.refill();
	const uint32_t nlen = br.take(5) + 257, ndist = br.take(5) + 1, ncode = br.take(4) + 4;
	if (nlen > 286 || ndist > 30) return INF_ECODES;
	// the code-length code: its 19 lengths arrive in this order; decoded through the distance slots of WS (19 symbols fit its 32)
	for (uint32_t i = 0; i < 19; ++i) ws.len(i) = 0;
	for (uint32_t i = 0; i < ncode; ++i) {
		const uint32_t ord = i < 3 ? 16 + i : i == 3 ? 0u : (i & 1u) ? 8u - (i - 3) / 2 : 8u + (i - 4) / 2;      // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
		br.refill();
		ws.len(ord) = (uint8_t)br.take(3);
	}
	{
		for (int l = 0; l < 16; ++l) ws.dcnt(l) = 0;
		for (uint32_t s = 0; s < 19; ++s) ++ws.dcnt(ws.len(s));
		int left = 1;
		for (int l = 1; l < 16; ++l) { left = (left << 1) - (int)ws.dcnt(l); if (left < 0) return INF_ECODES; }
		if (left > 0) return INF_ECODES;                                  // the code-length code must be complete
		uint16_t offs[16]; offs[1] = 0;
		for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + ws.dcnt(l));
		for (uint32_t s = 0; s < 19; ++s) { const uint32_t l = ws.len(s); if (l) ws.dsym(offs[l]++) = (uint16_t)s; }
	}
	uint32_t i = 0, prev = 0;
	while (i < nlen + ndist) {
		br.refill();
		const int sym = inf_walk<WS, false>(ws, br);
		if (sym < 0) return INF_ECODES;
		if (br.over()) return INF_ETRUNC;
		if (sym < 16) { ws.len(i++) = (uint8_t)sym; prev = (uint32_t)sym; continue; }
		uint32_t rep, val = 0;
		if (sym == 16) { if (i == 0) return INF_ECODES; val = prev; rep = 3 + br.take(2); }
		else if (sym == 17) rep = 3 + br.take(3);
		else rep = 11 + br.take(7);
		if (i + rep > nlen + ndist) return INF_ECODES;
		while (rep--) ws.len(i++) = (uint8_t)val;
		prev = val;
	}
	*nlen_ = nlen; *ndist_ = ndist;
	return INF_OK;
}

// literals, lengths and distances up to the end-of-block code
template <class WS>
INF_FN int inf_codes(WS &ws, inf_bits_t &br, inf_out_t &o)
{
	for (;;) {
		br.refill();
		int sym;
		const uint32_t e = ws.fast(br.peek(INF_FAST_BITS));
		if (e) { br.drop(e & 15u); sym = (int)(e >> 4); }
		else { sym = inf_walk<WS, true>(ws, br); if (sym < 0) return br.over() ? INF_ETRUNC : INF_ESYMBOL; }
		if (br.over()) return INF_ETRUNC;
		if (sym < 256) { if (!inf_put(ws, o, (uint32_t)sym)) return INF_ESIZE; continue; }
		if (sym == 256) return INF_OK;
		if (sym > 285) return INF_ESYMBOL;
		// length: symbols 257..264 are 3..10, then groups of four with 1..5 extra bits, 285 is 258
		uint32_t s = (uint32_t)sym - 257, length;
		if (s < 8) length = 3 + s;
		else if (s == 28) length = 258;
		else { const uint32_t eb = (s >> 2) - 1; length = 3 + ((4 + (s & 3u)) << eb) + br.take(eb); }
		const int ds = inf_walk<WS, false>(ws, br);                      // (a refill's 57 bits cover 15 + 5 + 15 + 13)
		if (ds < 0) return br.over() ? INF_ETRUNC : INF_ESYMBOL;
		if (ds > 29) return INF_ESYMBOL;
		uint32_t dist;
		if (ds < 4) dist = 1 + (uint32_t)ds;
		else { const uint32_t eb = ((uint32_t)ds >> 1) - 1; dist = 1 + ((2 + ((uint32_t)ds & 1u)) << eb) + br.take(eb); }
		if (br.over()) return INF_ETRUNC;
		if (dist > o.n) return INF_EDIST;
		if (length > o.cap - o.n) return INF_ESIZE;
		// byte by byte: an overlapping copy (dist < length) replicates the pattern
		for (uint32_t k = 0; k < length; ++k) inf_put(ws, o, o.out[o.n - dist]);
	}
}

// One member: in[0 .. in_len) inflated to out[0 .. min(isize, 65536)); *n_out: the bytes produced.  Returns INF_OK or the check that failed.
template <class WS>
INF_FN int inf_member(WS &ws, const uint8_t *in, uint32_t in_len, uint8_t *out, uint32_t isize, uint32_t crc_want, uint32_t *n_out)
{
	inf_bits_t br; br.init(in, in_len);
	inf_out_t o; o.out = out; o.n = 0; o.cap = isize < INF_MAX_OUT ? isize : INF_MAX_OUT; o.crc = 0xffffffffu;
	int rc = INF_OK;
	for (;;) {
		br.refill();
		const uint32_t last = br.take(1), type = br.take(2);
		if (br.over()) { rc = INF_ETRUNC; break; }
		if (type == 0) {
			br.drop(br.cnt & 7u);                                           // to the byte boundary
			br.refill();
			const uint32_t len = br.take(16), nlen = br.take(16);
			if (br.over()) { rc = INF_ETRUNC; break; }
			if ((len ^ 0xffffu) != nlen) { rc = INF_ESTORED; break; }
			// the bits held are whole bytes now: hand them back and copy from the input
			uint32_t p = br.pos - br.cnt / 8;
			if (len > in_len - p) { rc = INF_ETRUNC; break; }
			if (len > o.cap - o.n) { rc = INF_ESIZE; break; }
			for (uint32_t k = 0; k < len; ++k) inf_put(ws, o, in[p + k]);
			br.pos = p + len; br.buf = 0; br.cnt = 0;
		} else if (type == 1 || type == 2) {
			uint32_t nlen = 288, ndist = 30;
			if (type == 1) {
				for (uint32_t s = 0; s < 288; ++s) ws.len(s) = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
				for (uint32_t s = 0; s < 32; ++s) ws.len(288 + s) = 5;         // (30 and 31 have codes and are refused where they are used)
				ndist = 32;
			} else if ((rc = inf_dynamic_header(ws, br, &nlen, &ndist)) != INF_OK) break;
			if ((rc = inf_build<WS, true>(ws, 0, nlen)) != INF_OK) break;
			if ((rc = inf_build<WS, false>(ws, nlen, ndist)) != INF_OK) break;
			if ((rc = inf_codes(ws, br, o)) != INF_OK) break;
		} else { rc = INF_EBTYPE; break; }
		if (last) break;
	}
	*n_out = o.n;
	if (rc != INF_OK) return rc;
	if (isize > INF_MAX_OUT || o.n != isize) return INF_ESIZE;
	if ((o.crc ^ 0xffffffffu) != crc_want) return INF_ECRC;
	return INF_OK;
}

// plain arrays: the host's tables
struct inf_host_ws_t {
	uint16_t fast_[1 << INF_FAST_BITS], lcnt_[16], dcnt_[16], dsym_[32], lsym_[288]; uint8_t len_[320]; uint32_t crc_[256];
	inf_host_ws_t() { for (uint32_t i = 0; i < 256; ++i) crc_[i] = inf_crc_entry(i); }
	uint16_t &fast(uint32_t i) { return fast_[i]; }
	uint16_t &lcnt(uint32_t i) { return lcnt_[i]; }
	uint16_t &dcnt(uint32_t i) { return dcnt_[i]; }
	uint16_t &dsym(uint32_t i) { return dsym_[i]; }
	uint16_t &lsym(uint32_t i) { return lsym_[i]; }
	uint8_t &len(uint32_t i) { return len_[i]; }
	uint32_t crc_tab(uint32_t i) const { return crc_[i]; }
};
