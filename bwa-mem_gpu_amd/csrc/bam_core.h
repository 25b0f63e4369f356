// One SAM record line -> one BAM record (SAM spec section 4.2, little-endian), by one thread: the per-record logic of csrc/bam_kernels.hip (one lane per
// record, a sizes pass and a write pass) and, compiled as plain C++, of bmh_sam_to_bam_host and tests/bam_core_host.cpp (under the sanitizers).
//
//   block_size refID pos l_read_name mapq bin n_cigar_op flag l_seq next_refID next_pos tlen | read_name\0 | cigar | seq | qual | tags
//
// RNAME / RNEXT go through the contig name table ('*': -1, '=': the record's refID, a name that is not in the table: refused); POS / PNEXT are stored
// minus 1; CIGAR operations are len << 4 | op with op's place in "MIDNSHP=X" ('*': none); SEQ is packed two bases a byte with the table
// "=ACMGRSVTWYHKDBN" (either letter case, any other letter N), the high nibble first, a trailing nibble 0 ('*': l_seq 0); QUAL is stored minus 33 ('*':
// l_seq bytes 0xFF).
// bin = reg2bin(pos, end), both 0-based, end exclusive: end = pos + the CIGAR's reference length (M, D, N, =, X), or pos + 1 when that length is 0 or
// flag 0x4 is set; a record without a position (pos -1) gets 4680 -- what htslib computes (bam_reg2bin(-1, 0): 4681 + (-1 >> 14)).
// Tags XX:T:value -- A: one byte; Z, H: the bytes and a NUL; i: the smallest type in htslib's order (negative: c, s, i; else C, S, I; outside
// [-2^31, 2^32): refused); f: [-+]?digits[.digits] with at most 15 digits, stored as (float)((double)N / 10^k) -- N < 10^15 and 10^k are exact doubles
// and the division rounds once, so this is (float)strtod(), what htslib stores; any other spelling is refused; B is refused.
//
// The same function sizes (out == NULL) and writes, so the two passes cannot disagree about a record; the writer refuses byte `cap` anyway.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BAM_FN __host__ __device__ inline
#else
#define BAM_FN inline
#endif

enum {
	BAM_OK = 0,
	BAM_EFIELDS = 1,     // fewer than 11 fields
	BAM_ENAME = 2,       // an empty read name, or one longer than 254 bytes
	BAM_ECIGAR = 3,      // a CIGAR that is not (number, one of MIDNSHP=X)*, a length of 2^28 or more, more than 65 535 operations
	BAM_ETAG = 4,        // a tag that is not XX:T:value with T one of A i f Z H (an A value that is not one byte)
	BAM_ESEQQUAL = 5,    // SEQ and QUAL of different lengths
	BAM_ENOEOL = 6,      // the last line has no '\n'
	BAM_ERNAME = 7,      // RNAME or RNEXT is not in the contig table
	BAM_ENUMBER = 8,     // FLAG, POS, MAPQ, PNEXT or TLEN is no number of its range
	BAM_EINT = 9,        // an integer tag that is no integer, or outside [-2^31, 2^32)
	BAM_EFLOAT = 10,     // a float tag spelled otherwise than [-+]?digits[.digits] with at most 15 digits
	BAM_EBARRAY = 11,    // a B (array) tag
	BAM_ESIZE = 12       // the write pass and the sizes pass disagree (internal), or a line of 2^31 bytes or more
};

// the contig names: NUL-terminated, back to back; off [n + 1]
struct bam_refs_t { const char *names; const uint32_t *off; int n; };

struct bam_out_t {
	uint8_t *p; uint32_t n, cap;
	BAM_FN void u8(uint32_t b) { if (p && n < cap) p[n] = (uint8_t)b; ++n; }
	BAM_FN void u16(uint32_t v) { u8(v & 0xffu); u8((v >> 8) & 0xffu); }
	BAM_FN void u32(uint32_t v) { u16(v & 0xffffu); u16(v >> 16); }
};

// [-+]?digits, at most 18 of them; false: no such number
BAM_FN bool bam_int(const uint8_t *s, uint32_t a, uint32_t b, int64_t *v)
{
	bool neg = false;
	if (a < b && (s[a] == '-' || s[a] == '+')) { neg = s[a] == '-'; ++a; }
	if (a >= b || b - a > 18) return false;
	int64_t x = 0;
	for (; a < b; ++a) { if (s[a] < '0' || s[a] > '9') return false; x = x * 10 + (s[a] - '0'); }
	*v = neg ? -x : x;
	return true;
}

// the index of the name s[a, b) in the table; -1 for "*"; -2: not there
BAM_FN int bam_ref(const bam_refs_t &R, const uint8_t *s, uint32_t a, uint32_t b)
{
	const uint32_t l = b - a;
	if (l == 1 && s[a] == '*') return -1;
	for (int c = 0; c < R.n; ++c) {
		if (R.off[c + 1] - R.off[c] != l + 1) continue;
		const char *nm = R.names + R.off[c];
		uint32_t k = 0;
		while (k < l && (uint8_t)nm[k] == s[a + k]) ++k;
		if (k == l) return c;
	}
	return -2;
}

BAM_FN uint32_t bam_reg2bin(int64_t beg, int64_t end)
{
	--end;
	if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14)) & 0xffffu;
	if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17)) & 0xffffu;
	if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20)) & 0xffffu;
	if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23)) & 0xffffu;
	if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26)) & 0xffffu;
	return 0;
}

BAM_FN int bam_cigar_op(uint32_t c)
{
	switch (c) { case 'M': return 0; case 'I': return 1; case 'D': return 2; case 'N': return 3; case 'S': return 4; case 'H': return 5; case 'P': return 6; case '=': return 7; case 'X': return 8; }
	return -1;
}

BAM_FN uint32_t bam_nt16(uint32_t c)
{
	if (c >= 'a' && c <= 'z') c -= 32;
	switch (c) {
	case '=': return 0; case 'A': return 1; case 'C': return 2; case 'M': return 3; case 'G': return 4; case 'R': return 5; case 'S': return 6; case 'V': return 7;
	case 'T': return 8; case 'W': return 9; case 'Y': return 10; case 'H': return 11; case 'K': return 12; case 'D': return 13; case 'B': return 14;
	}
	return 15;
}

// the value of the float tag s[a, b) as the bits of a float; false: not [-+]?digits[.digits] with at most 15 digits
BAM_FN bool bam_float(const uint8_t *s, uint32_t a, uint32_t b, uint32_t *bits)
{
	bool neg = false;
	if (a < b && (s[a] == '-' || s[a] == '+')) { neg = s[a] == '-'; ++a; }
	uint64_t N = 0; uint32_t nd = 0, k = 0, ni = 0; bool dot = false;
	for (; a < b; ++a) {
		if (s[a] == '.') { if (dot || ni == 0) return false; dot = true; continue; }
		if (s[a] < '0' || s[a] > '9') return false;
		N = N * 10 + (uint64_t)(s[a] - '0');
		if (++nd > 15) return false;
		if (dot) ++k; else ++ni;
	}
	if (ni == 0 || (dot && k == 0)) return false;
	double p = 1.0;
	for (uint32_t i = 0; i < k; ++i) p *= 10.0;
	double d = (double)N / p;
	if (neg) d = -d;
	const float f = (float)d;
	memcpy(bits, &f, 4);
	return true;
}

// The record of the line s[0, n) (without its '\n'): sized (out == NULL) or written into out[0, cap); *size: its bytes, block_size included.
// Returns BAM_OK or the check that refused it (*size is then meaningless and the bytes written, all inside out[0, cap), are to be ignored).
BAM_FN uint32_t bam_record(const uint8_t *s, uint32_t n, const bam_refs_t &R, uint8_t *out, uint32_t cap, uint32_t *size)
{
	*size = 0;
	uint32_t fs[12], nt = 0;
	fs[0] = 0;
	for (uint32_t i = 0; i < n && nt < 11; ++i) if (s[i] == '\t') fs[++nt] = i + 1;
	if (nt < 10) return BAM_EFIELDS;
	const bool has_tags = nt == 11;
	if (!has_tags) fs[11] = n + 1;
#define BAM_F(i) fs[i], fs[(i) + 1] - 1
	const uint32_t l_name = fs[1] - 1 - fs[0];
	if (l_name < 1 || l_name > 254) return BAM_ENAME;
	int64_t flag, pos, mapq, pnext, tlen;
	if (!bam_int(s, BAM_F(1), &flag) || flag < 0 || flag > 65535) return BAM_ENUMBER;
	if (!bam_int(s, BAM_F(3), &pos) || pos < 0 || pos > 0x7fffffffll) return BAM_ENUMBER;
	if (!bam_int(s, BAM_F(4), &mapq) || mapq < 0 || mapq > 255) return BAM_ENUMBER;
	if (!bam_int(s, BAM_F(7), &pnext) || pnext < 0 || pnext > 0x7fffffffll) return BAM_ENUMBER;
	if (!bam_int(s, BAM_F(8), &tlen) || tlen < -0x80000000ll || tlen > 0x7fffffffll) return BAM_ENUMBER;
	const int ref = bam_ref(R, s, BAM_F(2));
	if (ref == -2) return BAM_ERNAME;
	int nref;
	if (fs[7] - 1 - fs[6] == 1 && s[fs[6]] == '=') nref = ref;
	else { nref = bam_ref(R, s, BAM_F(6)); if (nref == -2) return BAM_ERNAME; }
	// CIGAR: its operations counted, its reference length
	const uint32_t c0 = fs[5], c1 = fs[6] - 1;
	uint32_t n_ops = 0; int64_t rlen = 0;
	if (!(c1 - c0 == 1 && s[c0] == '*')) {
		uint32_t num = 0, nd = 0;
		for (uint32_t i = c0; i < c1; ++i) {
			const uint32_t c = s[i];
			if (c >= '0' && c <= '9') { num = num * 10 + (c - '0'); if (++nd > 9 || num >= (1u << 28)) return BAM_ECIGAR; continue; }
			const int op = bam_cigar_op(c);
			if (op < 0 || nd == 0) return BAM_ECIGAR;
			if (++n_ops > 65535) return BAM_ECIGAR;
			if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rlen += num;
			num = 0; nd = 0;
		}
		if (nd || n_ops == 0) return BAM_ECIGAR;
	}
	const uint32_t q0 = fs[9], q1 = fs[10] - 1, u0 = fs[10], u1 = fs[11] - 1;
	const bool no_seq = q1 - q0 == 1 && s[q0] == '*', no_qual = u1 - u0 == 1 && s[u0] == '*';
	const uint32_t l_seq = no_seq ? 0 : q1 - q0;
	if (q1 == q0 || u1 == u0) return BAM_ESEQQUAL;
	if (!no_qual && (no_seq || u1 - u0 != l_seq)) return BAM_ESEQQUAL;
	uint32_t bin = 4680;
	if (pos > 0) { const int64_t beg = pos - 1; bin = bam_reg2bin(beg, ((flag & 4) || rlen == 0) ? beg + 1 : beg + rlen); }
	bam_out_t o; o.p = out; o.n = 0; o.cap = cap;
	o.u32(0);                                                         // block_size: known at the end
	o.u32((uint32_t)ref); o.u32((uint32_t)(pos - 1));
	o.u8(l_name + 1); o.u8((uint32_t)mapq); o.u16(bin); o.u16(n_ops); o.u16((uint32_t)flag);
	o.u32(l_seq); o.u32((uint32_t)nref); o.u32((uint32_t)(pnext - 1)); o.u32((uint32_t)(int32_t)tlen);
	for (uint32_t i = 0; i < l_name; ++i) o.u8(s[fs[0] + i]);
	o.u8(0);
	if (n_ops) {
		uint32_t num = 0;
		for (uint32_t i = c0; i < c1; ++i) {
			const uint32_t c = s[i];
			if (c >= '0' && c <= '9') { num = num * 10 + (c - '0'); continue; }
			o.u32(num << 4 | (uint32_t)bam_cigar_op(c));
			num = 0;
		}
	}
	for (uint32_t i = 0; i < l_seq; i += 2) o.u8(bam_nt16(s[q0 + i]) << 4 | (i + 1 < l_seq ? bam_nt16(s[q0 + i + 1]) : 0u));
	for (uint32_t i = 0; i < l_seq; ++i) o.u8(no_qual ? 0xffu : (uint32_t)(s[u0 + i] - 33) & 0xffu);
	if (has_tags) {
		uint32_t t = fs[11];
		for (;;) {
			uint32_t e = t;
			while (e < n && s[e] != '\t') ++e;
			if (e - t < 5 || s[t + 2] != ':' || s[t + 4] != ':') return BAM_ETAG;
			const uint32_t ty = s[t + 3], v0 = t + 5;
			if (ty == 'B') return BAM_EBARRAY;
			if (ty != 'A' && ty != 'i' && ty != 'f' && ty != 'Z' && ty != 'H') return BAM_ETAG;
			o.u8(s[t]); o.u8(s[t + 1]);
			if (ty == 'A') {
				if (e - v0 != 1) return BAM_ETAG;
				o.u8('A'); o.u8(s[v0]);
			} else if (ty == 'Z' || ty == 'H') {
				o.u8(ty);
				for (uint32_t i = v0; i < e; ++i) o.u8(s[i]);
				o.u8(0);
			} else if (ty == 'i') {
				int64_t v;
				if (!bam_int(s, v0, e, &v) || v < -0x80000000ll || v > 0xffffffffll) return BAM_EINT;
				if (v < 0) {
					if (v >= -128) { o.u8('c'); o.u8((uint32_t)v & 0xffu); }
					else if (v >= -32768) { o.u8('s'); o.u16((uint32_t)v & 0xffffu); }
					else { o.u8('i'); o.u32((uint32_t)v); }
				} else {
					if (v <= 255) { o.u8('C'); o.u8((uint32_t)v); }
					else if (v <= 65535) { o.u8('S'); o.u16((uint32_t)v); }
					else { o.u8('I'); o.u32((uint32_t)v); }
				}
			} else {
				uint32_t bits;
				if (!bam_float(s, v0, e, &bits)) return BAM_EFLOAT;
				o.u8('f'); o.u32(bits);
			}
			if (e >= n) break;
			t = e + 1;
		}
	}
#undef BAM_F
	if (out && o.n <= cap) { const uint32_t bs = o.n - 4; out[0] = (uint8_t)bs; out[1] = (uint8_t)(bs >> 8); out[2] = (uint8_t)(bs >> 16); out[3] = (uint8_t)(bs >> 24); }
	*size = o.n;
	return BAM_OK;
}
