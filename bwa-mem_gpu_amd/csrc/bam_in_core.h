// One BAM record -> one read (SAM spec section 4.2, little-endian), the other way round from csrc/bam_core.h: the per-record logic of csrc/bam_in_kernels.hip
// and, compiled as plain C++, of the host form (csrc/reads_io.cpp: bmh_bam_host_run) and tests/bam_in_core_host.cpp (under the sanitizers).
//
//   block_size refID pos l_read_name mapq bin n_cigar_op flag l_seq next_refID next_pos tlen | read_name\0 | cigar | seq | qual | tags
//
// The caller knows that the record r[0, size) -- size = 4 + block_size -- lies inside its window (the chain of record starts is walked on the host); every
// check below bounds a field by `size` BEFORE it is read, fields are read byte by byte (records have no alignment), and nothing is written but through
// bi_out_t, which refuses byte `cap`.  The rules are those of `samtools fastq`: records with flag 0x100 or 0x800 give no read; flag 0x10 gives the read back
// in sequencing orientation (bases complemented and reversed, qualities reversed); qualities all 0xff are none.
// Tags become the comment -C copies: XX:T:value fields joined by tabs in file order -- A as it is, c C s S i I as i, Z and H copied; f and B are left out
// (and counted), and so are the tags the aligner writes itself or that describe the old alignment (NM MD AS XS SA XA pa RG MC MQ).
// The same function sizes (out.p == NULL) and writes the comment, so the two passes cannot disagree.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BI_FN __host__ __device__ inline
#else
#define BI_FN inline
#endif

enum {
	BI_OK = 0,
	BI_ESIZE = 1,        // block_size is too small for the record's own fields
	BI_ENAME0 = 2,       // l_read_name is 0
	BI_ENUL = 3,         // the name's last byte is not NUL
	BI_ETAGEXT = 4,      // a tag runs past the end of the record
	BI_ETAGTYPE = 5,     // a tag of unknown type (or a B array of unknown element type)
	BI_ELSEQ0 = 6,       // a read without bases (l_seq 0) -- kept records only
	BI_EQUAL = 7,        // a quality above 93 -- kept records only
	// a run that keeps the input's read groups (bi_read_group) -- kept records only
	BI_ERGNONE = 8,      // no RG tag
	BI_ERGTYPE = 9,      // an RG tag of a type other than Z
	BI_ERGUNKNOWN = 10   // RG:Z names an ID the header's @RG lines do not hold
};

BI_FN const char *bi_status_text(int st)
{
	switch (st) {
	case BI_ESIZE: return "block_size is too small for the record's own fields";
	case BI_ENAME0: return "l_read_name is 0";
	case BI_ENUL: return "the read name does not end with NUL";
	case BI_ETAGEXT: return "a tag runs past the end of the record";
	case BI_ETAGTYPE: return "a tag of unknown type";
	case BI_ELSEQ0: return "a read without bases (l_seq 0)";
	case BI_EQUAL: return "a base quality above 93";
	case BI_ERGNONE: return "no RG tag (the run keeps the input's read groups)";
	case BI_ERGTYPE: return "an RG tag of a type other than Z";
	case BI_ERGUNKNOWN: return "its RG:Z names a read group the header's @RG lines do not hold";
	}
	return "ok";
}

BI_FN uint32_t bi_u16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
BI_FN uint32_t bi_u32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// offsets from the record's first byte; l_name counts the NUL
struct bi_rec_t { uint32_t flag, l_seq, l_name, seq_off, qual_off, tag_off, size; };

enum { BI_NAME_OFF = 36, BI_SKIP_FLAGS = 0x900 };

// nibble -> letter ("=ACMGRSVTWYHKDBN" as two 64-bit words: no table in memory, the same on the host and the device)
BI_FN uint8_t bi_letter(uint32_t nib)
{
	const uint64_t lo = 0x565352474d43413dull /* = A C M G R S V */, hi = 0x4e42444b48595754ull /* T W Y H K D B N */;
	return (uint8_t)(((nib & 8u) ? hi : lo) >> (8u * (nib & 7u)));
}
// samtools' complement (seq_comp_table): the nibble's four bits reversed -- = N S W stay, A<->T C<->G M<->K R<->Y V<->B H<->D
BI_FN uint32_t bi_comp(uint32_t n) { return ((n & 1u) << 3) | ((n & 2u) << 1) | ((n & 4u) >> 1) | ((n & 8u) >> 3); }
// nst_nt4_table of the letters above: A 0, C 1, G 2, T 3, everything else 4
BI_FN uint8_t bi_nt4(uint8_t c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4; }

// base i of the read in sequencing orientation
BI_FN uint8_t bi_base(const uint8_t *r, const bi_rec_t &R, uint32_t i)
{
	const bool rev = (R.flag & 0x10u) != 0;
	const uint32_t j = rev ? R.l_seq - 1 - i : i;
	const uint32_t nib = (r[R.seq_off + (j >> 1)] >> ((~j & 1u) << 2)) & 15u;
	return bi_letter(rev ? bi_comp(nib) : nib);
}
// its quality, Phred + 33 (only for a record that has qualities)
BI_FN uint8_t bi_qual(const uint8_t *r, const bi_rec_t &R, uint32_t i)
{
	return (uint8_t)(r[R.qual_off + ((R.flag & 0x10u) ? R.l_seq - 1 - i : i)] + 33u);
}

// the tag at r[p ..): its bytes (BI_OK) or why it is refused; size: the record's
BI_FN int bi_tag_size(const uint8_t *r, uint32_t size, uint32_t p, uint32_t *bytes)
{
	if (size - p < 3) return BI_ETAGEXT;
	const uint32_t left = size - p - 3;
	uint32_t v;
	switch (r[p + 2]) {
	case 'A': case 'c': case 'C': v = 1; break;
	case 's': case 'S': v = 2; break;
	case 'i': case 'I': case 'f': v = 4; break;
	case 'Z': case 'H': {
		uint32_t k = 0;
		while (k < left && r[p + 3 + k] != 0) ++k;
		if (k == left) return BI_ETAGEXT;
		v = k + 1;
		break;
	}
	case 'B': {
		if (left < 5) return BI_ETAGEXT;
		uint32_t es;
		switch (r[p + 3]) {
		case 'c': case 'C': es = 1; break;
		case 's': case 'S': es = 2; break;
		case 'i': case 'I': case 'f': es = 4; break;
		default: return BI_ETAGTYPE;
		}
		const uint64_t b = 5 + (uint64_t)es * bi_u32(r + p + 4);
		if (b > left) return BI_ETAGEXT;
		v = (uint32_t)b;
		break;
	}
	default: return BI_ETAGTYPE;
	}
	if (v > left) return BI_ETAGEXT;
	*bytes = 3 + v;
	return BI_OK;
}

// the checks every record passes, kept or skipped: BI_OK and *o, or the check that refused it
BI_FN int bi_check(const uint8_t *r, uint32_t size, bi_rec_t *o)
{
	if (size < 36) return BI_ESIZE;                        // (block_size < 32: the fixed fields themselves are not there)
	const uint32_t l_name = r[12], n_cig = bi_u16(r + 16), l_seq = bi_u32(r + 20);
	const uint64_t need = 36 + (uint64_t)l_name + 4 * (uint64_t)n_cig + ((uint64_t)l_seq + 1) / 2 + (uint64_t)l_seq;
	if (need > size) return BI_ESIZE;
	if (l_name == 0) return BI_ENAME0;
	if (r[BI_NAME_OFF + l_name - 1] != 0) return BI_ENUL;
	o->flag = bi_u16(r + 18); o->l_seq = l_seq; o->l_name = l_name; o->size = size;
	o->seq_off = BI_NAME_OFF + l_name + 4 * n_cig; o->qual_off = o->seq_off + (l_seq + 1) / 2; o->tag_off = o->qual_off + l_seq;
	for (uint32_t p = o->tag_off; p < size;) {
		uint32_t b;
		const int st = bi_tag_size(r, size, p, &b);
		if (st != BI_OK) return st;
		p += b;
	}
	return BI_OK;
}

// what a kept record must satisfy beyond bi_check; *has_qual: 0 when its qualities are all 0xff
BI_FN int bi_check_kept(const uint8_t *r, const bi_rec_t &R, uint32_t *has_qual)
{
	if (R.l_seq == 0) return BI_ELSEQ0;
	uint32_t n_ff = 0, top = 0;
	for (uint32_t i = 0; i < R.l_seq; ++i) { const uint32_t q = r[R.qual_off + i]; if (q == 0xffu) ++n_ff; else if (q > top) top = q; }
	*has_qual = n_ff != R.l_seq;
	if (*has_qual && (n_ff != 0 || top > 93)) return BI_EQUAL;
	return BI_OK;
}

// The read groups a run keeps: the IDs back to back (no terminators) with offsets off [n + 1] -- the shape of bdp_groups_t (csrc/bam_dup_core.h).
struct bi_groups_t { const uint8_t *ids; const uint32_t *off; uint32_t n; };

// The read group of a record that passed bi_check: the first RG tag among its tags, its Z value looked up in G row by row, whole IDs compared ("a" is not "ab").
// BI_OK and *group, or BI_ERGNONE / BI_ERGTYPE / BI_ERGUNKNOWN.  The tags are walked with bi_tag_size inside [tag_off, size), so B arrays and every other type are
// stepped over by their own extent; the value's NUL lies inside the record (bi_tag_size found it).
BI_FN int bi_read_group(const uint8_t *r, const bi_rec_t &R, const bi_groups_t &G, uint32_t *group)
{
	for (uint32_t p = R.tag_off; p < R.size;) {
		uint32_t b;
		if (bi_tag_size(r, R.size, p, &b) != BI_OK) break;          // (not reached: bi_check walked the same tags)
		if (r[p] == 'R' && r[p + 1] == 'G') {
			if (r[p + 2] != 'Z') return BI_ERGTYPE;
			const uint8_t *v = r + p + 3;
			const uint32_t len = b - 4;                             // (3 bytes of name and type, the value, its NUL)
			for (uint32_t g = 0; g < G.n; ++g) {
				const uint32_t o = G.off[g];
				if (G.off[g + 1] - o != len) continue;
				uint32_t k = 0;
				while (k < len && G.ids[o + k] == v[k]) ++k;
				if (k == len) { *group = g; return BI_OK; }
			}
			return BI_ERGUNKNOWN;
		}
		p += b;
	}
	return BI_ERGNONE;
}

struct bi_out_t {
	uint8_t *p; uint32_t n, cap;
	BI_FN void u8(uint32_t b) { if (p && n < cap) p[n] = (uint8_t)b; ++n; }
};

BI_FN bool bi_tag_dropped_name(uint32_t a, uint32_t b)
{
	const uint32_t t = a << 8 | b;
	return t == ('N' << 8 | 'M') || t == ('M' << 8 | 'D') || t == ('A' << 8 | 'S') || t == ('X' << 8 | 'S') || t == ('S' << 8 | 'A') || t == ('X' << 8 | 'A') ||
	       t == ('p' << 8 | 'a') || t == ('R' << 8 | 'G') || t == ('M' << 8 | 'C') || t == ('M' << 8 | 'Q');
}

// The comment of a record that passed bi_check, without its NUL: sized (out == NULL) or written to out[0, cap).  Returns its bytes; *n_left_out: its f and B tags.
BI_FN uint32_t bi_comment(const uint8_t *r, const bi_rec_t &R, uint8_t *out, uint32_t cap, uint32_t *n_left_out)
{
	bi_out_t o; o.p = out; o.n = 0; o.cap = cap;
	uint32_t left_out = 0;
	for (uint32_t p = R.tag_off; p < R.size;) {
		uint32_t b;
		if (bi_tag_size(r, R.size, p, &b) != BI_OK) break;          // (not reached: bi_check walked the same tags)
		const uint32_t ty = r[p + 2];
		const uint8_t *v = r + p + 3;
		if (ty == 'f' || ty == 'B') ++left_out;
		else if (!bi_tag_dropped_name(r[p], r[p + 1])) {
			if (o.n) o.u8('\t');
			o.u8(r[p]); o.u8(r[p + 1]); o.u8(':');
			if (ty == 'A') { o.u8('A'); o.u8(':'); o.u8(v[0]); }
			else if (ty == 'Z' || ty == 'H') { o.u8(ty); o.u8(':'); for (uint32_t k = 0; k + 4 < b; ++k) o.u8(v[k]); }
			else {
				int64_t x;
				switch (ty) {
				case 'c': x = (int8_t)v[0]; break;
				case 'C': x = v[0]; break;
				case 's': x = (int16_t)bi_u16(v); break;
				case 'S': x = bi_u16(v); break;
				case 'i': x = (int32_t)bi_u32(v); break;
				default: x = bi_u32(v); break;
				}
				o.u8('i'); o.u8(':');
				uint64_t a = x < 0 ? (uint64_t)-x : (uint64_t)x;
				if (x < 0) o.u8('-');
				uint8_t d[12]; uint32_t nd = 0;
				do { d[nd++] = (uint8_t)('0' + a % 10); a /= 10; } while (a);
				while (nd) o.u8(d[--nd]);
			}
		}
		p += b;
	}
	*n_left_out = left_out;
	return o.n;
}

// 0: no read (secondary or supplementary), 1: the first read of its pair or a single read, 2: the second read; 3: a paired record that says neither or both
BI_FN uint32_t bi_role(uint32_t flag)
{
	if (flag & BI_SKIP_FLAGS) return 0;
	if (!(flag & 1u)) return 1;
	const uint32_t w = flag & 0xc0u;
	return w == 0x40u ? 1u : w == 0x80u ? 2u : 3u;
}
