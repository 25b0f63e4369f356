// Duplicate marking on the device (csrc/bam_dup_core.h's rules).
//
//   per batch   heads: one lane per record, through the converter's offsets -- does it begin a template, is it a secondary / supplementary / unmapped line;
//               an inclusive scan of the heads gives every record its batch-local template ordinal; starts: a head writes its record index at its ordinal;
//               entries: one lane per template over its few records -> (end word lo, end word hi, score, kind | records << 2), 24 bytes; with read groups the
//               lane also walks its first record's tags to RG:Z and compares the ID with the run's table row by row (a few short IDs in global memory: the
//               same rows for every lane of a batch of a run over groups, rows that differ from lane to lane in a run that keeps its input's read groups,
//               whose batches mix them) -- the library goes into the end words' top byte; such a mixed batch also counts its secondary / supplementary,
//               unmapped and template records per library (bdp_batch_lib_counts)
//   decision    at the end of the input, over all templates' entries.  Pair pass: three stable 64-bit radix passes (rank word, hi, lo; templates that are no
//               pair carry all-ones words and sort behind the pairs), then a lane is a duplicate iff its (lo, hi) equals the lane's before it.  Fragment pass:
//               the fragments plus two items per pair (one per end), compacted through a scan; two stable passes (pair ends first, fragments best-first; then
//               the end word); run heads, a max-scan of the heads' indices, and a lane decides from the first item of its run -- a run may span workgroups.
//               Output: a bitmap over global template ordinals and five counters.  Libraries need no pass of their own: their keys differ.  With read groups
//               one more kernel counts the five per library from the entries' library bytes and the bitmap (a histogram in LDS per workgroup)
//   optical     only with an optical distance (csrc/bam_dup_core.h): per batch the entries kernel's LOC instance also parses the template's read name into a 16-byte
//               location; at the decision, between the pair pass and the fragment pass and in their arrays: set heads and their scan, the sets' starts (so a
//               lane knows its set's size), the located pairs of the sets of 2 .. max_set compacted through a scan, two stable radix passes (tile and x; then
//               set head, read group and role), one lane per member walking its x window and uniting in a union-find in global memory (parent [v] <= v:
//               every find descends; atomicMin halves paths, atomicCAS hooks the larger root under the smaller), members and roots counted per library in LDS
//   barcodes    only when the run compares them (csrc/bam_dup_core.h): per batch the entries kernel's BC instance also walks the first record's tags to the barcode's
//               (or its name to the last field), hashes the value in one walk and writes one 64-bit word per template into a side array; at the decision the
//               words go up once, the pair pass and the fragment pass each take one more stable radix pass on them (LSD order rank, barcode, hi, lo; and
//               fragment word, barcode, end word), and the lanes that compare keys -- pair decide, run heads, the optical set heads -- compare the word too
//   grouping    only when the run groups barcodes by edits (csrc/bam_dup_core.h): per batch the entries kernel's PACK instance packs the value instead of hashing it.
//               At the decision, before the pair pass and again before the fragment pass's sorts, over the pass's barcoded elements (pairs; items): stable radix
//               passes to (key, word) order, heads of equal (key, word) and of equal key with their scans, one member per distinct (key, word) compacted with
//               its key's first member, one lane per member walking the later members of its key -- one xor, three folds and a popcount per candidate -- and
//               uniting in the optical step's union-find (members ascend by word inside a key, so a root is its component's smallest word), members, roots
//               and keys over the cap counted per library in LDS, and every element's canonical word written: by template for the pair pass (which pair
//               decide and the optical set heads then compare), by item for the fragment pass (whose barcode radix pass and run heads then read it)
//   per window  one lane per record tests the bitmap through the record's global template ordinal and ORs 0x04 into byte 19 (a byte store: records are unaligned)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <rocprim/rocprim.hpp>
#include <algorithm>
#include <vector>
#include "bam_dup.h"
#include "bam_sort.h"
#include "bam_ws.h"

struct bdp_dev_t {
	dev_buf<uint8_t> head, tpl, start, entries, info, tmp, lib3, locs, bcs;       // per batch (locs: only when optical duplicates are counted; bcs: only when barcodes are compared)
	dev_buf<uint8_t> bits, tord;                                                  // the bitmap of the run, a window's ordinals
	dev_buf<uint8_t> g_ids, g_off, g_lib; uint32_t g_n = 0;                       // the run's read groups (bdp_dev_set_groups): IDs, their offsets, libraries; 0: none
	uint64_t n_tpl = 0;                                                     // templates the bitmap covers
};

namespace {

// info: [0] templates (written by the host side from the scan) [1] the first bad record + 1 (atomicMin; 0xffffffff: none) [2] secondary / supplementary [3] unmapped
__global__ void __launch_bounds__(256) bdp_heads(const uint8_t *__restrict__ recs, const uint64_t *__restrict__ off, uint32_t n, uint64_t total, uint32_t *__restrict__ head, uint32_t *info)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	uint32_t fl = 0; bool valid = false;
	if (i < n) {
		const uint64_t o = off[i];
		valid = o <= total && total - o >= BSR_FIXED;
		if (valid) fl = bsr_flag(recs + o);
		head[i] = valid && bdp_head(fl) ? 1u : 0u;
		if (i == 0 && !(valid && bdp_head(fl))) atomicMin(info + 1, 0u);      // (0: the first record begins no template -- reported as n + 1 by the host side)
	}
	const int c0 = __syncthreads_count(valid && (fl & 0x900u)), c1 = __syncthreads_count(valid && (fl & 4u));
	if (threadIdx.x == 0) { if (c0) atomicAdd(info + 2, (uint32_t)c0); if (c1) atomicAdd(info + 3, (uint32_t)c1); }
}

// tpl: the inclusive scan of head -> ordinals (scan - 1); a head writes its record index at its ordinal
__global__ void __launch_bounds__(256) bdp_starts(const uint32_t *__restrict__ head, uint32_t *__restrict__ tpl, uint32_t n, uint32_t *__restrict__ start, uint32_t *info)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const uint32_t s = tpl[i];
	const uint32_t t = s ? s - 1 : 0;                                      // (s == 0 only when the first record begins no template: the batch is refused)
	tpl[i] = t;
	if (head[i] && t < n) start[t] = i;
	if (i == n - 1) { info[0] = s; if (s < n + 1) start[s < n ? s : n] = n; }
}

// LIB: the run has read groups (G) -- info [4], [5]: the first template without an RG:Z tag / with an unknown ID, as info [1]
// LOC: optical duplicates are counted -- the lane holds the template's first record and parses its name: locs [t]
// BC: barcodes are compared -- the lane walks its first record's tags to the barcode's, or its name to the last field, hashes the value in one walk and writes the
// word: bcs [t]; info [6], [7]: the first template whose tag is of another type than Z / whose tags cannot be walked, as info [1]
// BC 2: the words are packed, not hashed (grouping by edits) -- info [8]: the first template whose value does not pack
template <bool LIB, bool LOC, int BC>
__global__ void __launch_bounds__(256) bdp_entries(const uint8_t *__restrict__ recs, const uint64_t *__restrict__ off, uint32_t n, uint64_t total, const uint32_t *__restrict__ start,
                                                   bdp_entry_t *__restrict__ entries, uint32_t *info, bdp_groups_t G, bdp_loc_t *__restrict__ locs, bdp_bc_t bc, uint64_t *__restrict__ bcs)
{
	const uint32_t t = blockIdx.x * 256 + threadIdx.x;
	if (t >= n || t >= info[0] || info[1] == 0) return;
	const uint32_t a = start[t], b = start[t + 1];
	bdp_entry_t e; e.lo = e.hi = ~0ull; e.score = 0; e.kind_n = 0;
	uint32_t role = 0, row = 0;
	int st = a < b && b <= n && off[b] <= total ? BDP_E_OK : BDP_E_TEMPLATE;      // (offsets ascend: every record of the template lies inside the buffer)
	const bool inside = st == BDP_E_OK;
	if (st == BDP_E_OK) st = LIB ? bdp_entry_lib(recs, off, a, b, G, &e, LOC ? &role : nullptr, LOC ? &row : nullptr) : bdp_entry(recs, off, a, b, &e, LOC ? &role : nullptr) ? BDP_E_OK : BDP_E_TEMPLATE;
	entries[t] = e;
	if (LOC) {
		bdp_loc_t l; l.x = l.y = 0; l.tile = 0; l.rg = 0; l.flags = 0;
		if (inside && st == BDP_E_OK) l = bdp_location(recs + off[a], role, row, BC && bc.mode == BDP_BC_NAME);
		locs[t] = l;
	}
	if (BC) {
		uint64_t w = 0;
		if (inside) {                                                 // (record a lies inside the buffer: off [a + 1] <= off [b] <= total)
			const int bs = bdp_barcode(recs + off[a], off[a + 1] - off[a], bc, &w, BC == 2);
			if (bs != BDP_AUX_FOUND) atomicMin(info + (bs == BDP_AUX_TYPE ? 6 : BC == 2 && bs == BDP_AUX_PACK ? 8 : 7), a + 1);
		}
		bcs[t] = w;
	}
	if (st == BDP_E_TEMPLATE) atomicMin(info + 1, a + 1);
	else if (LIB && st != BDP_E_OK) atomicMin(info + (st == BDP_E_NO_RG ? 4 : 5), a + 1);
}

// A batch whose templates are of several libraries: per library its secondary / supplementary records, unmapped records and templates -- out [3 * n_lib], through a
// histogram in LDS (3 * n_lib 32-bit words, 3 KiB at the most; a batch holds fewer than 2^32 records).  A record's library is that of its template's entry; a batch
// that bdp_batch_device's info words refuse leaves nothing here that is used.
__global__ void __launch_bounds__(256) bdp_batch_lib_counts(const uint8_t *__restrict__ recs, const uint64_t *__restrict__ off, uint32_t n, uint64_t total, const uint32_t *__restrict__ tpl,
                                                            const bdp_entry_t *__restrict__ entries, const uint32_t *__restrict__ info, uint32_t n_lib, uint32_t *out)
{
	extern __shared__ uint32_t lib3_s[];
	for (uint32_t k = threadIdx.x; k < 3 * n_lib; k += 256) lib3_s[k] = 0;
	__syncthreads();
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i < n && info[1] != 0) {                                       // (info [1] == 0: the first record begins no template -- no ordinal means anything)
		const uint64_t o = off[i];
		const uint32_t t = tpl[i];
		if (o <= total && total - o >= BSR_FIXED && t < info[0] && t < n) {
			const uint32_t fl = bsr_flag(recs + o), lib = bdp_lib_of(entries[t]);
			if (lib < n_lib) {
				if (fl & 0x900u) atomicAdd(lib3_s + 3 * lib, 1u);
				if (fl & 4u) atomicAdd(lib3_s + 3 * lib + 1, 1u);
				if (bdp_head(fl)) atomicAdd(lib3_s + 3 * lib + 2, 1u);
			}
		}
	}
	__syncthreads();
	for (uint32_t k = threadIdx.x; k < 3 * n_lib; k += 256) if (lib3_s[k]) atomicAdd(out + k, lib3_s[k]);
}

// ---- the decision
__global__ void __launch_bounds__(256) bdp_iota(uint32_t *__restrict__ v, uint64_t n)
{
	const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (i < n) v[i] = (uint32_t)i;
}

// the pair pass's key of pass k (0: rank word, 1: hi, 2: lo) through the permutation so far
__global__ void __launch_bounds__(256) bdp_pair_keys(const bdp_entry_t *__restrict__ E, const uint32_t *__restrict__ perm, uint64_t n, int pass, uint64_t *__restrict__ key)
{
	const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const uint32_t t = perm[i];
	const bdp_entry_t e = E[t];
	const bool pair = bdp_kind(e) == BDP_PAIR;
	key[i] = pass == 0 ? bdp_rank_word(e, t) : !pair ? ~0ull : pass == 1 ? e.hi : e.lo;
}

// a barcode pass's key: the word of the template behind idx [i] (shift 0: a permutation of templates; 1: item ids)
__global__ void __launch_bounds__(256) bdp_bc_keys(const uint64_t *__restrict__ B, const uint32_t *__restrict__ idx, uint64_t n, int shift, uint64_t *__restrict__ key)
{
	const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (i < n) key[i] = B[idx[i] >> shift];
}

// counts: [0] pairs [1] fragments [2] duplicate pairs [3] duplicate fragments [4] records flagged
// BC: B [template] -- the barcode words, part of the key
template <bool BC>
__global__ void __launch_bounds__(256) bdp_pair_decide(const bdp_entry_t *__restrict__ E, const uint32_t *__restrict__ perm, uint64_t n, uint32_t *bits, unsigned long long *counts,
                                                       const uint64_t *__restrict__ B)
{
	__shared__ unsigned long long recs_s;
	if (threadIdx.x == 0) recs_s = 0;
	__syncthreads();
	const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	bool pair = false, dup = false;
	if (i < n) {
		const uint32_t t = perm[i];
		const bdp_entry_t e = E[t];
		pair = bdp_kind(e) == BDP_PAIR;
		if (pair && i) {
			const uint32_t tp = perm[i - 1];
			const bdp_entry_t p = E[tp];
			dup = bdp_kind(p) == BDP_PAIR && p.lo == e.lo && p.hi == e.hi && (!BC || B[tp] == B[t]);
		}
		if (dup) { atomicOr(bits + (t >> 5), 1u << (t & 31)); atomicAdd(&recs_s, (unsigned long long)bdp_n_rec(e)); }
	}
	const int cp = __syncthreads_count(pair), cd = __syncthreads_count(dup);
	if (threadIdx.x == 0) {
		if (cp) atomicAdd(counts + 0, (unsigned long long)cp);
		if (cd) atomicAdd(counts + 2, (unsigned long long)cd);
		if (recs_s) atomicAdd(counts + 4, recs_s);
	}
}

// items of the fragment pass per template: 2 for a pair, 1 for a fragment
__global__ void __launch_bounds__(256) bdp_item_counts(const bdp_entry_t *__restrict__ E, uint64_t n, uint32_t *__restrict__ cnt, unsigned long long *counts)
{
	const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	uint32_t k = BDP_NONE;
	if (t < n) { k = bdp_kind(E[t]); cnt[t] = k == BDP_PAIR ? 2u : k == BDP_FRAG ? 1u : 0u; }
	const int cf = __syncthreads_count(k == BDP_FRAG);
	if (threadIdx.x == 0 && cf) atomicAdd(counts + 1, (unsigned long long)cf);
}

// item ids: template << 1 | end (0: lo, 1: hi)
__global__ void __launch_bounds__(256) bdp_items(const bdp_entry_t *__restrict__ E, uint64_t n, const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ base, uint64_t m, uint32_t *__restrict__ item)
{
	const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (t >= n) return;
	const uint32_t c = cnt[t], b = base[t];
	if (c >= 1 && b < m) item[b] = (uint32_t)t << 1;
	if (c == 2 && (uint64_t)b + 1 < m) item[b + 1] = (uint32_t)t << 1 | 1u;
}

__global__ void __launch_bounds__(256) bdp_frag_keys(const bdp_entry_t *__restrict__ E, const uint32_t *__restrict__ item, uint64_t m, int pass, uint64_t *__restrict__ key)
{
	const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= m) return;
	const uint32_t id = item[i], t = id >> 1;
	const bdp_entry_t e = E[t];
	key[i] = pass == 0 ? bdp_frag_word(e, t) : (id & 1u) ? e.hi : e.lo;
}

// word: the sorted end words; hidx [i] = i where a run begins, else 0
// BC: a run is the items of one (end word, barcode word) -- item: the items in sorted order, B [template] (1) or, grouped by edits, B [item id] (2)
template <int BC>
__global__ void __launch_bounds__(256) bdp_run_heads(const uint64_t *__restrict__ word, uint64_t m, uint32_t *__restrict__ hidx, const uint32_t *__restrict__ item, const uint64_t *__restrict__ B)
{
	const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (i < m) hidx[i] = i && (word[i] != word[i - 1] || (BC && B[item[i] >> (BC == 1 ? 1 : 0)] != B[item[i - 1] >> (BC == 1 ? 1 : 0)])) ? (uint32_t)i : 0u;
}

// first [i]: the index of the first item of lane i's run (the max-scan of hidx)
__global__ void __launch_bounds__(256) bdp_frag_decide(const bdp_entry_t *__restrict__ E, const uint32_t *__restrict__ item, const uint32_t *__restrict__ first, uint64_t m, uint32_t *bits,
                                                       unsigned long long *counts)
{
	__shared__ unsigned long long recs_s;
	if (threadIdx.x == 0) recs_s = 0;
	__syncthreads();
	const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	bool dup = false;
	if (i < m) {
		const uint32_t t = item[i] >> 1;
		const bdp_entry_t e = E[t];
		if (bdp_kind(e) == BDP_FRAG) {
			const uint32_t f = first[i];
			dup = f != i;
			if (f < m && bdp_kind(E[item[f] >> 1]) == BDP_PAIR) dup = true;
			if (dup) { atomicOr(bits + (t >> 5), 1u << (t & 31)); atomicAdd(&recs_s, (unsigned long long)bdp_n_rec(e)); }
		}
	}
	const int cd = __syncthreads_count(dup);
	if (threadIdx.x == 0) { if (cd) atomicAdd(counts + 3, (unsigned long long)cd); if (recs_s) atomicAdd(counts + 4, recs_s); }
}

// the decision's five counters per library: out [BDP_N_COUNTS * n_lib] (words 0 .. 4 of every library), through a histogram in LDS (5 * n_lib 64-bit words, 10 KiB at the most)
__global__ void __launch_bounds__(256) bdp_lib_counts(const bdp_entry_t *__restrict__ E, uint64_t n, const uint32_t *__restrict__ bits, uint32_t n_lib, unsigned long long *out)
{
	extern __shared__ unsigned long long lib_s[];
	for (uint32_t k = threadIdx.x; k < 5 * n_lib; k += 256) lib_s[k] = 0;
	__syncthreads();
	const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (t < n) {
		const bdp_entry_t e = E[t];
		const uint32_t lib = bdp_lib_of(e);
		if (bdp_kind(e) != BDP_NONE && lib < n_lib) {
			unsigned long long *c = lib_s + 5 * lib;
			const uint32_t s = bdp_examined_slot(e);
			atomicAdd(c + s, 1ull);
			if (bits[t >> 5] >> (t & 31) & 1u) { atomicAdd(c + 2 + s, 1ull); atomicAdd(c + 4, (unsigned long long)bdp_n_rec(e)); }
		}
	}
	__syncthreads();
	for (uint32_t k = threadIdx.x; k < 5 * n_lib; k += 256) if (lib_s[k]) atomicAdd(out + BDP_N_COUNTS * (k / 5) + k % 5, lib_s[k]);
}

// ---- the optical step (csrc/bam_dup_core.h): after the pair pass perm [n] holds the templates with the pairs first, the pairs of one key (a set) next to each other

BSR_FN bool bdp_same_set(const bdp_entry_t &a, const bdp_entry_t &b) { return a.lo == b.lo && a.hi == b.hi; }

// head [i] = 1 where a set begins
// BC: a set is the pairs of one (lo, hi, barcode word) -- B [template]
template <bool BC>
__global__ void __launch_bounds__(256) bdp_opt_heads(const bdp_entry_t *__restrict__ E, const uint32_t *__restrict__ perm, uint64_t n, uint32_t *__restrict__ head, const uint64_t *__restrict__ B)
{
	const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const uint32_t t = perm[i];
	const bdp_entry_t e = E[t];
	bool h = bdp_kind(e) == BDP_PAIR;
	if (h && i) { const uint32_t tp = perm[i - 1]; const bdp_entry_t p = E[tp]; h = !(bdp_kind(p) == BDP_PAIR && bdp_same_set(p, e) && (!BC || B[tp] == B[t])); }
	head[i] = h ? 1u : 0u;
}

// sid: the inclusive scan of head (a pair's set is sid - 1); start [s] = where set s begins, and behind the last set where the pairs end: start has n + 1 places
__global__ void __launch_bounds__(256) bdp_opt_starts(const bdp_entry_t *__restrict__ E, const uint32_t *__restrict__ perm, uint64_t n, const uint32_t *__restrict__ sid, uint32_t *__restrict__ start)
{
	const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= n || bdp_kind(E[perm[i]]) != BDP_PAIR) return;
	const uint32_t s = sid[i];                                            // (1 .. n: a pair follows at least its own set's head)
	if (s == 0 || s > n) return;
	if (s != (i ? sid[i - 1] : 0u)) start[s - 1] = (uint32_t)i;
	if (i + 1 == n || bdp_kind(E[perm[i + 1]]) != BDP_PAIR) start[s] = (uint32_t)(i + 1);
}

// member [i] = 1 for a located pair in a set of 2 .. max_set pairs; oc [4 * lib]: += located pairs, sets skipped for their size (counted at their heads) -- through a
// histogram in LDS (2 * n_lib 32-bit words; n_lib 0: one library, the entries carry none)
__global__ void __launch_bounds__(256) bdp_opt_members(const bdp_entry_t *__restrict__ E, const bdp_loc_t *__restrict__ L, const uint32_t *__restrict__ perm, uint64_t n, const uint32_t *__restrict__ sid,
                                                       const uint32_t *__restrict__ start, uint32_t max_set, uint32_t n_lib, uint32_t *__restrict__ member, unsigned long long *oc)
{
	extern __shared__ uint32_t opt_s[];
	const uint32_t nl = n_lib ? n_lib : 1u;
	for (uint32_t k = threadIdx.x; k < 2 * nl; k += 256) opt_s[k] = 0;
	__syncthreads();
	const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (i < n) {
		const uint32_t t = perm[i];
		const bdp_entry_t e = E[t];
		uint32_t m = 0;
		const uint32_t s = sid[i];
		if (bdp_kind(e) == BDP_PAIR && s >= 1 && s <= n) {
			const uint32_t lib = n_lib ? bdp_lib_of(e) : 0u;
			const uint32_t a = start[s - 1], b = start[s], len = b - a;
			const bool located = (L[t].flags & BDP_LOC_LOCATED) != 0;
			if (lib < nl) {
				if (located) atomicAdd(opt_s + 2 * lib, 1u);
				if (a == i && len > max_set) atomicAdd(opt_s + 2 * lib + 1, 1u);
			}
			m = located && len >= 2 && len <= max_set ? 1u : 0u;
		}
		member[i] = m;
	}
	__syncthreads();
	for (uint32_t k = threadIdx.x; k < 2 * nl; k += 256) if (opt_s[k]) atomicAdd(oc + 4 * (k / 2) + k % 2, (unsigned long long)opt_s[k]);
}

// the members, compacted: place p = mpos [i] - 1 (mpos: the inclusive scan of member) takes the template, the head of its set and the first sort word; m: the members
__global__ void __launch_bounds__(256) bdp_opt_compact(const bdp_loc_t *__restrict__ L, const uint32_t *__restrict__ perm, uint64_t n, const uint32_t *__restrict__ sid, const uint32_t *__restrict__ start,
                                                       const uint32_t *__restrict__ mpos, uint32_t m, uint32_t *__restrict__ otpl, uint32_t *__restrict__ oset, uint64_t *__restrict__ key, uint32_t *__restrict__ val)
{
	const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const uint32_t q = mpos[i];
	if (q == (i ? mpos[i - 1] : 0u) || q == 0 || q > m) return;           // (no member; or a place outside the arrays: never, and never written)
	const uint32_t p = q - 1, t = perm[i], s = sid[i];
	otpl[p] = t; oset[p] = s >= 1 && s <= n ? start[s - 1] : 0u; key[p] = bdp_opt_word1(L[t]); val[p] = p;
}

// the second sort word through the order of the first pass (val: places of bdp_opt_compact)
__global__ void __launch_bounds__(256) bdp_opt_keys2(const bdp_loc_t *__restrict__ L, const uint32_t *__restrict__ otpl, const uint32_t *__restrict__ oset, const uint32_t *__restrict__ val, uint32_t m,
                                                     uint64_t *__restrict__ key)
{
	const uint32_t j = blockIdx.x * 256 + threadIdx.x;
	if (j >= m) return;
	const uint32_t p = val[j];
	key[j] = p < m ? bdp_opt_word2(oset[p], L[otpl[p]]) : ~0ull;
}

// the members in their final order: tile, x, y beside the sorted second words, every member its own root
__global__ void __launch_bounds__(256) bdp_opt_gather(const bdp_loc_t *__restrict__ L, const uint32_t *__restrict__ otpl, const uint32_t *__restrict__ val, uint32_t m, uint32_t *__restrict__ tile,
                                                      int32_t *__restrict__ x, int32_t *__restrict__ y, uint32_t *__restrict__ parent)
{
	const uint32_t j = blockIdx.x * 256 + threadIdx.x;
	if (j >= m) return;
	const uint32_t p = val[j];
	bdp_loc_t l; l.x = l.y = 0; l.tile = 0; l.rg = 0; l.flags = 0;
	if (p < m) l = L[otpl[p]];
	tile[j] = l.tile; x[j] = l.x; y[j] = l.y; parent[j] = j;
}

// one lane per member: bdp_opt_walk -- bounded by m, its finds by parent [v] <= v (csrc/bam_dup_core.h)
__global__ void __launch_bounds__(256) bdp_opt_cluster(const uint64_t *__restrict__ word2, const uint32_t *__restrict__ tile, const int32_t *__restrict__ x, const int32_t *__restrict__ y, uint32_t m,
                                                       int64_t D, uint32_t *parent)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i < m) bdp_opt_walk(i, m, word2, tile, x, y, D, parent);
}

// oc [4 * lib + 2], [+ 3]: += the members and those that are their own root (their difference: the optical duplicates), as bdp_opt_members counts
__global__ void __launch_bounds__(256) bdp_opt_counts(const bdp_entry_t *__restrict__ E, const uint32_t *__restrict__ otpl, const uint32_t *__restrict__ val, const uint32_t *__restrict__ parent, uint32_t m,
                                                      uint32_t n_lib, unsigned long long *oc)
{
	extern __shared__ uint32_t opt_s[];
	const uint32_t nl = n_lib ? n_lib : 1u;
	for (uint32_t k = threadIdx.x; k < 2 * nl; k += 256) opt_s[k] = 0;
	__syncthreads();
	const uint32_t j = blockIdx.x * 256 + threadIdx.x;
	if (j < m && val[j] < m) {
		const uint32_t lib = n_lib ? bdp_lib_of(E[otpl[val[j]]]) : 0u;
		if (lib < nl) { atomicAdd(opt_s + 2 * lib, 1u); if (parent[j] == j) atomicAdd(opt_s + 2 * lib + 1, 1u); }
	}
	__syncthreads();
	for (uint32_t k = threadIdx.x; k < 2 * nl; k += 256) if (opt_s[k]) atomicAdd(oc + 4 * (k / 2) + 2 + k % 2, (unsigned long long)opt_s[k]);
}

// ---- grouping barcodes by edits (csrc/bam_dup_core.h).  An element is a barcoded pair (idx: a permutation of the templates) or, FRAG, a barcoded item of the fragment
// pass (idx: item ids); its key is (lo, hi) or the item's end word

template <bool FRAG>
__device__ inline bool bdp_grp_elem(const bdp_entry_t *__restrict__ E, const uint64_t *__restrict__ B, uint32_t id, uint64_t *a, uint64_t *b, uint64_t *w, uint32_t *t)
{
	*t = FRAG ? id >> 1 : id;
	const bdp_entry_t e = E[*t];
	*w = B[*t];
	*a = FRAG && (id & 1u) ? e.hi : e.lo; *b = FRAG ? 0ull : e.hi;
	return *w != 0 && (FRAG ? bdp_kind(e) != BDP_NONE : bdp_kind(e) == BDP_PAIR);
}

// the key of radix pass k (0: word, 1: hi, 2: lo or the end word) through the permutation so far; what is no element sorts behind the elements
template <bool FRAG>
__global__ void __launch_bounds__(256) bdp_grp_keys(const bdp_entry_t *__restrict__ E, const uint64_t *__restrict__ B, const uint32_t *__restrict__ idx, uint64_t n, int pass, uint64_t *__restrict__ key)
{
	const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	uint64_t a, b, w; uint32_t t;
	const bool el = bdp_grp_elem<FRAG>(E, B, idx[i], &a, &b, &w, &t);
	key[i] = !el ? ~0ull : pass == 0 ? w : pass == 1 ? b : a;
}

// hw [i] = 1 where a distinct (key, word) begins, hk [i] = 1 where a key begins, among the elements in sorted order
template <bool FRAG>
__global__ void __launch_bounds__(256) bdp_grp_heads(const bdp_entry_t *__restrict__ E, const uint64_t *__restrict__ B, const uint32_t *__restrict__ idx, uint64_t n, uint32_t *__restrict__ hw,
                                                     uint32_t *__restrict__ hk)
{
	const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	uint64_t a, b, w, pa = 0, pb = 0, pw = 0; uint32_t t;
	const bool el = bdp_grp_elem<FRAG>(E, B, idx[i], &a, &b, &w, &t);
	const bool prev = el && i && bdp_grp_elem<FRAG>(E, B, idx[i - 1], &pa, &pb, &pw, &t);
	const bool same_key = prev && pa == a && pb == b;
	hk[i] = el && !same_key ? 1u : 0u;
	hw[i] = el && !(same_key && pw == w) ? 1u : 0u;
}

// wid, kid: the inclusive scans of hw and hk (an element's member is wid - 1, its key kid - 1).  The head of a member writes its word, key and template and makes it
// its own root; the head of a key writes where the key's members begin: kstart has nk + 1 places, the last one m
template <bool FRAG>
__global__ void __launch_bounds__(256) bdp_grp_compact(const bdp_entry_t *__restrict__ E, const uint64_t *__restrict__ B, const uint32_t *__restrict__ idx, uint64_t n, const uint32_t *__restrict__ wid,
                                                       const uint32_t *__restrict__ kid, uint32_t m, uint32_t nk, uint64_t *__restrict__ mword, uint32_t *__restrict__ mkey, uint32_t *__restrict__ mtpl,
                                                       uint32_t *__restrict__ parent, uint32_t *__restrict__ kstart)
{
	const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	if (i == 0) kstart[nk] = m;
	const uint32_t q = wid[i], k = kid[i];
	if (q == (i ? wid[i - 1] : 0u) || q == 0 || q > m || k == 0 || k > nk) return;      // (no head; or a place outside the arrays: never, and never written)
	uint64_t a, b, w; uint32_t t;
	(void)bdp_grp_elem<FRAG>(E, B, idx[i], &a, &b, &w, &t);
	const uint32_t p = q - 1;
	mword[p] = w; mkey[p] = k - 1; mtpl[p] = t; parent[p] = p;
	if (k != (i ? kid[i - 1] : 0u)) kstart[k - 1] = p;
}

// one lane per member: bdp_bc_walk over the later members of its key -- bounded by m, its finds by parent [v] <= v; a key over the cap is left alone
__global__ void __launch_bounds__(256) bdp_grp_cluster(const uint64_t *__restrict__ mword, const uint32_t *__restrict__ mkey, const uint32_t *__restrict__ kstart, uint32_t m, uint32_t nk, uint32_t edits,
                                                       uint32_t max_set, uint32_t *parent)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= m) return;
	const uint32_t k = mkey[i];
	if (k >= nk || kstart[k + 1] - kstart[k] > max_set) return;
	bdp_bc_walk(i, m, mkey, mword, edits, parent);
}

// gc [3 * lib + BDP_GRP_*]: += the members and those that are their own root (pairs: the pair pass alone counts them) and the keys over the cap, counted at their
// first member -- through a histogram in LDS (3 * n_lib 32-bit words; n_lib 0: one library, the entries carry none)
__global__ void __launch_bounds__(256) bdp_grp_counts(const bdp_entry_t *__restrict__ E, const uint32_t *__restrict__ mtpl, const uint32_t *__restrict__ mkey, const uint32_t *__restrict__ kstart,
                                                      const uint32_t *__restrict__ parent, uint32_t m, uint32_t nk, uint32_t max_set, uint32_t n_lib, bool pairs, unsigned long long *gc)
{
	extern __shared__ uint32_t grp_s[];
	const uint32_t nl = n_lib ? n_lib : 1u;
	for (uint32_t k = threadIdx.x; k < BDP_GRP_N * nl; k += 256) grp_s[k] = 0;
	__syncthreads();
	const uint32_t j = blockIdx.x * 256 + threadIdx.x;
	if (j < m) {
		const uint32_t lib = n_lib ? bdp_lib_of(E[mtpl[j]]) : 0u, k = mkey[j];
		if (lib < nl) {
			if (pairs) { atomicAdd(grp_s + BDP_GRP_N * lib + BDP_GRP_OBSERVED, 1u); if (parent[j] == j) atomicAdd(grp_s + BDP_GRP_N * lib + BDP_GRP_INFERRED, 1u); }
			if (k < nk && kstart[k] == j && kstart[k + 1] - j > max_set) atomicAdd(grp_s + BDP_GRP_N * lib + BDP_GRP_SKIPPED, 1u);
		}
	}
	__syncthreads();
	for (uint32_t k = threadIdx.x; k < BDP_GRP_N * nl; k += 256) if (grp_s[k]) atomicAdd(gc + k, (unsigned long long)grp_s[k]);
}

// every element's canonical word -- its member's root's -- and every other's own: out [template], or FRAG out [item id]
template <bool FRAG>
__global__ void __launch_bounds__(256) bdp_grp_write(const bdp_entry_t *__restrict__ E, const uint64_t *__restrict__ B, const uint32_t *__restrict__ idx, uint64_t n, const uint32_t *__restrict__ wid,
                                                     const uint64_t *__restrict__ mword, uint32_t *parent, uint32_t m, uint64_t *__restrict__ out)
{
	const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const uint32_t id = idx[i];
	uint64_t a, b, w; uint32_t t;
	const bool el = bdp_grp_elem<FRAG>(E, B, id, &a, &b, &w, &t);
	const uint32_t q = wid[i];
	out[id] = el && q >= 1 && q <= m ? mword[bdp_uf_find(parent, q - 1)] : w;
}

// ---- the flags of a window
__global__ void __launch_bounds__(256) bdp_flag(uint8_t *__restrict__ recs, const uint64_t *__restrict__ off, const uint32_t *__restrict__ tord, uint32_t n, uint64_t total,
                                                const uint32_t *__restrict__ bits, uint64_t n_tpl)
{
	const uint32_t j = blockIdx.x * 256 + threadIdx.x;
	if (j >= n) return;
	const uint32_t t = tord[j];
	const uint64_t o = off[j];
	if (t >= n_tpl || o > total || total - o < BSR_FIXED) return;
	if (bits[t >> 5] >> (t & 31) & 1u) recs[o + 19] |= 0x04;
}

unsigned blocks(uint64_t n) { return (unsigned)((n + 255) / 256); }

// The arrays of one grouping of barcodes by edits: the decision's key and value arrays (free when it runs) and the step's own -- wid [n], mkey, mtpl, parent [m],
// kstart [m + 1]; tmp: the sorts' (sb) and the scans' (ib) work space; gc [3 * libraries]: the counters
struct grp_arrays_t { uint64_t *ka, *kb; uint32_t *va, *vb, *wid, *mkey, *mtpl, *parent, *kstart; void *tmp; size_t sb, ib; unsigned long long *gc; };

// n elements behind W.va (templates, or FRAG item ids) -> out: every element's canonical word (csrc/bam_dup_core.h), by template or by item id; the counts are added
// to W.gc.  One wait for the device: the members and the keys
template <bool FRAG>
int bdp_group_device(hipStream_t st, const bdp_entry_t *dE, const uint64_t *B, uint64_t n, grp_arrays_t W, const bdp_group_t &G, uint32_t n_lib, uint64_t *out)
{
	if (!n) return BMH_OK;
	for (int pass = 0; pass < 3; ++pass) {
		if (FRAG && pass == 1) continue;
		bdp_grp_keys<FRAG><<<blocks(n), 256, 0, st>>>(dE, B, W.va, n, pass, W.ka);
		HIPCK(rocprim::radix_sort_pairs(W.tmp, W.sb, W.ka, W.kb, W.va, W.vb, (size_t)n, 0, 64, st));
		std::swap(W.va, W.vb);
	}
	// va: the elements in (key, word) order; vb takes the key heads and their scan, ka the members' words
	uint32_t *kid = W.vb; uint64_t *mword = W.ka;
	bdp_grp_heads<FRAG><<<blocks(n), 256, 0, st>>>(dE, B, W.va, n, W.wid, kid);
	HIPCK(rocprim::inclusive_scan(W.tmp, W.ib, W.wid, W.wid, (size_t)n, rocprim::plus<uint32_t>(), st));      // (in place: heads -> members + 1, keys + 1)
	HIPCK(rocprim::inclusive_scan(W.tmp, W.ib, kid, kid, (size_t)n, rocprim::plus<uint32_t>(), st));
	uint32_t m = 0, nk = 0;
	HIPCK(hipMemcpyAsync(&m, W.wid + (n - 1), 4, hipMemcpyDeviceToHost, st));
	HIPCK(hipMemcpyAsync(&nk, kid + (n - 1), 4, hipMemcpyDeviceToHost, st));
	HIPCK(hipStreamSynchronize(st));
	if (m > n || nk > m) { bmh_set_error("duplicate marking: internal error: %u distinct barcodes on %u keys among %llu elements", m, nk, (unsigned long long)n); return BMH_EINVAL; }
	if (m) {
		const uint32_t nl = n_lib ? n_lib : 1u;
		bdp_grp_compact<FRAG><<<blocks(n), 256, 0, st>>>(dE, B, W.va, n, W.wid, kid, m, nk, mword, W.mkey, W.mtpl, W.parent, W.kstart);
		bdp_grp_cluster<<<blocks(m), 256, 0, st>>>(mword, W.mkey, W.kstart, m, nk, G.edits, G.max_set, W.parent);
		bdp_grp_counts<<<blocks(m), 256, 4 * BDP_GRP_N * nl, st>>>(dE, W.mtpl, W.mkey, W.kstart, W.parent, m, nk, G.max_set, n_lib, !FRAG, W.gc);
	}
	bdp_grp_write<FRAG><<<blocks(n), 256, 0, st>>>(dE, B, W.va, n, W.wid, mword, W.parent, m, out);
	HIPCK(hipGetLastError());
	return BMH_OK;
}

}   // namespace

bdp_dev_t *bdp_dev_create(void) { return new bdp_dev_t(); }
void bdp_dev_free(bdp_dev_t *d) { delete d; }

int bdp_batch_device(bdp_dev_t *d, const uint8_t *d_recs, const uint64_t *d_off, uint32_t n, uint64_t total, void *stream, const uint32_t **d_tpl, const bdp_entry_t **d_entries, const uint32_t **d_info,
                     const bdp_loc_t **d_locs, const bdp_bc_t *bc, const uint64_t **d_bcs, int tpl_rule)
{
	const bool want_bc = bc && bc->mode != BDP_BC_OFF;
	if (want_bc && !d_bcs) { bmh_set_error("duplicate marking: internal error: barcodes without a place for their words"); return BMH_EINVAL; }
	hipStream_t st = (hipStream_t)stream;
	size_t tb = scan_tmp_bytes<uint32_t, uint32_t, true>((size_t)n + 1);
	RCK(d->head.need(4 * ((size_t)n + 1))); RCK(d->tpl.need(4 * ((size_t)n + 1))); RCK(d->start.need(4 * ((size_t)n + 2))); RCK(d->entries.need(sizeof(bdp_entry_t) * ((size_t)n + 1)));
	const bool pack = want_bc && bc->pack;
	RCK(d->info.need(4 * (pack ? BDP_INFO_WORDS_PACK : BDP_INFO_WORDS))); RCK(d->tmp.need(tb));
	if (d_locs) RCK(d->locs.need(sizeof(bdp_loc_t) * ((size_t)n + 1)));
	if (want_bc) RCK(d->bcs.need(8 * ((size_t)n + 1)));
	static const uint32_t init[BDP_INFO_WORDS_PACK] = {0u, 0xffffffffu, 0u, 0u, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
	HIPCK(hipMemcpyAsync(d->info.p, init, 4 * (pack ? BDP_INFO_WORDS_PACK : BDP_INFO_WORDS), hipMemcpyHostToDevice, st));
	if (n) {
		if (tpl_rule == BDP_TPL_NAME) RCK(bpo_heads_device(d_recs, d_off, n, total, (uint32_t *)d->head.p, (uint32_t *)d->info.p, stream));
		else bdp_heads<<<blocks(n), 256, 0, st>>>(d_recs, d_off, n, total, (uint32_t *)d->head.p, (uint32_t *)d->info.p);
		HIPCK(rocprim::inclusive_scan(d->tmp.p, tb, (uint32_t *)d->head.p, (uint32_t *)d->tpl.p, (size_t)n, rocprim::plus<uint32_t>(), st));
		bdp_starts<<<blocks(n), 256, 0, st>>>((const uint32_t *)d->head.p, (uint32_t *)d->tpl.p, n, (uint32_t *)d->start.p, (uint32_t *)d->info.p);
		const bdp_groups_t G = {(const char *)d->g_ids.p, (const uint32_t *)d->g_off.p, (const uint8_t *)d->g_lib.p, d->g_n};
		const uint32_t *sp = (const uint32_t *)d->start.p; bdp_entry_t *ep = (bdp_entry_t *)d->entries.p; uint32_t *ip = (uint32_t *)d->info.p; bdp_loc_t *lp = (bdp_loc_t *)d->locs.p;
		const bdp_bc_t no_bc = {BDP_BC_OFF, 0, 0};
		if (pack) {
			uint64_t *bp = (uint64_t *)d->bcs.p;
			if (d_locs) {
				if (d->g_n) bdp_entries<true, true, 2><<<blocks(n), 256, 0, st>>>(d_recs, d_off, n, total, sp, ep, ip, G, lp, *bc, bp);
				else bdp_entries<false, true, 2><<<blocks(n), 256, 0, st>>>(d_recs, d_off, n, total, sp, ep, ip, G, lp, *bc, bp);
			} else if (d->g_n) bdp_entries<true, false, 2><<<blocks(n), 256, 0, st>>>(d_recs, d_off, n, total, sp, ep, ip, G, nullptr, *bc, bp);
			else bdp_entries<false, false, 2><<<blocks(n), 256, 0, st>>>(d_recs, d_off, n, total, sp, ep, ip, G, nullptr, *bc, bp);
		} else if (want_bc) {
			uint64_t *bp = (uint64_t *)d->bcs.p;
			if (d_locs) {
				if (d->g_n) bdp_entries<true, true, 1><<<blocks(n), 256, 0, st>>>(d_recs, d_off, n, total, sp, ep, ip, G, lp, *bc, bp);
				else bdp_entries<false, true, 1><<<blocks(n), 256, 0, st>>>(d_recs, d_off, n, total, sp, ep, ip, G, lp, *bc, bp);
			} else if (d->g_n) bdp_entries<true, false, 1><<<blocks(n), 256, 0, st>>>(d_recs, d_off, n, total, sp, ep, ip, G, nullptr, *bc, bp);
			else bdp_entries<false, false, 1><<<blocks(n), 256, 0, st>>>(d_recs, d_off, n, total, sp, ep, ip, G, nullptr, *bc, bp);
		} else if (d_locs) {
			if (d->g_n) bdp_entries<true, true, 0><<<blocks(n), 256, 0, st>>>(d_recs, d_off, n, total, sp, ep, ip, G, lp, no_bc, nullptr);
			else bdp_entries<false, true, 0><<<blocks(n), 256, 0, st>>>(d_recs, d_off, n, total, sp, ep, ip, G, lp, no_bc, nullptr);
		} else if (d->g_n) bdp_entries<true, false, 0><<<blocks(n), 256, 0, st>>>(d_recs, d_off, n, total, sp, ep, ip, G, nullptr, no_bc, nullptr);
		else bdp_entries<false, false, 0><<<blocks(n), 256, 0, st>>>(d_recs, d_off, n, total, sp, ep, ip, G, nullptr, no_bc, nullptr);
		HIPCK(hipGetLastError());
	}
	if (d_locs) *d_locs = (const bdp_loc_t *)d->locs.p;
	if (want_bc) *d_bcs = (const uint64_t *)d->bcs.p;
	*d_tpl = (const uint32_t *)d->tpl.p; *d_entries = (const bdp_entry_t *)d->entries.p; *d_info = (const uint32_t *)d->info.p;
	return BMH_OK;
}

int bdp_batch_lib_counts_device(bdp_dev_t *d, const uint8_t *d_recs, const uint64_t *d_off, uint32_t n, uint64_t total, uint32_t n_lib, void *stream, const uint32_t **d_lib3)
{
	hipStream_t st = (hipStream_t)stream;
	if (n_lib == 0 || n_lib > BDP_MAX_LIBS) { bmh_set_error("duplicate marking: %u libraries in a batch's counts (1 .. %d)", n_lib, (int)BDP_MAX_LIBS); return BMH_EINVAL; }
	RCK(d->lib3.need(4 * 3 * (size_t)n_lib));
	HIPCK(hipMemsetAsync(d->lib3.p, 0, 4 * 3 * (size_t)n_lib, st));
	if (n) {
		bdp_batch_lib_counts<<<blocks(n), 256, 4 * 3 * n_lib, st>>>(d_recs, d_off, n, total, (const uint32_t *)d->tpl.p, (const bdp_entry_t *)d->entries.p, (const uint32_t *)d->info.p, n_lib, (uint32_t *)d->lib3.p);
		HIPCK(hipGetLastError());
	}
	*d_lib3 = (const uint32_t *)d->lib3.p;
	return BMH_OK;
}

int bdp_dev_set_groups(bdp_dev_t *d, const bdp_table_t *T, void *stream)
{
	hipStream_t st = (hipStream_t)stream;
	d->g_n = 0;
	if (!T || T->empty()) return BMH_OK;
	const size_t n = T->lib.size();
	RCK(d->g_ids.need(T->ids.size() + 1)); RCK(d->g_off.need(4 * (n + 1))); RCK(d->g_lib.need(n));
	HIPCK(hipMemcpyAsync(d->g_ids.p, T->ids.data(), T->ids.size(), hipMemcpyHostToDevice, st));
	HIPCK(hipMemcpyAsync(d->g_off.p, T->id_off.data(), 4 * (n + 1), hipMemcpyHostToDevice, st));
	HIPCK(hipMemcpyAsync(d->g_lib.p, T->lib.data(), n, hipMemcpyHostToDevice, st));
	HIPCK(hipStreamSynchronize(st));                                      // (the table may go before the kernels that read it have run)
	d->g_n = (uint32_t)n;
	return BMH_OK;
}

int bdp_decide_device(bdp_dev_t *d, const bdp_entry_t *entries, const bdp_loc_t *locs, const uint64_t *bcs, uint64_t T, void *stream, uint64_t counts[5], const bdp_plan_t &P,
                      uint64_t n_records, double *opt_ms)
{
	hipStream_t st = (hipStream_t)stream;
	uint32_t n_lib = P.n_lib(); uint64_t *lib_counts = P.lib_counts;
	const bdp_optical_t *O = P.optical(); const bdp_group_t *G = bcs ? P.grouping() : nullptr;
	for (int k = 0; k < 5; ++k) counts[k] = 0;
	const uint32_t g_lib = G && G->lib_out ? n_lib : 0;                    // (as the optical counts: per library whether or not lib_counts is asked for)
	if (G) { for (int k = 0; k < BDP_GRP_N; ++k) G->out[k] = 0; for (uint32_t k = 0; k < BDP_GRP_N * g_lib; ++k) G->lib_out[k] = 0; }
	const uint32_t o_lib = O && O->lib_out ? n_lib : 0;                    // (the optical counts per library do not hang on lib_counts)
	if (O) { for (int k = 0; k < BDP_OPT_N; ++k) O->out[k] = 0; for (uint32_t k = 0; k < BDP_OPT_N * o_lib; ++k) O->lib_out[k] = 0; }
	if (O && T && !locs) { bmh_set_error("duplicate marking: internal error: optical duplicates without the templates' locations"); return BMH_EINVAL; }
	if (!lib_counts) n_lib = 0;
	for (uint32_t k = 0; k < BDP_N_COUNTS * n_lib; ++k) lib_counts[k] = 0;
	if (n_lib > BDP_MAX_LIBS) { bmh_set_error("duplicate marking: %u libraries: a run holds at most %d", n_lib, (int)BDP_MAX_LIBS); return BMH_EINVAL; }
	d->n_tpl = T;
	RCK(d->bits.need(4 * (size_t)((T + 31) / 32) + 4));
	HIPCK(hipMemsetAsync(d->bits.p, 0, 4 * (size_t)((T + 31) / 32) + 4, st));
	if (T == 0) { HIPCK(hipStreamSynchronize(st)); return BMH_OK; }
	if (T >= 1ull << 31) { bmh_set_error("duplicate marking: %llu templates: the decision takes fewer than 2^31", (unsigned long long)T); return BMH_EINVAL; }
	// entries, two key and two value arrays of up to 2 T items (T templates in the pair pass), the item counts and their scan, the sorts' work space, the bitmap:
	// 24 + 2 * (16 + 8) + 8 = 80 bytes per template and the work space -- freed before the final sort allocates its own (with barcodes 88)
	const size_t M = 2 * (size_t)T; size_t sb = sort_pairs_tmp_bytes<uint64_t, uint32_t>(M);
	const size_t gib = G ? scan_tmp_bytes<uint32_t, uint32_t, true>(M) : 0;      // (grouping by edits scans the heads of up to M items)
	const size_t cb = std::max(std::max(std::max(scan_tmp_bytes<uint32_t, uint32_t>((size_t)T + 1), max_scan_tmp_bytes<uint32_t>(M)), sb), gib);
	size_t fr = 0, tot = 0;
	HIPCK(hipMemGetInfo(&fr, &tot));
	// (a buffer is allocated a quarter larger than asked: that is what is counted)
	// optical duplicates: 16 bytes per template more -- the locations; the step's members, sort words and union-find live in the pair pass's key and value arrays
	const size_t opt_ask = O ? sizeof(bdp_loc_t) * (size_t)T + 8 * 4 * (size_t)(o_lib ? o_lib : 1) : 0;
	// barcodes: 8 bytes per template more -- the words; their two radix passes run in the key and value arrays of the passes beside them
	const size_t bc_ask = bcs ? 8 * (size_t)T : 0;
	// grouping by edits: 56 bytes per template more -- the canonical words of a pass (by template, then by item: 16), and for up to M elements their members
	// (4), the members' keys and templates (8), the union-find and the keys' starts (8); the sorts, the key heads and the members' words live in the key and value arrays
	const size_t grp_ask = G ? 8 * M + 4 * M + 8 * M + 4 * M + 4 * (M + 2) + 8 * BDP_GRP_N * (size_t)(g_lib ? g_lib : 1) : 0;
	const size_t ask = sizeof(bdp_entry_t) * (size_t)T + 2 * 8 * M + 2 * 4 * M + 2 * 4 * ((size_t)T + 1) + cb + opt_ask + bc_ask + grp_ask, want = ask + ask / 4 + (64u << 20);
	// the final sort that follows: keys and ordinals in and out, 24 bytes per record, a quarter more as allocated, and its work space
	const size_t sort_ask = 24 * (size_t)n_records + (n_records ? sort_pairs_tmp_bytes<uint64_t, uint32_t>((size_t)n_records) : 0), sort_want = sort_ask + sort_ask / 4 + (64u << 20);
	if (want <= fr && sort_want > fr) {
		bmh_set_error("sorted BAM: the final sort of %llu records (%llu templates to mark duplicates among) needs %zu bytes of device memory, %zu are free (sort fewer reads per run, or on a device with more memory)",
		              (unsigned long long)n_records, (unsigned long long)T, sort_want, fr);
		return BMH_ENOMEM;
	}
	if (want > fr) {
		if (G) bmh_set_error("sorted BAM: marking the duplicates among %llu templates with their barcodes grouped by edits needs %zu bytes of device memory (%zu of them the grouping's), %zu are free (align fewer reads per run, or on a device with more memory)",
		                     (unsigned long long)T, want, grp_ask + grp_ask / 4, fr);
		else if (O && bcs) bmh_set_error("sorted BAM: marking the duplicates among %llu templates by their barcodes and counting the optical ones needs %zu bytes of device memory (%zu of them the templates' locations and the optical step's counters, %zu the barcode words), %zu are free (align fewer reads per run, or on a device with more memory)",
		                            (unsigned long long)T, want, opt_ask + opt_ask / 4, bc_ask + bc_ask / 4, fr);
		else if (bcs) bmh_set_error("sorted BAM: marking the duplicates among %llu templates by their barcodes needs %zu bytes of device memory (%zu of them the barcode words), %zu are free (align fewer reads per run, or on a device with more memory)",
		                            (unsigned long long)T, want, bc_ask + bc_ask / 4, fr);
		else if (O) bmh_set_error("sorted BAM: marking the duplicates among %llu templates and counting the optical ones needs %zu bytes of device memory (%zu of them the templates' locations and the optical step's counters), %zu are free (align fewer reads per run, or on a device with more memory)",
		                     (unsigned long long)T, want, opt_ask + opt_ask / 4, fr);
		else bmh_set_error("sorted BAM: marking the duplicates among %llu templates needs %zu bytes of device memory, %zu are free (align fewer reads per run, or on a device with more memory)",
		              (unsigned long long)T, want, fr);
		return BMH_ENOMEM;
	}
	// (nine buffers allocated and freed per decision: it runs once per sorted file, and what it frees is what the final sort then takes)
	dev_buf<uint8_t> E, k0, k1, v0, v1, cnt, base, tmp, dc;
	RCK(E.need(sizeof(bdp_entry_t) * (size_t)T)); RCK(k0.need(8 * M)); RCK(k1.need(8 * M)); RCK(v0.need(4 * M)); RCK(v1.need(4 * M)); RCK(cnt.need(4 * ((size_t)T + 1)));
	RCK(base.need(4 * ((size_t)T + 1))); RCK(tmp.need(cb)); RCK(dc.need(8 * 5));
	HIPCK(hipMemcpyAsync(E.p, entries, sizeof(bdp_entry_t) * (size_t)T, hipMemcpyHostToDevice, st));
	HIPCK(hipMemsetAsync(dc.p, 0, 8 * 5, st));
	const bdp_entry_t *dE = (const bdp_entry_t *)E.p;
	uint64_t *ka = (uint64_t *)k0.p, *kb = (uint64_t *)k1.p; uint32_t *va = (uint32_t *)v0.p, *vb = (uint32_t *)v1.p;
	unsigned long long *dcnt = (unsigned long long *)dc.p;
	// the pair pass: after every radix pass vb holds the permutation, swapped into va for the next.  (tmp and sb are sized for M items and serve the sorts of T and
	// of m <= M items: rocprim takes a work space larger than it asks for, as csrc/bam_sort_kernels.hip's sorts rely on too)
	// barcodes: the words go up once; one more stable pass on them behind the rank pass (LSD order rank, barcode, hi, lo)
	dev_buf<uint8_t> dB;
	if (bcs) {
		RCK(dB.need(8 * (size_t)T));
		HIPCK(hipMemcpyAsync(dB.p, bcs, 8 * (size_t)T, hipMemcpyHostToDevice, st));
	}
	const uint64_t *B = (const uint64_t *)dB.p;
	// grouping by edits: the pair pass's canonical words first, in the arrays the pair pass then takes; the pass compares them in place of the words
	dev_buf<uint8_t> gW, g0, g1, g2, gcb; std::vector<unsigned long long> h_gc;
	grp_arrays_t GA = {};
	if (G) {
		const uint32_t nl = g_lib ? g_lib : 1u;
		RCK(gW.need(8 * M)); RCK(g0.need(4 * M)); RCK(g1.need(8 * M)); RCK(g2.need(4 * M + 4 * (M + 2))); RCK(gcb.need(8 * BDP_GRP_N * (size_t)nl));
		HIPCK(hipMemsetAsync(gcb.p, 0, 8 * BDP_GRP_N * (size_t)nl, st));
		GA = {ka, kb, va, vb, (uint32_t *)g0.p, (uint32_t *)g1.p, (uint32_t *)g1.p + M, (uint32_t *)g2.p, (uint32_t *)g2.p + M, tmp.p, sb, gib, (unsigned long long *)gcb.p};
		bdp_iota<<<blocks(T), 256, 0, st>>>(va, T);
		RCK(bdp_group_device<false>(st, dE, B, T, GA, *G, g_lib, (uint64_t *)gW.p));
	}
	const uint64_t *Bp = G ? (const uint64_t *)gW.p : B;
	bdp_iota<<<blocks(T), 256, 0, st>>>(va, T);
	for (int pass = 0; pass < 3; ++pass) {
		bdp_pair_keys<<<blocks(T), 256, 0, st>>>(dE, va, T, pass, ka);
		HIPCK(rocprim::radix_sort_pairs(tmp.p, sb, ka, kb, va, vb, (size_t)T, 0, 64, st));
		std::swap(va, vb);
		if (pass == 0 && bcs) {
			bdp_bc_keys<<<blocks(T), 256, 0, st>>>(Bp, va, T, 0, ka);
			HIPCK(rocprim::radix_sort_pairs(tmp.p, sb, ka, kb, va, vb, (size_t)T, 0, 64, st));
			std::swap(va, vb);
		}
	}
	if (bcs) bdp_pair_decide<true><<<blocks(T), 256, 0, st>>>(dE, va, T, (uint32_t *)d->bits.p, dcnt, Bp);
	else bdp_pair_decide<false><<<blocks(T), 256, 0, st>>>(dE, va, T, (uint32_t *)d->bits.p, dcnt, nullptr);
	// the optical step, on va as the pair pass left it.  Until the compaction it keeps its words in cnt, base and vb; from there on the pair pass's arrays are free
	// and take the members (m <= T of them): ka -- sort words in, values in and out; kb -- sort words out, templates, set heads; va -- x, y; vb -- tile, parent
	dev_buf<uint8_t> dL, oc; std::vector<unsigned long long> h_oc;
	struct ev_pair_t { hipEvent_t e[2] = {nullptr, nullptr}; ~ev_pair_t() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); } } oev;
	if (O) {
		const uint32_t nl = o_lib ? o_lib : 1u;
		HIPCK(hipEventCreate(&oev.e[0])); HIPCK(hipEventCreate(&oev.e[1]));
		HIPCK(hipEventRecord(oev.e[0], st));
		RCK(dL.need(sizeof(bdp_loc_t) * (size_t)T)); RCK(oc.need(8 * 4 * (size_t)nl));
		HIPCK(hipMemcpyAsync(dL.p, locs, sizeof(bdp_loc_t) * (size_t)T, hipMemcpyHostToDevice, st));
		HIPCK(hipMemsetAsync(oc.p, 0, 8 * 4 * (size_t)nl, st));
		const bdp_loc_t *L = (const bdp_loc_t *)dL.p;
		uint32_t *head = (uint32_t *)cnt.p, *sid = (uint32_t *)base.p, *start = vb;      // (start: T + 1 of vb's 2 T places)
		size_t ib = scan_tmp_bytes<uint32_t, uint32_t, true>((size_t)T + 1);
		if (ib > cb) { bmh_set_error("duplicate marking: internal error: the optical step's scan asks for %zu bytes of work space, %zu are there", ib, cb); return BMH_EINVAL; }
		if (bcs) bdp_opt_heads<true><<<blocks(T), 256, 0, st>>>(dE, va, T, head, Bp);
		else bdp_opt_heads<false><<<blocks(T), 256, 0, st>>>(dE, va, T, head, nullptr);
		HIPCK(rocprim::inclusive_scan(tmp.p, ib, head, sid, (size_t)T, rocprim::plus<uint32_t>(), st));
		bdp_opt_starts<<<blocks(T), 256, 0, st>>>(dE, va, T, sid, start);
		bdp_opt_members<<<blocks(T), 256, 4 * 2 * nl, st>>>(dE, L, va, T, sid, start, O->max_set, o_lib, head, (unsigned long long *)oc.p);
		HIPCK(rocprim::inclusive_scan(tmp.p, ib, head, head, (size_t)T, rocprim::plus<uint32_t>(), st));      // (in place: member flags -> places + 1)
		uint32_t m = 0;
		HIPCK(hipMemcpyAsync(&m, head + (T - 1), 4, hipMemcpyDeviceToHost, st));
		HIPCK(hipStreamSynchronize(st));
		if (m > T) { bmh_set_error("duplicate marking: internal error: %u optical members among %llu templates", m, (unsigned long long)T); return BMH_EINVAL; }
		if (m) {
			uint64_t *keyA = ka, *keyB = kb;
			uint32_t *valA = (uint32_t *)(ka + m), *valB = valA + m, *otpl = (uint32_t *)(kb + m), *oset = otpl + m;      // (16 m <= 16 T bytes of each array)
			bdp_opt_compact<<<blocks(T), 256, 0, st>>>(L, va, T, sid, start, head, m, otpl, oset, keyA, valA);
			HIPCK(rocprim::radix_sort_pairs(tmp.p, sb, keyA, keyB, valA, valB, (size_t)m, 0, 64, st));
			bdp_opt_keys2<<<blocks(m), 256, 0, st>>>(L, otpl, oset, valB, m, keyA);
			HIPCK(rocprim::radix_sort_pairs(tmp.p, sb, keyA, keyB, valB, valA, (size_t)m, 0, 64, st));
			// keyB: the sorted second words, valA: the members' places in that order; the pair pass's permutation has been read: va and vb take the rest
			uint32_t *gtile = vb, *parent = vb + m; int32_t *gx = (int32_t *)va, *gy = gx + m;
			bdp_opt_gather<<<blocks(m), 256, 0, st>>>(L, otpl, valA, m, gtile, gx, gy, parent);
			bdp_opt_cluster<<<blocks(m), 256, 0, st>>>(keyB, gtile, gx, gy, m, O->distance, parent);
			bdp_opt_counts<<<blocks(m), 256, 4 * 2 * nl, st>>>(dE, otpl, valA, parent, m, o_lib, (unsigned long long *)oc.p);
		}
		h_oc.assign(4 * (size_t)nl, 0);
		HIPCK(hipMemcpyAsync(h_oc.data(), oc.p, 8 * 4 * (size_t)nl, hipMemcpyDeviceToHost, st));
		HIPCK(hipEventRecord(oev.e[1], st));
		HIPCK(hipGetLastError());
	}
	// the fragment pass
	size_t eb = scan_tmp_bytes<uint32_t, uint32_t>((size_t)T + 1);
	HIPCK(hipMemsetAsync((uint32_t *)cnt.p + T, 0, 4, st));
	bdp_item_counts<<<blocks(T), 256, 0, st>>>(dE, T, (uint32_t *)cnt.p, dcnt);
	HIPCK(rocprim::exclusive_scan(tmp.p, eb, (uint32_t *)cnt.p, (uint32_t *)base.p, 0u, (size_t)T + 1, rocprim::plus<uint32_t>(), st));
	uint32_t m32 = 0;
	HIPCK(hipMemcpyAsync(&m32, (const uint32_t *)base.p + T, 4, hipMemcpyDeviceToHost, st));
	HIPCK(hipStreamSynchronize(st));
	const uint64_t m = m32;
	if (m > M) { bmh_set_error("duplicate marking: internal error: %llu items of %llu templates", (unsigned long long)m, (unsigned long long)T); return BMH_EINVAL; }
	if (m) {
		bdp_items<<<blocks(T), 256, 0, st>>>(dE, T, (const uint32_t *)cnt.p, (const uint32_t *)base.p, m, va);
		if (G) {                                                          // (the pair pass's canonical words have been read: gW takes the items')
			GA.ka = ka; GA.kb = kb; GA.va = va; GA.vb = vb;
			RCK(bdp_group_device<true>(st, dE, B, m, GA, *G, g_lib, (uint64_t *)gW.p));
			bdp_items<<<blocks(T), 256, 0, st>>>(dE, T, (const uint32_t *)cnt.p, (const uint32_t *)base.p, m, va);      // (the grouping has sorted its items: these are the pass's again)
		}
		for (int pass = 0; pass < 2; ++pass) {
			bdp_frag_keys<<<blocks(m), 256, 0, st>>>(dE, va, m, pass, ka);
			HIPCK(rocprim::radix_sort_pairs(tmp.p, sb, ka, kb, va, vb, (size_t)m, 0, 64, st));
			std::swap(va, vb);
			if (pass == 0 && bcs) {                                       // (the items carry their templates' words: LSD order frag word, barcode, end word)
				if (G) bdp_bc_keys<<<blocks(m), 256, 0, st>>>((const uint64_t *)gW.p, va, m, 0, ka);
				else bdp_bc_keys<<<blocks(m), 256, 0, st>>>(B, va, m, 1, ka);
				HIPCK(rocprim::radix_sort_pairs(tmp.p, sb, ka, kb, va, vb, (size_t)m, 0, 64, st));
				std::swap(va, vb);
			}
		}
		// kb: the sorted end words, va: the items in that order; vb is free: it takes the run heads' indices, whose max-scan goes into k0's bytes
		uint32_t *hidx = vb, *first = (uint32_t *)k0.p;                   // (ka's bytes: the keys have been read)
		size_t mb = max_scan_tmp_bytes<uint32_t>((size_t)m);
		if (G) bdp_run_heads<2><<<blocks(m), 256, 0, st>>>(kb, m, hidx, va, (const uint64_t *)gW.p);
		else if (bcs) bdp_run_heads<1><<<blocks(m), 256, 0, st>>>(kb, m, hidx, va, B);
		else bdp_run_heads<0><<<blocks(m), 256, 0, st>>>(kb, m, hidx, nullptr, nullptr);
		HIPCK(rocprim::inclusive_scan(tmp.p, mb, hidx, first, (size_t)m, rocprim::maximum<uint32_t>(), st));
		bdp_frag_decide<<<blocks(m), 256, 0, st>>>(dE, va, first, m, (uint32_t *)d->bits.p, dcnt);
	}
	unsigned long long h[5] = {0, 0, 0, 0, 0};
	HIPCK(hipMemcpyAsync(h, dcnt, 8 * 5, hipMemcpyDeviceToHost, st));
	if (G) {
		h_gc.assign(BDP_GRP_N * (size_t)(g_lib ? g_lib : 1u), 0);
		HIPCK(hipMemcpyAsync(h_gc.data(), gcb.p, 8 * h_gc.size(), hipMemcpyDeviceToHost, st));
	}
	dev_buf<uint8_t> lc;                                                  // (64 bytes per library: beside the decision's buffers nothing)
	if (n_lib) {
		RCK(lc.need(8 * BDP_N_COUNTS * (size_t)n_lib));
		HIPCK(hipMemsetAsync(lc.p, 0, 8 * BDP_N_COUNTS * (size_t)n_lib, st));
		bdp_lib_counts<<<blocks(T), 256, 8 * 5 * (size_t)n_lib, st>>>(dE, T, (const uint32_t *)d->bits.p, n_lib, (unsigned long long *)lc.p);
		HIPCK(hipMemcpyAsync(lib_counts, lc.p, 8 * BDP_N_COUNTS * (size_t)n_lib, hipMemcpyDeviceToHost, st));
	}
	HIPCK(hipStreamSynchronize(st));
	HIPCK(hipGetLastError());
	for (int k = 0; k < 5; ++k) counts[k] = h[k];
	for (size_t k = 0; k < h_gc.size(); ++k) { G->out[k % BDP_GRP_N] += h_gc[k]; if (g_lib) G->lib_out[k] = h_gc[k]; }
	if (O) {
		for (size_t l = 0; l < h_oc.size() / 4; ++l) {
			const uint64_t v[BDP_OPT_N] = {h_oc[4 * l + 2] - h_oc[4 * l + 3], h_oc[4 * l], h_oc[4 * l + 1]};
			for (int k = 0; k < BDP_OPT_N; ++k) { O->out[k] += v[k]; if (o_lib) O->lib_out[BDP_OPT_N * l + k] = v[k]; }
		}
		float ms = 0;
		HIPCK(hipEventElapsedTime(&ms, oev.e[0], oev.e[1]));
		if (opt_ms) *opt_ms += ms;
	}
	return BMH_OK;
}

int bdp_flag_device(bdp_dev_t *d, uint8_t *d_recs, const uint64_t *d_off, const uint32_t *tord, uint32_t n, uint64_t total, void *stream)
{
	hipStream_t st = (hipStream_t)stream;
	if (n == 0) return BMH_OK;
	RCK(d->tord.need(4 * (size_t)n));
	HIPCK(hipMemcpyAsync(d->tord.p, tord, 4 * (size_t)n, hipMemcpyHostToDevice, st));
	bdp_flag<<<blocks(n), 256, 0, st>>>(d_recs, d_off, (const uint32_t *)d->tord.p, n, total, (const uint32_t *)d->bits.p, d->n_tpl);
	HIPCK(hipGetLastError());
	return BMH_OK;
}

// ---------------------------------------------------------------------------------------------------------------- the stand-alone entry point

// probe: stop at the templates' locations or barcode words (bdp_probe_t)
static int markdup_device(const char *fn, const uint8_t *recs, uint64_t n_bytes, const bdp_plan_t &P, bdp_probe_t probe, void *stream, uint8_t **out, uint64_t counts[BDP_N_COUNTS])
{
	const bdp_table_t *G = P.groups(); const bdp_bc_t *bc = P.barcode();
	if (P.no_barcode) *P.no_barcode = 0;
	hipStream_t st = (hipStream_t)stream;
	if (!out || (n_bytes && !recs)) { bmh_set_error("%s: null argument", fn); return BMH_EINVAL; }
	*out = nullptr;
	for (int k = 0; k < BDP_N_COUNTS; ++k) counts[k] = 0;
	std::vector<uint64_t> off;
	RCK(bsr_walk(recs, n_bytes, -1, off, fn));
	const uint32_t n = (uint32_t)(off.size() - 1);
	for (uint32_t i = 0; i < n; ++i)
		if (!bdp_record_whole(recs + off[i], off[i + 1] - off[i])) { bmh_set_error("%s: record %u is cut: its bases and qualities do not lie inside its block_size", fn, i); return BMH_EINVAL; }
	if (G) RCK(bdp_refs_fit(recs, off.data(), n, fn));
	bdp_dev_t d;
	dev_buf<uint8_t> in, in_off;
	RCK(bdp_dev_set_groups(&d, G, st));
	RCK(in.need((size_t)n_bytes + 16)); RCK(in_off.need(8 * off.size()));
	if (n_bytes) HIPCK(hipMemcpyAsync(in.p, recs, (size_t)n_bytes, hipMemcpyHostToDevice, st));
	HIPCK(hipMemcpyAsync(in_off.p, off.data(), 8 * off.size(), hipMemcpyHostToDevice, st));
	const uint32_t *d_tpl; const bdp_entry_t *d_e; const uint32_t *d_info; const bdp_loc_t *d_l = nullptr; const uint64_t *d_b = nullptr;
	const bool want_locs = probe == BDP_PROBE_LOCS || (probe == BDP_MARK && P.optical());
	RCK(bdp_batch_device(&d, (const uint8_t *)in.p, (const uint64_t *)in_off.p, n, n_bytes, st, &d_tpl, &d_e, &d_info, want_locs ? &d_l : nullptr, bc, bc ? &d_b : nullptr));
	uint32_t info[BDP_INFO_WORDS_PACK];
	HIPCK(hipMemcpyAsync(info, d_info, 4 * bdp_info_words(bc), hipMemcpyDeviceToHost, st));
	HIPCK(hipStreamSynchronize(st));
	RCK(bdp_batch_check(n, info, G != nullptr, fn, bc != nullptr, bc && bc->pack));
	const uint32_t T = n ? info[0] : 0;
	if (T > n) { bmh_set_error("%s: internal error: %u templates among %u records", fn, T, n); return BMH_EINVAL; }
	std::vector<bdp_entry_t> E(T); std::vector<uint32_t> tpl(n); std::vector<bdp_loc_t> L(want_locs ? T : 0); std::vector<uint64_t> Bw(bc ? T : 0);
	if (T && bc) HIPCK(hipMemcpyAsync(Bw.data(), d_b, 8 * (size_t)T, hipMemcpyDeviceToHost, st));
	if (T) HIPCK(hipMemcpyAsync(E.data(), d_e, sizeof(bdp_entry_t) * (size_t)T, hipMemcpyDeviceToHost, st));
	if (n) HIPCK(hipMemcpyAsync(tpl.data(), d_tpl, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
	if (T && want_locs) HIPCK(hipMemcpyAsync(L.data(), d_l, sizeof(bdp_loc_t) * (size_t)T, hipMemcpyDeviceToHost, st));
	HIPCK(hipStreamSynchronize(st));
	if (probe != BDP_MARK) {
		const size_t nb = (probe == BDP_PROBE_LOCS ? sizeof(bdp_loc_t) : 8) * (size_t)T;
		uint8_t *o = (uint8_t *)malloc(nb + 1);
		if (!o) { bmh_set_error("%s: out of memory", fn); return BMH_ENOMEM; }
		if (T) memcpy(o, probe == BDP_PROBE_LOCS ? (const void *)L.data() : (const void *)Bw.data(), nb);
		*out = o; counts[BDP_TEMPLATES] = T;
		return BMH_OK;
	}
	if (bc && P.no_barcode) *P.no_barcode = bdp_no_barcode(Bw.data(), T);
	RCK(bdp_decide_device(&d, E.data(), L.data(), bc ? Bw.data() : nullptr, T, st, counts, P));
	counts[BDP_SECSUP] = info[2]; counts[BDP_UNMAPPED] = info[3]; counts[BDP_TEMPLATES] = T;
	if (G && P.lib_counts) bdp_lib_tally_host(recs, off.data(), n, tpl.data(), E.data(), T, G->n_lib, P.lib_counts);
	RCK(bdp_flag_device(&d, (uint8_t *)in.p, (const uint64_t *)in_off.p, tpl.data(), n, n_bytes, st));
	uint8_t *o = (uint8_t *)malloc((size_t)n_bytes + 1);
	if (!o) { bmh_set_error("%s: out of memory", fn); return BMH_ENOMEM; }
	if (n_bytes && hipMemcpyAsync(o, in.p, (size_t)n_bytes, hipMemcpyDeviceToHost, st) != hipSuccess) { free(o); bmh_set_error("%s: the copy of the records failed", fn); return BMH_ENODEV; }
	if (hipStreamSynchronize(st) != hipSuccess) { free(o); bmh_set_error("%s: %s", fn, hipGetErrorString(hipGetLastError())); return BMH_ENODEV; }
	*out = o;
	return BMH_OK;
}

extern "C" int bmh_bam_markdup_device(const uint8_t *recs, uint64_t n_bytes, const bmh_markdup_opt_t *opt, void *stream, uint8_t **out, bmh_markdup_counts_t *res)
{
	const char *fn = "bmh_bam_markdup_device";
	bdp_plan_t P;
	if (out) *out = nullptr;
	RCK(bdp_plan_make(P, opt, res, fn));
	return markdup_device(fn, recs, n_bytes, P, BDP_MARK, stream, out, res->counts);
}

extern "C" int bmh_bam_dup_locations_device(const uint8_t *recs, uint64_t n_bytes, const char *const *rg_ids, const int32_t *rg_lib, int n_groups, void *stream, uint8_t **locs, uint64_t *n_templates)
{
	const char *fn = "bmh_bam_dup_locations_device";
	if (locs) *locs = nullptr;
	if (!n_templates) { bmh_set_error("%s: null argument", fn); return BMH_EINVAL; }
	*n_templates = 0;
	bdp_plan_t P; uint64_t counts[BDP_N_COUNTS];
	RCK(bdp_probe_plan(P, rg_ids, rg_lib, n_groups, BDP_BC_OFF, nullptr, 0, fn));
	RCK(markdup_device(fn, recs, n_bytes, P, BDP_PROBE_LOCS, stream, locs, counts));
	*n_templates = counts[BDP_TEMPLATES];
	return BMH_OK;
}

extern "C" int bmh_bam_dup_barcodes_device(const uint8_t *recs, uint64_t n_bytes, int barcode_mode, const char tag[2], int packed, void *stream, uint64_t **words, uint64_t *n_templates)
{
	const char *fn = "bmh_bam_dup_barcodes_device";
	if (words) *words = nullptr;
	if (!n_templates) { bmh_set_error("%s: null argument", fn); return BMH_EINVAL; }
	*n_templates = 0;
	if (barcode_mode == BDP_BC_OFF) { bmh_set_error("%s: no barcode source (1: a tag, 2: the read name)", fn); return BMH_EINVAL; }
	bdp_plan_t P; uint64_t counts[BDP_N_COUNTS];
	RCK(bdp_probe_plan(P, nullptr, nullptr, 0, barcode_mode, tag, packed, fn));
	RCK(markdup_device(fn, recs, n_bytes, P, BDP_PROBE_BCS, stream, (uint8_t **)words, counts));
	*n_templates = counts[BDP_TEMPLATES];
	return BMH_OK;
}
