// Types shared by the seeding kernels (seed_kernels.hip) and the re-seeding rounds (reseed_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fmd_dev.h"
#include "../../include/bwamem_hip.h"

struct read_view_t {
	const uint32_t *pk;   // [word][read] 2-bit, base i at bits 2*(i&15)
	const uint32_t *nm;   // [word32][read] N mask, base i at bit i&31
	uint32_t n_reads;
};

__device__ __forceinline__ int read_base(const read_view_t &v, uint32_t r, int i)
{
	uint32_t w = v.pk[(size_t)(i >> 4) * v.n_reads + r];
	uint32_t m = v.nm[(size_t)(i >> 5) * v.n_reads + r];
	return ((m >> (i & 31)) & 1) ? 4 : (int)((w >> ((i & 15) << 1)) & 3);
}

struct res_t { uint32_t read, be, s, pad; };   // be = begin<<16 | end; s == 0: dropped

// The scan over the first round's occurrence counts carries the number of kept results in its high bits (seed_kernels.hip)
#define OCC_OFF_SHIFT 36
#define OCC_OFF_MASK ((1ull << OCC_OFF_SHIFT) - 1ull)

// ---- re-seeding (reseed_kernels.hip): the first round's kept SMEMs in, the merged groups of all rounds out
struct reseed_in_t {
	fmd_dev_t f; read_view_t rv;
	const uint32_t *lens; uint32_t n_reads; uint32_t max_len; int min_seed_len;
	const res_t *res_a; const uint64_t *res_k; const uint32_t *occ; const uint64_t *occ_off;   // first round: [n_cands], occ != 0 = kept
	uint64_t n_cands, n_kept;
	bmh_reseed_opt_t opt;
	uint32_t *n_ref_pos, *prefix;          // [n_reads], written
};
struct reseed_out_t {
	const res_t *res_a; const uint64_t *res_k; const uint32_t *occ; const uint64_t *occ_off;   // [n] groups by (read, begin, end); occ_off plain sums
	uint64_t n, n_occ;
	uint64_t n_round[3];                   // groups from rounds 1, 2, 3
};
struct reseed_state_t;
int reseed_merge(reseed_state_t **R, const reseed_in_t &in, hipStream_t st, reseed_out_t *out);
void reseed_state_free(reseed_state_t *R);
void reseed_counts_reset(void);         // zeroes what bmh_reseed_last_counts returns (the calling thread's)
