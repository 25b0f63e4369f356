// Bitmap of the K-mers of the indexed text T = fwd . revcomp(fwd), built on the device from the 2-bit text of an index handle.
//
// What it is for (smem_forward_kernel, seed_kernels.hip): a candidate [x, e) of the forward search is kept only if its backward
// search ends at a begin b with e - b >= min_seed_len.  Then read[e-K .. e) is a substring of T for every K <= min_seed_len, so a
// candidate shorter than K whose last K read bases are NOT a K-mer of T can never be kept, and everything downstream already
// ignores candidates that end too short (smem_filter_kernel skips s == 0 results, the re-seeding rounds read kept results only).
// Not emitting it saves its backward walk -- 5-15 dependent rank steps -- and its slot in every pass over the candidates.
//
// The bitmap must hold EVERY length-K substring of T: the FM index matches across the forward / reverse boundary, across contig
// boundaries and inside the filled holes alike, and all of these are plain positions of the 2-bit text.  A spurious bit would only
// cost a walk; a missing one would lose a seed.
//
// K per index: the smallest K with 4^K >= 8 x seq_len (at most one bit in eight set), capped at 18 (2^36 bits = 8 GiB beside a
// 29.5 GB index at hg38 scale).  The bitmap is a pure function of the text, built once when a handle is made; each device builds
// its own (nothing is broadcast).  Without a text, with BMH_SEED_KBITS=0, or when the allocation fails the handle has none and
// seeding runs as it does without one.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "bmh_internal.h"

#define KBITS_MAX_K 18
#define KBITS_PER_THREAD 8        // windows per thread and round: 8 + KBITS_MAX_K - 1 = 25 symbols, inside the 32 of two text words

extern "C" int bmh_kbits_k_for(uint64_t seq_len)
{
	int K = 1;
	while (K < KBITS_MAX_K && ((1ull << (2 * K)) >> 3) < seq_len) ++K;
	return K;
}

__global__ void __launch_bounds__(256) kbits_build_kernel(fmd_dev_t f, int K, uint64_t n_win, uint32_t *__restrict__ bits)
{
	const uint64_t n_grp = (n_win + KBITS_PER_THREAD - 1) / KBITS_PER_THREAD, mask = kbits_mask(K);
	for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n_grp; g += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t t0 = g * KBITS_PER_THREAD;
		// symbols t0 .. t0+31, symbol j at bits 2j+1:2j (beyond the text: 0 -- no window that starts below n_win reaches there)
		const uint64_t w = (uint64_t)fmd_text16(f, t0) | ((uint64_t)fmd_text16(f, t0 + 16) << 32);
#pragma unroll
		for (int p = 0; p < KBITS_PER_THREAD; ++p) {
			if (t0 + (uint64_t)p >= n_win) break;
			uint64_t word; uint32_t bit;
			kbits_slot((w >> (2 * p)) & mask, word, bit);
			atomicOr(&bits[word], bit);
		}
	}
}

// Builds the bitmap of `ix` on the CURRENT device (the one that holds ix's arrays) and waits for it.  Never fails the caller: on any
// problem the handle is left without a bitmap.
void bmh_kbits_attach(bmh_index *ix)
{
	ix->dev.kbits = nullptr; ix->dev.kbits_k = 0;
	const fmd_dev_t &f = ix->dev;
	const char *sw = getenv("BMH_SEED_KBITS");
	if (sw && sw[0] == '0') return;
	if (!f.pac || f.l_pac == 0 || f.seq_len != 2 * f.l_pac) return;       // no text, or not the text of this index
	const int K = bmh_kbits_k_for(f.seq_len);
	if (f.seq_len < (uint64_t)K) return;
	const uint64_t n_words = kbits_n_words(K), n_win = f.seq_len - (uint64_t)K + 1;
	uint32_t *d = nullptr;
	hipEvent_t e0 = nullptr, e1 = nullptr;
	bool ok = hipMalloc((void **)&d, (size_t)n_words * 4) == hipSuccess;
	ok = ok && hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess;
	ok = ok && hipEventRecord(e0, 0) == hipSuccess && hipMemsetAsync(d, 0, (size_t)n_words * 4, 0) == hipSuccess;
	if (ok) {
		const uint64_t nb = ((n_win + KBITS_PER_THREAD - 1) / KBITS_PER_THREAD + 255) / 256;
		kbits_build_kernel<<<(unsigned)(nb < (1u << 20) ? nb : (1u << 20)), 256>>>(f, K, n_win, d);
		ok = hipGetLastError() == hipSuccess && hipEventRecord(e1, 0) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
	}
	if (ok && getenv("BMH_SEED_STATS")) {
		float ms = 0.f;
		(void)hipEventElapsedTime(&ms, e0, e1);
		fprintf(stderr, "[kbits] K = %d, %llu windows, bitmap %.3f MiB, built in %.1f ms\n", K, (unsigned long long)n_win, (double)n_words * 4.0 / 1048576.0, ms);
	}
	if (e0) (void)hipEventDestroy(e0);
	if (e1) (void)hipEventDestroy(e1);
	if (!ok) {
		(void)hipGetLastError();                 // the handle simply has no bitmap: leave no sticky error behind
		if (d) (void)hipFree(d);
		return;
	}
	ix->dev.kbits = d; ix->dev.kbits_k = K;
}

void bmh_kbits_free(bmh_index *ix)
{
	if (ix->dev.kbits) (void)hipFree((void *)ix->dev.kbits);
	ix->dev.kbits = nullptr; ix->dev.kbits_k = 0;
}

// K (0: the handle has no bitmap), the bitmap's device pointer and its length in 32-bit words
extern "C" int bmh_index_kbits_info(const bmh_index_t *ix, int *k, const uint32_t **d_bits, uint64_t *n_words)
{
	if (!ix) { bmh_set_error("bmh_index_kbits_info: null index"); return BMH_EINVAL; }
	const bool has = ix->dev.kbits != nullptr;
	if (k) *k = has ? ix->dev.kbits_k : 0;
	if (d_bits) *d_bits = ix->dev.kbits;
	if (n_words) *n_words = has ? kbits_n_words(ix->dev.kbits_k) : 0;
	return BMH_OK;
}
