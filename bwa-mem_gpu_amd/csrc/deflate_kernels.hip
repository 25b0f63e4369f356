// Bytes in device memory -> BGZF members (bmh_bgzf_deflate_device; the BAM output of csrc/align_pipeline.hip), and the same on host threads.
//
// Mapping: one wave per member -- a workgroup of 64 lanes takes the piece of at most 0xff00 bytes at blockIdx.x and runs csrc/deflate_core.h on it, its
// state (the position table, the CRC table, histograms, codes: about 38 KiB) in LDS, so four waves share a CU.  Every member is written into a zeroed slot
// of 65 536 bytes (the bits are ORed in); a scan over the members' sizes and a copy kernel then put them back to back.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <cstring>
#include <rocprim/rocprim.hpp>
#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>
#include "bmh_internal.h"
#include "deflate_core.h"
#include "bam_ws.h"

extern "C" const uint8_t bmh_bgzf_eof[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};

namespace {

__global__ void __launch_bounds__(64) dfl_members(const uint8_t *__restrict__ in, uint64_t n, int level, uint8_t *slots, uint32_t *__restrict__ sizes)
{
	__shared__ dfl_state_t sh;
	const uint64_t a = (uint64_t)blockIdx.x * DFL_PIECE;
	if (a >= n) return;
	const uint32_t len = n - a < DFL_PIECE ? (uint32_t)(n - a) : DFL_PIECE;
	const uint32_t sz = dfl_member(sh, in + a, len, (uint32_t *)(slots + (size_t)blockIdx.x * DFL_SLOT), level);
	if (threadIdx.x == 0) sizes[blockIdx.x] = sz;
}

__global__ void __launch_bounds__(256) dfl_gather(const uint8_t *__restrict__ slots, const uint32_t *__restrict__ sizes, const uint64_t *__restrict__ off, uint8_t *__restrict__ out, uint64_t out_bytes)
{
	const uint32_t m = blockIdx.x, sz = sizes[m];
	const uint64_t o = off[m];
	if (sz > DFL_SLOT || o > out_bytes || sz > out_bytes - o) return;
	const uint8_t *s = slots + (size_t)m * DFL_SLOT;
	for (uint32_t k = threadIdx.x; k < sz; k += 256) out[o + k] = s[k];
}

}   // namespace

extern "C" int bmh_bgzf_deflate_device(bmh_bam_ws_t *ws, const uint8_t *d_in, uint64_t n, int level, void *stream_, const uint8_t **d_out, uint64_t *out_bytes)
{
	const char *fn = "bmh_bgzf_deflate_device";
	if (!ws || !d_out || !out_bytes || (n && !d_in)) { bmh_set_error("%s: null argument", fn); return BMH_EINVAL; }
	if (level != 0 && level != 1) { bmh_set_error("%s: level %d (0 or 1)", fn, level); return BMH_EINVAL; }
	*d_out = nullptr; *out_bytes = 0;
	if (n == 0) return BMH_OK;
	hipStream_t st = (hipStream_t)stream_;
	const uint64_t nm = (n + DFL_PIECE - 1) / DFL_PIECE;
	if (nm > 0x7fffffffull) { bmh_set_error("%s: %llu bytes in one call", fn, (unsigned long long)n); return BMH_EINVAL; }
	RCK(ws->slots.need((size_t)nm * DFL_SLOT)); RCK(ws->msize.need(4 * (nm + 1))); RCK(ws->moff.need(8 * (nm + 2)));
	size_t tb = scan_tmp_bytes<uint32_t, uint64_t>((size_t)nm + 1);
	RCK(ws->mtmp.need(tb));
	uint32_t *sizes = (uint32_t *)ws->msize.p; uint64_t *off = (uint64_t *)ws->moff.p;
	HIPCK(hipMemsetAsync(ws->slots.p, 0, (size_t)nm * DFL_SLOT, st));
	HIPCK(hipMemsetAsync(sizes, 0, 4 * (nm + 1), st));
	hipLaunchKernelGGL(dfl_members, dim3((unsigned)nm), dim3(64), 0, st, d_in, n, level, (uint8_t *)ws->slots.p, sizes);
	HIPCK(hipGetLastError());
	HIPCK(rocprim::exclusive_scan(ws->mtmp.p, tb, sizes, off, (uint64_t)0, (size_t)nm + 1, rocprim::plus<uint64_t>(), st));
	uint64_t total = 0;
	HIPCK(hipMemcpyAsync(&total, off + nm, 8, hipMemcpyDeviceToHost, st));
	HIPCK(hipStreamSynchronize(st));
	if (total < 28 * nm || total > nm * (uint64_t)(DFL_PIECE + 31)) { bmh_set_error("%s: internal error: %llu members of %llu bytes", fn, (unsigned long long)nm, (unsigned long long)total); return BMH_EINVAL; }
	RCK(ws->members.need((size_t)total + 16));
	hipLaunchKernelGGL(dfl_gather, dim3((unsigned)nm), dim3(256), 0, st, (const uint8_t *)ws->slots.p, sizes, off, (uint8_t *)ws->members.p, total);
	HIPCK(hipGetLastError());
	*d_out = (const uint8_t *)ws->members.p; *out_bytes = total;
	return BMH_OK;
}

extern "C" int bmh_deflate_blocks_host(const uint8_t *in, uint64_t n, int level, uint8_t *slots, uint32_t *sizes, int n_threads)
{
	const char *fn = "bmh_deflate_blocks_host";
	if (n == 0) return BMH_OK;
	if (!in || !slots || !sizes) { bmh_set_error("%s: null argument", fn); return BMH_EINVAL; }
	if (level != 0 && level != 1) { bmh_set_error("%s: level %d (0 or 1)", fn, level); return BMH_EINVAL; }
	const uint64_t nm = (n + DFL_PIECE - 1) / DFL_PIECE;
	const unsigned T = (unsigned)std::max<int64_t>(1, std::min<int64_t>(n_threads > 0 ? n_threads : bmh_effective_cpus(), (int64_t)nm));
	std::atomic<uint64_t> next{0};
	auto work = [&]() {
		dfl_state_t *sh = new dfl_state_t();
		for (uint64_t m = next.fetch_add(1); m < nm; m = next.fetch_add(1)) {
			const uint64_t a = m * DFL_PIECE;
			sizes[m] = dfl_member(*sh, in + a, n - a < DFL_PIECE ? (uint32_t)(n - a) : DFL_PIECE, (uint32_t *)(slots + (size_t)m * DFL_SLOT), level);
		}
		delete sh;
	};
	if (T == 1) work();
	else { std::vector<std::thread> th; for (unsigned t = 0; t < T; ++t) th.emplace_back(work); for (auto &x : th) x.join(); }
	return BMH_OK;
}

extern "C" int bmh_bgzf_deflate_host(const uint8_t *in, uint64_t n, int level, int n_threads, uint8_t **out, uint64_t *out_bytes)
{
	const char *fn = "bmh_bgzf_deflate_host";
	if (!out || !out_bytes || (n && !in)) { bmh_set_error("%s: null argument", fn); return BMH_EINVAL; }
	*out = nullptr; *out_bytes = 0;
	const uint64_t nm = (n + DFL_PIECE - 1) / DFL_PIECE;
	uint8_t *slots = (uint8_t *)calloc((size_t)nm * DFL_SLOT + 4, 1);
	std::vector<uint32_t> sizes(nm + 1, 0);
	if (!slots) { bmh_set_error("%s: out of memory", fn); return BMH_ENOMEM; }
	const int rc = bmh_deflate_blocks_host(in, n, level, slots, sizes.data(), n_threads);
	if (rc != BMH_OK) { free(slots); return rc; }
	uint64_t total = 0;
	for (uint64_t m = 0; m < nm; ++m) total += sizes[m];
	uint8_t *o = (uint8_t *)malloc(total + 1);
	if (!o) { free(slots); bmh_set_error("%s: out of memory", fn); return BMH_ENOMEM; }
	uint64_t p = 0;
	for (uint64_t m = 0; m < nm; ++m) { memcpy(o + p, slots + (size_t)m * DFL_SLOT, sizes[m]); p += sizes[m]; }
	free(slots);
	*out = o; *out_bytes = total;
	return BMH_OK;
}
