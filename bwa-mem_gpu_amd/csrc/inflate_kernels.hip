// BGZF members inflated on the device (bmh_inflate_members_device, bmh_bgzf_inflate; the read-file path of csrc/reads_parse.hip).
//
// Mapping: one lane per member, 64 members per workgroup of one wave.  A member is one dependent bit stream of at most 64 KiB of text, a read window
// holds thousands of them, and the decoder of csrc/inflate_core.h is the same code the host runs.  Per lane, in LDS (interleaved by lane, so the 64
// lanes' entry i share banks pairwise whatever i each lane asks for): the 9-bit literal / length lookup table, the counts per code length and the
// distance symbols -- 576 halfwords, 72 KiB per wave, 73 KiB (74 752 bytes) with the shared 1 KiB CRC table: two waves per CU.  The sorted literal / length symbols (used by
// codes beyond 9 bits and while a table is built) and the code lengths are in the lane's private memory.  The text goes straight to its final place in
// HBM: a back-reference reads bytes the same lane stored, which needs no fence.  The CRC32 runs beside the decode, a byte-table walk in LDS.
// Every table entry is checked against the buffers' sizes before its member is touched; a member that fails a check only writes its status word.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <thread>
#include <vector>
#include "bmh_internal.h"
#include "inflate_core.h"

namespace {

constexpr int INF_HOT = (1 << INF_FAST_BITS) + 16 + 16 + 32;       // halfwords per lane in LDS

struct inf_dev_ws_t {
	uint16_t *hot; const uint32_t *crc; uint16_t *lsym_; uint8_t *len_;
	__device__ __forceinline__ uint16_t &fast(uint32_t i) { return hot[i * 64]; }
	__device__ __forceinline__ uint16_t &lcnt(uint32_t i) { return hot[((1 << INF_FAST_BITS) + i) * 64]; }
	__device__ __forceinline__ uint16_t &dcnt(uint32_t i) { return hot[((1 << INF_FAST_BITS) + 16 + i) * 64]; }
	__device__ __forceinline__ uint16_t &dsym(uint32_t i) { return hot[((1 << INF_FAST_BITS) + 32 + i) * 64]; }
	__device__ __forceinline__ uint16_t &lsym(uint32_t i) { return lsym_[i]; }
	__device__ __forceinline__ uint8_t &len(uint32_t i) { return len_[i]; }
	__device__ __forceinline__ uint32_t crc_tab(uint32_t i) const { return crc[i]; }
};

__global__ void __launch_bounds__(64) inf_members(const uint8_t *__restrict__ in, uint64_t in_bytes, const bmh_inflate_member_t *__restrict__ tab, uint32_t n,
                                                  uint8_t *out, uint64_t out_bytes, uint32_t *__restrict__ status)
{
	__shared__ uint16_t hot[INF_HOT * 64];
	__shared__ uint32_t crc[256];
	uint16_t lsym[288]; uint8_t len[320];
	const uint32_t lane = threadIdx.x;
	for (uint32_t i = lane; i < 256; i += 64) crc[i] = inf_crc_entry(i);
	__syncthreads();
	const uint32_t m = blockIdx.x * 64 + lane;
	if (m >= n) return;
	const bmh_inflate_member_t t = tab[m];
	const uint32_t cap = t.isize < INF_MAX_OUT ? t.isize : INF_MAX_OUT;
	if (t.in_off > in_bytes || t.in_len > in_bytes - t.in_off || t.out_off > out_bytes || cap > out_bytes - t.out_off) { status[m] = INF_ETABLE; return; }
	inf_dev_ws_t ws; ws.hot = hot + lane; ws.crc = crc; ws.lsym_ = lsym; ws.len_ = len;
	uint32_t got = 0;
	status[m] = (uint32_t)inf_member(ws, in + t.in_off, t.in_len, out + t.out_off, t.isize, t.crc32, &got);
}

const char *inf_what(uint32_t s)
{
	static const char *const w[] = {"ok", "block type 3", "a stored block whose LEN and NLEN disagree", "a bad code-length set", "a bit pattern that is no symbol",
	                                "a distance beyond the start of the text", "the deflate data end early", "the text is not ISIZE bytes", "the CRC32 differs", "the member table points outside the buffers"};
	return s < sizeof(w) / sizeof(w[0]) ? w[s] : "unknown status";
}

}   // namespace

extern "C" int bmh_inflate_members_device(const uint8_t *d_in, uint64_t in_bytes, const bmh_inflate_member_t *d_tab, uint32_t n, uint8_t *d_out, uint64_t out_bytes,
                                          uint32_t *d_status, void *stream)
{
	if (n == 0) return BMH_OK;
	if (!d_in || !d_tab || !d_out || !d_status) { bmh_set_error("bmh_inflate_members_device: null argument"); return BMH_EINVAL; }
	hipLaunchKernelGGL(inf_members, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, d_in, in_bytes, d_tab, n, d_out, out_bytes, d_status);
	const hipError_t e = hipGetLastError();
	if (e != hipSuccess) { bmh_set_error("bmh_inflate_members_device: launch failed: %s", hipGetErrorString(e)); return BMH_ENODEV; }
	return BMH_OK;
}

extern "C" const char *bmh_inflate_status_name(uint32_t status) { return inf_what(status); }

extern "C" int bmh_inflate_members_host(const uint8_t *in, uint64_t in_bytes, const bmh_inflate_member_t *tab, uint32_t n, uint8_t *out, uint64_t out_bytes, uint32_t *status, int n_threads)
{
	if (n == 0) return BMH_OK;
	if (!in || !tab || !out || !status) { bmh_set_error("bmh_inflate_members_host: null argument"); return BMH_EINVAL; }
	const unsigned T = (unsigned)std::max<int64_t>(1, std::min<int64_t>(n_threads > 0 ? n_threads : bmh_effective_cpus(), (n + 15) / 16));
	auto work = [&](unsigned t) {
		inf_host_ws_t ws;
		for (uint32_t m = t; m < n; m += T) {
			const bmh_inflate_member_t &e = tab[m];
			const uint32_t cap = e.isize < INF_MAX_OUT ? e.isize : INF_MAX_OUT;
			if (e.in_off > in_bytes || e.in_len > in_bytes - e.in_off || e.out_off > out_bytes || cap > out_bytes - e.out_off) { status[m] = INF_ETABLE; continue; }
			uint32_t got = 0;
			status[m] = (uint32_t)inf_member(ws, in + e.in_off, e.in_len, out + e.out_off, e.isize, e.crc32, &got);
		}
	};
	if (T == 1) work(0);
	else { std::vector<std::thread> th; for (unsigned t = 0; t < T; ++t) th.emplace_back(work, t); for (auto &x : th) x.join(); }
	return BMH_OK;
}

extern "C" int bmh_bgzf_inflate(const uint8_t *data, uint64_t n_bytes, int flags, uint8_t **text, uint64_t *text_bytes)
{
	const char *fn = "bmh_bgzf_inflate";
	if (!data || !text || !text_bytes) { bmh_set_error("%s: null argument", fn); return BMH_EINVAL; }
	*text = nullptr; *text_bytes = 0;
	uint64_t nm = 0, used = 0, tb = 0;
	int rc = bmh_bgzf_scan(data, n_bytes, nullptr, 0, &nm, &used, &tb);
	if (rc != BMH_OK) return rc;
	if (used != n_bytes) { bmh_set_error("%s: the gzip stream is truncated (member %llu is cut)", fn, (unsigned long long)nm); return BMH_EINVAL; }
	if (nm >= 0xFFFFFFFFull) { bmh_set_error("%s: 2^32 members", fn); return BMH_EINVAL; }
	std::vector<bmh_inflate_member_t> tab(nm);
	rc = bmh_bgzf_scan(data, n_bytes, tab.data(), nm, &nm, &used, &tb);
	if (rc != BMH_OK) return rc;
	uint8_t *o = (uint8_t *)malloc(tb + 1);
	std::vector<uint32_t> st(nm, 0);
	if (!o) { bmh_set_error("%s: out of memory (%llu bytes of text)", fn, (unsigned long long)tb); return BMH_ENOMEM; }
	if (flags & BMH_INFLATE_HOST) rc = bmh_inflate_members_host(data, n_bytes, tab.data(), (uint32_t)nm, o, tb, st.data(), 0);
	else if (nm) {
		uint8_t *d_in = nullptr, *d_out = nullptr; bmh_inflate_member_t *d_tab = nullptr; uint32_t *d_st = nullptr;
		const bool ok = hipMalloc((void **)&d_in, n_bytes + 16) == hipSuccess && hipMalloc((void **)&d_out, tb + 16) == hipSuccess &&
		                hipMalloc((void **)&d_tab, nm * sizeof(bmh_inflate_member_t)) == hipSuccess && hipMalloc((void **)&d_st, nm * 4) == hipSuccess;
		hipError_t e = ok ? hipSuccess : hipErrorOutOfMemory;
		if (e == hipSuccess) e = hipMemcpy(d_in, data, n_bytes, hipMemcpyHostToDevice);
		if (e == hipSuccess) e = hipMemcpy(d_tab, tab.data(), nm * sizeof(bmh_inflate_member_t), hipMemcpyHostToDevice);
		if (e == hipSuccess) { rc = bmh_inflate_members_device(d_in, n_bytes, d_tab, (uint32_t)nm, d_out, tb, d_st, nullptr); if (rc == BMH_OK) e = hipDeviceSynchronize(); }
		if (e == hipSuccess && rc == BMH_OK && tb) e = hipMemcpy(o, d_out, tb, hipMemcpyDeviceToHost);
		if (e == hipSuccess && rc == BMH_OK) e = hipMemcpy(st.data(), d_st, nm * 4, hipMemcpyDeviceToHost);
		(void)hipFree(d_in); (void)hipFree(d_out); (void)hipFree(d_tab); (void)hipFree(d_st);
		if (e != hipSuccess) { (void)hipGetLastError(); bmh_set_error("%s: %s", fn, hipGetErrorString(e)); rc = BMH_ENODEV; }
	}
	if (rc != BMH_OK) { free(o); return rc; }
	for (uint64_t m = 0; m < nm; ++m)
		if (st[m] != INF_OK) { free(o); bmh_set_error("%s: damaged BGZF member %llu (%s)", fn, (unsigned long long)m, inf_what(st[m])); return BMH_EINVAL; }
	o[tb] = 0;
	*text = o; *text_bytes = tb;
	return BMH_OK;
}
