// Host-side plumbing shared by the stages of libbwamem_hip.so ("Host-side memory conventions"): the growth rule and the
// per-(device, stream) scratch registry, which need no HIP (tests/devmem_host.cpp builds them with a plain C++ compiler: it defines
// BMH_DEVMEM_NO_HIP), then the error checks, the grow-only device / pinned buffers and the rocprim temp-size queries.
#pragma once
#include <stddef.h>
#include <map>
#include <memory>
#include <mutex>
#include <utility>

// THE growth rule: a buffer asked for n elements gets a quarter more and 1024, so that batches of slowly growing size do not
// reallocate every time (a reallocation frees device memory, and hipFree waits for the whole device)
constexpr size_t bmh_grow_cap(size_t n) { return n + n / 4 + 1024; }

// One T per (device, stream), created on first use.  The contract of include/bwamem_hip.h makes this enough: a stream is used by one
// host thread at a time, and released (take) while it is idle and its device current.  No HIP calls: the caller passes the device.
template <class T> class stream_scratch {
	std::mutex mu;
	std::map<std::pair<int, void *>, std::unique_ptr<T>> m;
public:
	T &get(int dev, void *stream)
	{
		std::lock_guard<std::mutex> lk(mu);
		std::unique_ptr<T> &u = m[std::make_pair(dev, stream)];
		if (!u) u.reset(new T());
		return *u;
	}
	// the entry leaves the registry; it dies with the returned pointer (null: there was none)
	std::unique_ptr<T> take(int dev, void *stream)
	{
		std::lock_guard<std::mutex> lk(mu);
		auto it = m.find(std::make_pair(dev, stream));
		if (it == m.end()) return nullptr;
		std::unique_ptr<T> u = std::move(it->second);
		m.erase(it);
		return u;
	}
};

#ifndef BMH_DEVMEM_NO_HIP
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include "bmh_internal.h"

// a file whose messages carry a prefix ("index build: ") defines BMH_CK_PREFIX before the include
#ifndef BMH_CK_PREFIX
#define BMH_CK_PREFIX ""
#endif
// (the failure is reported here: the runtime's last-error word is cleared, so that a later hipGetLastError() check does not report it again)
inline int bmh_hip_failed(const char *prefix, hipError_t e, const char *what)
{
	bmh_set_error("%s%s: %s", prefix, what, hipGetErrorString(e));
	(void)hipGetLastError();
	return BMH_ENODEV;
}
// a failed HIP call sets the message and returns BMH_ENODEV; a non-OK BMH_* code is returned unchanged
#define HIPCK(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) return bmh_hip_failed(BMH_CK_PREFIX, e_, #x); } while (0)
#define RCK(x) do { const int rc_ = (x); if (rc_ != BMH_OK) return rc_; } while (0)

// Device (dev_buf) / pinned host (pin_buf) buffers that only ever grow: need(n) keeps a buffer of at least n elements (the contents
// do not survive a growth: the old buffer is freed BEFORE the new one is allocated), resize(c) one of exactly c.
template <class T, bool PINNED> struct grow_buf {
	T *p = nullptr; size_t cap = 0;
	grow_buf() = default;
	grow_buf(const grow_buf &) = delete;
	grow_buf &operator=(const grow_buf &) = delete;
	template <class U> U *as() const { return (U *)p; }
	void swap(grow_buf &o) { std::swap(p, o.p); std::swap(cap, o.cap); }
	void drop() { if (p) (void)(PINNED ? hipHostFree(p) : hipFree(p)); p = nullptr; cap = 0; }
	int resize(size_t c)
	{
		drop();
		if ((PINNED ? hipHostMalloc((void **)&p, c * sizeof(T), hipHostMallocDefault) : hipMalloc((void **)&p, c * sizeof(T))) != hipSuccess) {
			bmh_set_error("%zu bytes of %s memory: %s", c * sizeof(T), PINNED ? "pinned" : "device", hipGetErrorString(hipGetLastError()));
			p = nullptr; return BMH_ENOMEM;
		}
		cap = c;
		return BMH_OK;
	}
	int need(size_t n) { return n <= cap ? BMH_OK : resize(bmh_grow_cap(n)); }
	~grow_buf() { drop(); }
};
template <class T> using dev_buf = grow_buf<T, false>;
template <class T> using pin_buf = grow_buf<T, true>;

// bytes of temporary storage rocprim asks for (the nullptr query) plus the 256 bytes of slack every caller adds
// (INCLUSIVE is a template argument: a run-time flag would instantiate the kernels of both scans in every file that asks)
template <class In, class Out, bool INCLUSIVE = false> inline size_t scan_tmp_bytes(size_t n)
{
	size_t t = 0;
	if constexpr (INCLUSIVE) (void)rocprim::inclusive_scan(nullptr, t, (In *)nullptr, (Out *)nullptr, n, rocprim::plus<Out>(), 0);
	else (void)rocprim::exclusive_scan(nullptr, t, (In *)nullptr, (Out *)nullptr, Out(0), n, rocprim::plus<Out>(), 0);
	return t + 256;
}
template <class T> inline size_t max_scan_tmp_bytes(size_t n)
{
	size_t t = 0;
	(void)rocprim::inclusive_scan(nullptr, t, (T *)nullptr, (T *)nullptr, n, rocprim::maximum<T>(), 0);
	return t + 256;
}
template <class K, class V> inline size_t sort_pairs_tmp_bytes(size_t n)
{
	size_t t = 0;
	(void)rocprim::radix_sort_pairs(nullptr, t, (K *)nullptr, (K *)nullptr, (V *)nullptr, (V *)nullptr, n, 0, 8 * sizeof(K), 0);
	return t + 256;
}
#endif
