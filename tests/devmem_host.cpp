// The HIP-free part of csrc/devmem.h as plain C++ for tests/test_devmem.py, built once with -fsanitize=address,undefined and once with -fsanitize=thread:
// the growth rule of every buffer and the per-(device, stream) scratch registry with a payload that counts its constructions and destructions.
// Prints "ok" and returns 0, or says what failed.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>
#define BMH_DEVMEM_NO_HIP
#include "../bwa-mem_gpu_amd/csrc/devmem.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "devmem_host: line %d: %s\n", __LINE__, #x); exit(1); } } while (0)

// the rule every stage wrote out by hand: a quarter more than asked and 1024
static_assert(bmh_grow_cap(0) == 1024, "growth rule at 0");
static_assert(bmh_grow_cap(1) == 1 + 1 / 4 + 1024, "growth rule at 1");
static_assert(bmh_grow_cap(1023) == 1023 + 1023 / 4 + 1024, "growth rule at 1023");
static_assert(bmh_grow_cap((size_t)1 << 32) == ((size_t)1 << 32) + ((size_t)1 << 30) + 1024, "growth rule at 2^32");
static_assert(bmh_grow_cap((size_t)1 << 62) == ((size_t)1 << 62) + ((size_t)1 << 60) + 1024, "growth rule at 2^62: no overflow");

static std::atomic<int> g_made{0}, g_gone{0};
struct payload_t {
	int v = 0; void *p = nullptr;        // (value-initialised by the registry)
	payload_t() { ++g_made; }
	~payload_t() { ++g_gone; }
	payload_t(const payload_t &) = delete;
};

static void *stream_of(uintptr_t k) { return (void *)(k * 64); }

static void test_growth()
{
	for (int s = 0; s <= 62; ++s)
		for (size_t n : {((size_t)1 << s) - 1, (size_t)1 << s, ((size_t)1 << s) + 3}) {
			if (n > (size_t)1 << 62) continue;
			const size_t c = bmh_grow_cap(n);
			CHECK(c == n + n / 4 + 1024 && c > n && c - n == n / 4 + 1024);
		}
}

static void test_registry()
{
	stream_scratch<payload_t> reg;
	payload_t &a = reg.get(0, stream_of(1));
	CHECK(g_made == 1 && a.v == 0 && a.p == nullptr);
	a.v = 7;
	CHECK(&reg.get(0, stream_of(1)) == &a && g_made == 1 && reg.get(0, stream_of(1)).v == 7);      // the same key: the same object
	payload_t &b = reg.get(0, stream_of(2)), &c = reg.get(1, stream_of(1)), &d = reg.get(0, nullptr);  // another stream, another device, the null stream
	CHECK(&b != &a && &c != &a && &c != &b && &d != &a && &d != &b && &d != &c && g_made == 4 && g_gone == 0);
	CHECK(!reg.take(2, stream_of(1)) && !reg.take(0, stream_of(3)) && g_gone == 0);                    // unknown keys: null, nothing destroyed
	{
		std::unique_ptr<payload_t> t = reg.take(0, stream_of(1));
		CHECK(t.get() == &a && t->v == 7 && g_gone == 0);                                              // it lives as long as the caller holds it
	}
	CHECK(g_gone == 1);
	CHECK(!reg.take(0, stream_of(1)) && g_gone == 1);                                                  // exactly one entry left, exactly once
	CHECK(&reg.get(0, stream_of(2)) == &b && &reg.get(1, stream_of(1)) == &c && &reg.get(0, nullptr) == &d && g_made == 4);
	payload_t &a2 = reg.get(0, stream_of(1));                                                          // a recycled handle starts from a fresh payload
	CHECK(g_made == 5 && a2.v == 0);
	CHECK(reg.take(0, stream_of(2)) && reg.take(1, stream_of(1)) && reg.take(0, nullptr));              // (the three die at the end of the statement)
	CHECK(g_gone == 4);
	// (a2 is still registered: the registry's own end destroys it)
}

// eight threads create the scratch of their own streams while eight others release streams created before
static void test_threads()
{
	const int made0 = g_made, gone0 = g_gone;
	{
		stream_scratch<payload_t> reg;
		const int T = 8, K = 200;
		for (int t = 0; t < T; ++t) for (int k = 0; k < K; ++k) reg.get(1, stream_of(1000 * (T + t) + k)).v = k;
		std::atomic<int> taken{0}, bad{0};
		std::vector<std::thread> th;
		for (int t = 0; t < T; ++t) {
			th.emplace_back([&, t] {
				for (int k = 0; k < K; ++k) {
					payload_t &p = reg.get(1, stream_of(1000 * t + k));
					if (p.v != 0) ++bad;
					p.v = k + 1;
					if (&reg.get(1, stream_of(1000 * t + k)) != &p || p.v != k + 1) ++bad;
				}
			});
			th.emplace_back([&, t] {
				for (int k = 0; k < K; ++k) {
					std::unique_ptr<payload_t> p = reg.take(1, stream_of(1000 * (T + t) + k));
					if (!p || p->v != k) ++bad; else ++taken;
					if (reg.take(1, stream_of(1000 * (T + t) + k))) ++bad;
				}
			});
		}
		for (auto &x : th) x.join();
		CHECK(bad == 0 && taken == T * K);
		CHECK(g_made - made0 == 2 * T * K && g_gone - gone0 == T * K);
		for (int t = 0; t < T; t += 2) for (int k = 0; k < K; ++k) CHECK(reg.take(1, stream_of(1000 * t + k)));
		CHECK(g_gone - gone0 == T * K + T / 2 * K);
	}
	CHECK(g_made - made0 == g_gone - gone0);           // the rest went with the registry
}

int main()
{
	test_growth();
	test_registry();
	CHECK(g_made == 5 && g_gone == 5);
	test_threads();
	CHECK(g_made == g_gone);
	printf("ok\n");
	return 0;
}
