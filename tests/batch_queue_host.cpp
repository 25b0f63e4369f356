// csrc/batch_queue.h as plain C++ for tests/test_batch_queue.py, built once with -fsanitize=address,undefined and once with -fsanitize=thread: the loader's queue
// of the aligner's runs from files with a dummy buffer, 1 / 2 / 4 consumer threads and fills of 0 / 1 / 50 batches.  Prints "ok" and returns 0, or says what failed.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include "../bwa-mem_gpu_amd/csrc/batch_queue.h"

struct buf_t { uint32_t index = 0; int payload = -1; };
typedef batch_queue_t<buf_t> queue_t;
typedef std::vector<std::unique_ptr<buf_t>> bufs_t;

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "batch_queue_host: line %d: %s (consumers %d, batches %d, cap %d, after_release %d)\n", __LINE__, #x, g_c, g_n, g_cap, g_ar); exit(1); } } while (0)
static int g_c, g_n, g_cap, g_ar;
static void pause_ms(int ms) { std::this_thread::sleep_for(std::chrono::milliseconds(ms)); }

// n batches, then the end -- or, refuse_at >= 0, a refusal (-7, "refused at <k>") in place of batch refuse_at
static queue_t::fill_t counting_fill(int n, int refuse_at, std::atomic<int> &made)
{
	return [n, refuse_at, &made](buf_t &b, std::string &err) {
		const int k = made.load();
		if (k == refuse_at) { err = "refused at " + std::to_string(k); return -7; }
		if (k == n) return 0;
		b.payload = k; made.store(k + 1);
		return 1;
	};
}

// every consumer takes batches until next() says 0 or refuses; a refusal stops the queue, as a failed run does.  What came out: seen[index] counts, rc / msg the refusal
struct taken_t { std::mutex mu; std::vector<int> seen; int rc = 0; std::string msg; };
static void consume(queue_t &q, taken_t &t, int n_consumers)
{
	std::vector<std::thread> th;
	for (int c = 0; c < n_consumers; ++c) th.emplace_back([&] {
		long last = -1;
		for (;;) {
			buf_t *b = nullptr; std::string err;
			const int got = q.next(&b, err);
			if (got < 0) { { std::lock_guard<std::mutex> lk(t.mu); t.rc = got; t.msg = err; } q.stop(); return; }
			if (got == 0) return;
			CHECK(b && b->payload == (int)b->index && (long)b->index > last);       // the batch the loader numbered, later than this consumer's last
			last = b->index;
			{ std::lock_guard<std::mutex> lk(t.mu); if (t.seen.size() <= b->index) t.seen.resize(b->index + 1, 0); ++t.seen[b->index]; }
			std::this_thread::yield();
			q.release(b);
		}
	});
	for (auto &x : th) x.join();
}
static void check_taken(const taken_t &t, int n) { CHECK((int)t.seen.size() == n); for (int v : t.seen) CHECK(v == 1); }

int main()
{
	for (int ar = 0; ar < 2; ++ar) for (int c : {1, 2, 4}) for (int n : {0, 1, 50}) for (int cap : {1, 3, 7}) {
		g_ar = ar; g_c = c; g_n = n; g_cap = cap;
		bufs_t all;
		for (int run = 0; run < 2; ++run) {                          // the buffers stay with the caller: a second run makes no more
			std::atomic<int> made{0}; taken_t t;
			queue_t q(all, cap, ar != 0);
			q.start(counting_fill(n, -1, made));
			consume(q, t, c);
			q.join();
			check_taken(t, n);                                       // every batch once
			CHECK(t.rc == 0 && (int)all.size() <= cap && q.n_free() == all.size());
		}
		for (int k : {0, 3}) {                                       // a refusal in place of batch k: batches 0 .. k - 1, then the code and the message
			if (k > n) continue;
			std::atomic<int> made{0}; taken_t t;
			queue_t q(all, cap, ar != 0);
			q.start(counting_fill(n, k, made));
			consume(q, t, c);
			q.join();
			check_taken(t, k);
			CHECK(t.rc == -7 && t.msg == "refused at " + std::to_string(k) && (int)all.size() <= cap && q.n_free() == all.size());
		}
	}
	// a refusal behind a batch that is held: with after_release, next() refuses only once that batch has been released; at once, it refuses while it is held
	for (int ar = 0; ar < 2; ++ar) for (int c : {1, 2, 4}) {
		g_ar = ar; g_c = c; g_n = 1; g_cap = 3;
		bufs_t all; std::atomic<int> made{0}, refusals{0}; std::atomic<bool> released{false};
		queue_t q(all, 3, ar != 0);
		q.start(counting_fill(5, 1, made));
		buf_t *held = nullptr; std::string err;
		CHECK(q.next(&held, err) == 1 && held->index == 0);
		std::vector<std::thread> th;
		for (int k = 0; k < c; ++k) th.emplace_back([&] {
			buf_t *b = nullptr; std::string e;
			const int got = q.next(&b, e);
			CHECK(got == -7 && e == "refused at 1");
			CHECK(ar == 0 || released.load());
			++refusals;
		});
		if (ar) { pause_ms(20); CHECK(refusals.load() == 0); }       // (they wait for the held batch)
		else { for (auto &x : th) x.join(); th.clear(); CHECK(refusals.load() == c); }
		released = true;
		q.release(held);
		for (auto &x : th) x.join();
		q.join();
		CHECK(refusals.load() == c && q.n_free() == all.size());
	}
	// stop() unblocks a loader that waits for a free buffer (nobody takes a batch) ...
	{
		g_c = 0; g_n = -1; g_cap = 2; g_ar = 0;
		bufs_t all; std::atomic<int> made{0};
		queue_t q(all, 2, false);
		q.start(counting_fill(1 << 30, -1, made));
		while (made.load() < 2) std::this_thread::yield();
		pause_ms(5);
		q.join();                                                    // (stop, then the thread's end)
		CHECK(made.load() == 2 && all.size() == 2);
	}
	// ... and a consumer that waits in next() while the loader is busy filling
	for (int c : {1, 2, 4}) {
		g_c = c; g_n = 1; g_cap = 3; g_ar = 0;
		bufs_t all; std::mutex mu; std::condition_variable cv; bool go = false; int made = 0;
		queue_t q(all, 3, false);
		q.start([&](buf_t &b, std::string &) { if (made == 0) { b.payload = made++; return 1; } std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return go; }); return 0; });
		taken_t t; std::thread cons([&] { consume(q, t, c); });
		for (bool taken = false; !taken; std::this_thread::yield()) { std::lock_guard<std::mutex> lk(t.mu); taken = t.seen.size() == 1; }
		pause_ms(10);                                                // (batch 0 is out; the consumers are back in next())
		q.stop();
		cons.join();                                                 // (returns although the loader has not said whether more comes)
		{ std::lock_guard<std::mutex> lk(mu); go = true; } cv.notify_all();
		q.join();
		CHECK(t.rc == 0 && t.seen.size() == 1 && q.n_free() == all.size());
	}
	printf("ok\n");
	return 0;
}
