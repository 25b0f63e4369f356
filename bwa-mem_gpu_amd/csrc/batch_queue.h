// The loader's side of a run from read files (csrc/align_pipeline.hip: run_loaded): a loader thread fills batch buffers ahead of the lanes, the lanes take them in
// order, the writer gives them back.  Plain C++17: tests/batch_queue_host.cpp runs it without a device.
//   B: the batch buffer; the queue sets B::index (uint32_t), the batch's number in the run.  The buffers live in `all`, the caller's (kept between runs); at most
//      `cap` of them ever exist: the loader is that far ahead and no further.
//   fill(B &, err) on the loader thread: 1 = the buffer holds the next batch, 0 = the end of the input, < 0 = refused (err: the message).  A refusal reaches the
//      consumers through next() behind the batches before it -- at once, or, with after_release, only when every batch handed out has been released.
#ifndef BMH_BATCH_QUEUE_H
#define BMH_BATCH_QUEUE_H
#include <condition_variable>
#include <cstdint>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

template <class B> class batch_queue_t {
public:
	typedef std::function<int(B &, std::string &)> fill_t;
	typedef std::function<int(std::string &)> prologue_t;          // first on the loader thread (0, or a code and its message): the thread's device
	batch_queue_t(std::vector<std::unique_ptr<B>> &all_, int cap_, bool after_release_) : all(all_), cap(cap_), after_release(after_release_) { for (auto &b : all) free_list.push_back(b.get()); }
	~batch_queue_t() { join(); }
	void start(fill_t fill, prologue_t prologue = nullptr) { loader = std::thread([this, fill, prologue] { load(fill, prologue); }); }
	// 1: *out is the next batch in index order, 0: no more (the end of the input, or stop()), < 0: the loader's refusal (err: its message); thread-safe, may block
	int next(B **out, std::string &err)
	{
		std::unique_lock<std::mutex> lk(mu);
		cv.wait(lk, [&] { return stopped || ready.count(next_out) || eof; });
		if (!stopped && !ready.count(next_out) && load_rc != 0 && after_release) cv.wait(lk, [&] { return stopped || outstanding == 0; });
		if (stopped) return 0;
		if (!ready.count(next_out)) { err = load_err; return load_rc; }
		*out = ready[next_out]; ready.erase(next_out); ++next_out; ++outstanding;
		return 1;
	}
	void release(B *b) { if (!b) return; std::lock_guard<std::mutex> lk(mu); free_list.push_back(b); --outstanding; cv.notify_all(); }      // a batch next() handed out
	void stop() { std::lock_guard<std::mutex> lk(mu); stopped = true; cv.notify_all(); }      // unblocks next() and a loader waiting for a buffer
	void join() { if (loader.joinable()) { stop(); loader.join(); } }
	size_t n_free() { std::lock_guard<std::mutex> lk(mu); return free_list.size(); }

private:
	void load(const fill_t &fill, const prologue_t &prologue)
	{
		std::string err;
		int rc = prologue ? prologue(err) : 0;
		for (uint32_t index = 0; rc == 0;) {
			B *b = nullptr;
			{
				std::unique_lock<std::mutex> lk(mu);
				cv.wait(lk, [&] { return stopped || !free_list.empty() || (int)all.size() < cap; });
				if (stopped) break;
				if (!free_list.empty()) { b = free_list.back(); free_list.pop_back(); }
				else { all.emplace_back(new B()); b = all.back().get(); }
			}
			rc = fill(*b, err);
			std::lock_guard<std::mutex> lk(mu);
			if (rc != 1) { free_list.push_back(b); break; }
			b->index = index++; ready[b->index] = b; rc = 0;
			cv.notify_all();
		}
		std::lock_guard<std::mutex> lk(mu);
		if (rc < 0) { load_rc = rc; load_err = err; }
		eof = true;
		cv.notify_all();
	}
	std::vector<std::unique_ptr<B>> &all; const int cap; const bool after_release;
	std::mutex mu; std::condition_variable cv;
	std::vector<B *> free_list; std::map<uint32_t, B *> ready;
	uint32_t next_out = 0; int outstanding = 0; bool eof = false, stopped = false;
	int load_rc = 0; std::string load_err;
	std::thread loader;
};
#endif
