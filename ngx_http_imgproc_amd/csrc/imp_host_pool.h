// imp_host_pool.h -- a few helper threads for the host's per-file work of a BATCH (never started by single-file calls): the
// JPEG batch's unstuffing / entropy preparation (imp_jpeg_api.cpp) and the PNG batch's inflates (imp_png.hip) share ONE pool
// per process (the function-local static of an inline function is one object across the library's objects).
#pragma once
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdlib>
#include <deque>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace imp {

class HostPool {
public:
    // (never destroyed: its threads sleep on the condition variable for life, and destroying a condition variable that has
    // waiters blocks -- a static instance made every process that had run a batch hang in its exit handlers)
    static HostPool& get() { static HostPool* p = new HostPool(); return *p; }
    int helpers() const { return (int)threads_.size(); }
    // runs fn(items[k]) for every k, the caller taking part; returns when all are done
    template <class Fn>
    void run(const std::vector<int>& items, Fn& fn) {
        std::atomic<size_t> next{0}, done{0};
        const size_t n = items.size();
        auto work = [&]() {
            for (;;) {
                const size_t k = next.fetch_add(1, std::memory_order_relaxed);
                if (k >= n) break;
                fn(items[k]);
                done.fetch_add(1, std::memory_order_release);
            }
        };
        std::function<void()> job = work;
        {
            std::lock_guard<std::mutex> lk(mu_);
            const int want = (int)std::min<size_t>(threads_.size(), n > 1 ? n - 1 : 0);
            for (int i = 0; i < want; i++) queue_.push_back(&job);
        }
        cv_.notify_all();
        work();
        // helpers that took the job but found nothing left have touched nothing of ours; those in the middle of an item are waited for
        while (done.load(std::memory_order_acquire) < n) std::this_thread::yield();
        std::unique_lock<std::mutex> lk(mu_);
        for (auto it = queue_.begin(); it != queue_.end();) it = (*it == &job) ? queue_.erase(it) : it + 1;
        idle_.wait(lk, [&] { return running_ == 0 || !uses(&job); });
    }
private:
    HostPool() {
        const char* s = std::getenv("IMPGPU_HOST_THREADS");
        unsigned hw = std::thread::hardware_concurrency();
        int n = s ? std::atoi(s) : (int)std::min(3u, hw / 8);              // helpers beside the caller
        if (n < 0) n = 0;
        if (n > 15) n = 15;
        for (int i = 0; i < n; i++) threads_.emplace_back([this] { loop(); });
        for (auto& t : threads_) t.detach();
    }
    bool uses(std::function<void()>* j) const { for (auto* c : current_) if (c == j) return true; return false; }
    void loop() {
        for (;;) {
            std::function<void()>* job = nullptr;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return !queue_.empty(); });
                job = queue_.front();
                queue_.pop_front();
                current_.push_back(job);
                running_++;
            }
            (*job)();
            {
                std::lock_guard<std::mutex> lk(mu_);
                running_--;
                for (auto it = current_.begin(); it != current_.end(); ++it) if (*it == job) { current_.erase(it); break; }
            }
            idle_.notify_all();
        }
    }
    std::mutex mu_;
    std::condition_variable cv_, idle_;
    std::deque<std::function<void()>*> queue_;
    std::vector<std::function<void()>*> current_;
    std::vector<std::thread> threads_;
    int running_ = 0;
};

template <class Fn>
void host_parallel(const std::vector<int>& items, size_t bytes, Fn& fn) {
    if (items.size() >= 4 && bytes >= (size_t(256) << 10) && HostPool::get().helpers() > 0) HostPool::get().run(items, fn);
    else for (int i : items) fn(i);
}

}  // namespace imp
