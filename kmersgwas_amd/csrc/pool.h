// pool.h — the persistent worker pool of the association scan's host side: the dense fill's columns, the streaming replay's
// worker loops and kgwas_scan_finish's batches run on it (scan_replay.cpp, scan_gpu.cpp, scan_api.cpp).
#pragma once
#include <atomic>
#include <condition_variable>
#include <exception>
#include <functional>
#include <mutex>
#include <system_error>
#include <thread>
#include <vector>

#include <pthread.h>

#include "common.h"

namespace kgwas {

// Minimal persistent worker pool: parallel_for over phenotype columns. The caller does not take part: it
// sleeps until the workers are done, so exactly size() threads are busy (sized to the CPU quota).
class Pool {
   public:
    // cpus: optional CPU to pin worker i to (empty = leave placement to the scheduler).
    explicit Pool(unsigned n, const std::vector<std::vector<int>>& cpus = {})
        : stop_(false), gen_(0), n_items_(0) {
        if (n < 1) n = 1;
        for (unsigned i = 0; i < n; i++) {
            const std::vector<int> mine = i < cpus.size() ? cpus[i] : std::vector<int>();
            try {
                th_.emplace_back([this, i, mine] {
                    kgwas_name_this_thread("kgwas-replay");
                    if (!mine.empty()) {
                        cpu_set_t set;
                        CPU_ZERO(&set);
                        for (int c : mine)
                            if (c >= 0 && c < CPU_SETSIZE) CPU_SET(c, &set);
                        (void)pthread_setaffinity_np(pthread_self(), sizeof(set), &set);
                    }
                    loop(i);
                });
            } catch (const std::system_error&) {
                // no more threads to be had: the pool is the workers that exist (items are claimed, not assigned, so any
                // number of workers runs them all); with none at all the session cannot be built
                if (th_.empty()) throw;
                break;
            }
        }
    }
    ~Pool() {
        {
            std::unique_lock<std::mutex> lk(mu_);
            stop_ = true;
            gen_++;
        }
        cv_.notify_all();
        for (auto& t : th_) t.join();
    }
    // Static assignment: item i always runs on worker i % size(), so a phenotype column's heap
    // (~320 KB at N = 10001) stays in one core's cache from chunk to chunk.
    void parallel_for(size_t n, const std::function<void(size_t)>& fn) {
        if (n == 0) return;
        start(n, fn);
        wait();
        rethrow();
    }
    // An item that throws (an allocation that fails) ends its worker's turn; the first such exception is kept until the next
    // start() and rethrown here: by parallel_for itself, and by callers of start()/wait() once they are on their normal path.
    void rethrow() {
        std::exception_ptr e;
        {
            std::unique_lock<std::mutex> lk(mu_);
            e = err_;
            err_ = nullptr;
        }
        if (e) std::rethrow_exception(e);
    }
    // The two halves of parallel_for: start() hands the items out and returns, wait() blocks until every ITEM is done - not
    // until every worker has looked in: on a shared host a worker that was asleep may get its CPU milliseconds late, and its
    // items are long done by the others (they are claimed, not assigned) - the dense fill of a headline step, 1.4 ms of work,
    // took 6-9 ms in one step of twenty on such boxes while wait() counted workers. Between the two the workers run on their own
    // (the streaming replay: items are worker loops that end when told to). fn must stay alive until wait() returns; one start
    // at a time.
    void start(size_t n, const std::function<void(size_t)>& fn) {
        std::unique_lock<std::mutex> lk(mu_);
        // (a worker of the previous start that woke late may still be walking the claim flags - it finds nothing - before they
        // are reset: workers enter run() under mu_, so none slips in behind this check)
        while (in_run_.load(std::memory_order_acquire) != 0) {
            lk.unlock();
            __builtin_ia32_pause();
            lk.lock();
        }
        fn_ = &fn;
        n_items_ = n;
        if (claimed_.size() < n) claimed_ = std::vector<std::atomic<uint8_t>>(n);
        for (size_t i = 0; i < n; i++) claimed_[i].store(0, std::memory_order_relaxed);
        left_.store(n, std::memory_order_relaxed);
        err_ = nullptr;
        done_.store(n == 0 ? 1 : 0, std::memory_order_relaxed);
        gen_.fetch_add(1, std::memory_order_release);
        lk.unlock();
        cv_.notify_all();
    }
    void wait(bool spin = true) {
        for (int sp = 0; spin && sp < 20000; sp++) {  // replays take a few ms at most: spin before sleeping
            if (done_.load(std::memory_order_acquire)) break;
            __builtin_ia32_pause();
        }
        std::unique_lock<std::mutex> lk(mu_);
        done_cv_.wait(lk, [this] { return done_.load(std::memory_order_acquire) != 0; });
    }
    size_t size() const { return th_.size(); }
    bool finished() const { return done_.load(std::memory_order_acquire) != 0; }  // every started item has run

   private:
    // Own items first, in increasing order; then take whatever nobody has started yet, from the far end
    // (with 101 columns on 16 workers the five workers that own a seventh column give it away to a worker
    // that is done with its six). An item runs exactly once, on one thread; one that throws (an allocation that fails) is
    // done all the same, and the first such exception is kept for rethrow().
    void item(size_t i) {
        try {
            (*fn_)(i);
        } catch (...) {
            std::unique_lock<std::mutex> lk(mu_);
            if (!err_) err_ = std::current_exception();
        }
        if (left_.fetch_sub(1, std::memory_order_acq_rel) == 1) {
            std::unique_lock<std::mutex> lk(mu_);
            done_.store(1, std::memory_order_release);
            done_cv_.notify_all();
        }
    }
    void run(size_t me) {
        const size_t T = th_.size();
        for (size_t i = me; i < n_items_; i += T)
            if (!claimed_[i].exchange(1, std::memory_order_acq_rel)) item(i);
        for (size_t i = n_items_; i-- > 0;)
            if (!claimed_[i].load(std::memory_order_relaxed) && !claimed_[i].exchange(1, std::memory_order_acq_rel)) item(i);
    }
    void loop(size_t me) {
        uint64_t seen = 0;
        for (;;) {
            // Chunks arrive every few milliseconds while a scan is running: spin briefly before
            // sleeping so the wake-up does not cost a futex round trip per worker per chunk.
            bool got = false;
            for (int spin = 0; spin < 4000; spin++) {
                if (gen_.load(std::memory_order_acquire) != seen) {
                    got = true;
                    break;
                }
                __builtin_ia32_pause();
            }
            {
                std::unique_lock<std::mutex> lk(mu_);
                if (!got) cv_.wait(lk, [&] { return gen_.load(std::memory_order_acquire) != seen; });
                seen = gen_.load(std::memory_order_acquire);
                if (stop_) return;
                in_run_.fetch_add(1, std::memory_order_acq_rel);  // (under mu_: start() looks at it there)
            }
            run(me);
            in_run_.fetch_sub(1, std::memory_order_acq_rel);
        }
    }
    std::vector<std::thread> th_;
    std::mutex mu_;
    std::condition_variable cv_, done_cv_;
    bool stop_;
    std::atomic<uint64_t> gen_;
    std::atomic<int> done_{0};
    std::atomic<int> in_run_{0};      // workers between the claim of their first item and their last look at the flags
    std::atomic<size_t> left_{0};     // items of the current start that have not finished
    std::vector<std::atomic<uint8_t>> claimed_;
    const std::function<void(size_t)>* fn_ = nullptr;
    size_t n_items_;
    std::exception_ptr err_;  // the first exception an item of the current start() threw (guarded by mu_)
};

}  // namespace kgwas
