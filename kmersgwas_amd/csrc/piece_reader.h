// piece_reader.h — the reader thread behind a streaming pass over a k-mers table: lmm_table.cpp's table_pass and proxy.cpp's
// search take their pieces of rows from it.
#pragma once
#include <algorithm>
#include <condition_variable>
#include <exception>
#include <mutex>
#include <thread>

#include "device.h"

namespace kgwas {

// The reader of a table pass: its thread fills two pinned row buffers in turn, piece k going into buffer k & 1 once piece k - 2
// has left it, while the device works on the piece before. The consumer takes piece k with wait(k), which rethrows what a failed
// read threw, and hands its buffer back with release(k). The destructor stops the thread and joins it.
class PieceReader {
  public:
    PieceReader(kgwas_table* t, uint64_t n_rows, uint64_t piece, uint64_t stride) : t_(t), n_rows_(n_rows), piece_(piece) {
        for (PinBuf<uint64_t>& b : rows_) b.alloc(piece * stride);
        thread_ = std::thread([this] { fill(); });
    }
    ~PieceReader() {
        {
            std::unique_lock<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        if (thread_.joinable()) thread_.join();
    }
    const uint64_t* wait(uint64_t k) {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return stop_ || filled_ > k; });
        if (filled_ <= k) std::rethrow_exception(err_);  // (only the reader's failure stops it before the consumer is done)
        return rows_[k & 1].p;
    }
    void release(uint64_t k) {
        {
            std::unique_lock<std::mutex> lk(mu_);
            consumed_ = k + 1;
        }
        cv_.notify_all();
    }

  private:
    void fill() {
        kgwas_name_this_thread("kgwas-lmm-read");
        try {
            for (uint64_t k = 0; k * piece_ < n_rows_; k++) {
                {
                    std::unique_lock<std::mutex> lk(mu_);
                    cv_.wait(lk, [&] { return stop_ || consumed_ + 2 > k; });
                    if (stop_) return;
                }
                const uint64_t pos = k * piece_;
                if (kgwas_table_read_rows(t_, pos, std::min(piece_, n_rows_ - pos), rows_[k & 1].p) != KGWAS_OK)
                    throw Error(KGWAS_ERR_IO, kgwas_last_error());
                {
                    std::unique_lock<std::mutex> lk(mu_);
                    filled_ = k + 1;
                }
                cv_.notify_all();
            }
        } catch (...) {
            std::unique_lock<std::mutex> lk(mu_);
            err_ = std::current_exception();
            stop_ = true;
            cv_.notify_all();
        }
    }
    kgwas_table* const t_;
    const uint64_t n_rows_, piece_;
    PinBuf<uint64_t> rows_[2];
    std::mutex mu_;
    std::condition_variable cv_;
    uint64_t filled_ = 0, consumed_ = 0;
    bool stop_ = false;
    std::exception_ptr err_;
    std::thread thread_;
};

}  // namespace kgwas
