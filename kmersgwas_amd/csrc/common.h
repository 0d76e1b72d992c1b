// common.h — error plumbing and the small helpers shared by the host side of libkgwas.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>

#include "../../include/kgwas.h"
#include "env.h"

namespace kgwas {

// Thread-local last error (kgwas_last_error()).
void set_error(const std::string& msg);

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

#define KGWAS_HIP(expr)                                                                                     \
    do {                                                                                                    \
        hipError_t _e = (expr);                                                                             \
        if (_e != hipSuccess)                                                                               \
            throw ::kgwas::Error(KGWAS_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e));      \
    } while (0)

// heap_guard.cpp: throws KGWAS_ERR_STATE unless csrc/heap.h reproduces this process's std::priority_queue (checked once).
void require_heap_emulation();

// Run body, translate exceptions into a status code + message. No exception crosses the C ABI.
template <class F>
int guarded(F&& body) {
    try {
        body();
        return KGWAS_OK;
    } catch (const Error& e) {
        set_error(e.what());
        return e.code;
    } catch (const std::bad_alloc&) {
        set_error("out of host memory");
        return KGWAS_ERR_NOMEM;
    } catch (const std::exception& e) {
        set_error(e.what());
        return KGWAS_ERR_ARG;
    }
}

inline void ck(int rc) {  // a status of the C ABI (the library calling itself) -> the Error it stands for
    if (rc != KGWAS_OK) throw Error(rc, kgwas_last_error());
}
inline double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// the whole of a text file in one write; mode is fopen's ("wb", "ab")
inline void write_text(const std::string& path, const std::string& body, const char* mode = "wb") {
    FILE* fo = fopen(path.c_str(), mode);
    const bool ok = fo && fwrite(body.data(), 1, body.size(), fo) == body.size();
    if ((fo && fclose(fo) != 0) || !ok) throw Error(KGWAS_ERR_IO, "can't write " + path);
}

// bits2kmer31 (the reference's src/kmer_general.cpp:77-87): the most significant base first; out gets kmer_len <= 32 letters, no 0
inline void kmer_letters(uint64_t word, uint32_t kmer_len, char* out) {
    for (uint32_t i = 0; i < kmer_len; i++) out[i] = "ACGT"[(word >> (2 * (kmer_len - 1 - i))) & 3];
}
inline std::string kmer_letters(uint64_t word, uint32_t kmer_len) {
    std::string s(kmer_len, 'A');
    kmer_letters(word, kmer_len, &s[0]);
    return s;
}

// an r^2 threshold in millionths as the logs spell it: 800000 -> "0.800000"
inline std::string r2_text(uint32_t r2_millionths) {
    char buf[16];
    snprintf(buf, sizeof(buf), "%u.%06u", r2_millionths / 1000000u, r2_millionths % 1000000u);
    return buf;
}

// Rows per piece of a streaming pass over a table of n_rows rows of `stride` words: about budget_bytes of rows, within 1024 ..
// max_rows, never more than the table has. The environment switch switch_name (the tests' hook) sets it, up to forced_cap.
inline uint64_t piece_rows(uint64_t n_rows, uint64_t stride, uint64_t budget_bytes, uint64_t max_rows, uint64_t forced_cap, const char* switch_name) {
    uint64_t piece = std::max<uint64_t>(1024, std::min<uint64_t>(max_rows, budget_bytes / (8 * stride)));
    const long long forced = opt_int(switch_name, 0);
    if (forced > 0) piece = std::min<uint64_t>((uint64_t)forced, forced_cap);
    return std::min(piece, std::max<uint64_t>(n_rows, 1));
}

}  // namespace kgwas

// Names the calling thread (comm, <= 15 characters): a hang report (tools/fuzz_parity.py's watchdog reads /proc/self/task) or
// a profiler then says WHICH of the library's helper threads it is looking at.
#include <pthread.h>
inline void kgwas_name_this_thread(const char* name) { (void)pthread_setname_np(pthread_self(), name); }

// Runs `work` on the calling thread and on up to n - 1 others (fewer if the system has no more threads to give), joins them all
// whatever happens and rethrows the first exception any of them left: `work` takes its items from a shared counter.
#include <exception>
#include <mutex>
#include <system_error>
#include <thread>
#include <vector>
template <class F>
void kgwas_run_on_threads(unsigned n, const char* name, F&& work) {
    std::exception_ptr err;
    std::mutex emu;
    auto guarded_work = [&](bool named) {
        try {
            if (named) kgwas_name_this_thread(name);
            work();
        } catch (...) {
            std::lock_guard<std::mutex> lk(emu);
            if (!err) err = std::current_exception();
        }
    };
    std::vector<std::thread> th;
    for (unsigned t = 1; t < n; t++) {
        try {
            th.emplace_back(guarded_work, true);
        } catch (const std::system_error&) {
            break;
        }
    }
    guarded_work(false);
    for (auto& t : th) t.join();
    if (err) std::rethrow_exception(err);
}
