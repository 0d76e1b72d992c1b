// device.h — the owners of HIP resources on the host side of libkgwas: device memory, streams, events, the squeeze's column map, the
// r^2 kernels' operands, and the one device check.
//
// Teardown order is declaration order, reversed. A Stream's destructor synchronises before it destroys, so an owner declares the
// pinned and device buffers a stream's work reads BEFORE the stream: the stream goes first, idle, and the buffers after it.
#pragma once
#include <sys/mman.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <thread>
#include <vector>

#include "common.h"
#include "kernels.h"

namespace kgwas {

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) {
        o.p = nullptr;
        o.n = 0;
    }
    void alloc(size_t count) {
        release();
        if (count) KGWAS_HIP(hipMalloc((void**)&p, count * sizeof(T)));
        n = count;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    ~DevBuf() { release(); }
};

// Pinned, device-mapped host memory. hipHostMalloc costs 0.16 s per GiB (it faults and zeroes 4 KiB pages one by one; a
// fresh `associate_kmers` spent 0.17 of its 0.52 s there): large buffers are mapped with MADV_HUGEPAGE, touched by a few
// threads and registered instead - 5 ms per 512 MiB where transparent huge pages are available (16x), ~45 ms where they
// are not - and fall back to hipHostMalloc if any step fails (KGWAS_PIN_PLAIN=1 forces that).
struct PinRegion {
    void* p = nullptr;       // what the caller uses
    void* map = nullptr;     // the mapping it lies in (registered memory), nullptr: hipHostMalloc
    size_t map_bytes = 0;
    static constexpr size_t HUGE = 2u << 20;
    void alloc(size_t bytes) {
        release();
        if (!bytes) return;
        static const bool plain = opt_set("KGWAS_PIN_PLAIN");
        if (!plain && bytes >= (8u << 20)) {
            const size_t len = (bytes + HUGE - 1) / HUGE * HUGE;
            void* m = mmap(nullptr, len + HUGE, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
            if (m != MAP_FAILED) {
                char* al = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(m) + HUGE - 1) & ~(uintptr_t)(HUGE - 1));
                (void)madvise(al, len, MADV_HUGEPAGE);
                {
                    // touched in segments of 32 MiB by up to 8 threads (this one among them; fewer if no more are to be had)
                    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
                    const size_t seg = 32u << 20, n_seg = (len + seg - 1) / seg;
                    const unsigned nt = (unsigned)std::min<size_t>(std::min<size_t>(8, hw), n_seg);
                    std::atomic<size_t> next(0);
                    kgwas_run_on_threads(nt, "kgwas-touch", [&] {
                        for (size_t i; (i = next.fetch_add(1, std::memory_order_relaxed)) < n_seg;)
                            for (size_t o = i * seg, b = std::min(len, (i + 1) * seg); o < b; o += 4096) al[o] = 0;
                    });
                }
                if (hipHostRegister(al, len, hipHostRegisterMapped) == hipSuccess) {
                    p = al;
                    map = m;
                    map_bytes = len + HUGE;
                    return;
                }
                (void)hipGetLastError();  // (not sticky: the plain allocation below is the answer)
                munmap(m, len + HUGE);
            }
        }
        KGWAS_HIP(hipHostMalloc(&p, bytes, hipHostMallocMapped));
    }
    void release() {
        if (map) {
            (void)hipHostUnregister(p);
            munmap(map, map_bytes);
        } else if (p)
            (void)hipHostFree(p);
        p = map = nullptr;
        map_bytes = 0;
    }
};
template <class T>
struct PinBuf {
    T* p = nullptr;
    size_t n = 0;
    PinRegion r;
    PinBuf() = default;
    PinBuf(const PinBuf&) = delete;
    PinBuf& operator=(const PinBuf&) = delete;
    PinBuf(PinBuf&& o) noexcept : p(o.p), n(o.n), r(o.r) {
        o.p = nullptr;
        o.n = 0;
        o.r = PinRegion();
    }
    void alloc(size_t count) {
        release();
        r.alloc(count * sizeof(T));
        p = static_cast<T*>(r.p);
        n = count;
    }
    T* dev() const {
        T* d = nullptr;
        if (p) KGWAS_HIP(hipHostGetDevicePointer((void**)&d, p, 0));
        return d;
    }
    void release() {
        r.release();
        p = nullptr;
        n = 0;
    }
    ~PinBuf() { release(); }
};

// A stream of its own. The destructor waits for the stream's work, then destroys it.
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    Stream(Stream&& o) noexcept : s(o.s) { o.s = nullptr; }
    Stream& operator=(Stream&& o) noexcept {
        if (this != &o) release(), s = o.s, o.s = nullptr;
        return *this;
    }
    void create(unsigned flags) {
        release();
        KGWAS_HIP(hipStreamCreateWithFlags(&s, flags));
    }
    void create_with_priority(unsigned flags, int priority) {
        release();
        KGWAS_HIP(hipStreamCreateWithPriority(&s, flags, priority));
    }
    void release() {
        if (s) (void)hipStreamSynchronize(s), (void)hipStreamDestroy(s);
        s = nullptr;
    }
    operator hipStream_t() const { return s; }
    ~Stream() { release(); }
};

struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
    Event& operator=(Event&& o) noexcept {
        if (this != &o) release(), e = o.e, o.e = nullptr;
        return *this;
    }
    void create(unsigned flags = hipEventDefault) {
        release();
        KGWAS_HIP(hipEventCreateWithFlags(&e, flags));
    }
    void release() {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
    operator hipEvent_t() const { return e; }
    ~Event() { release(); }
};

// One upload lane: two pinned blocks that take turns, a stream of its own, and per block a blocking event that says its last copy
// is through (blocking: a thread that has to wait for a copy sleeps). The stream is declared last, so nothing of the lane is in
// flight when its blocks go away.
template <class T>
struct UploadLane {
    PinBuf<T> h[2];
    Event ev[2];
    Stream st;
    uint64_t turn = 0;
    int cur = 0;  // the block last taken
    void create(size_t block) {
        for (int i = 0; i < 2; i++) {
            h[i].alloc(block);
            ev[i].create(hipEventDisableTiming | hipEventBlockingSync);
        }
        st.create(hipStreamNonBlocking);
    }
    // the block whose turn it is, once the copy that last left it is through
    T* take() {
        cur = (int)(turn++ & 1);
        KGWAS_HIP(hipEventSynchronize(ev[cur]));
        return h[cur].p;
    }
    // the work queued on st so far reads the block last taken
    void sent() { KGWAS_HIP(hipEventRecord(ev[cur], st)); }
};

// The squeeze of table rows to a list of the table's columns (launch_squeeze): the padded column map on the device and W_m, the
// 64-bit words of a squeezed row. Built from col[0..S), the columns in output order, and W_f, the words of a table row's bits.
struct Squeezer {
    uint32_t W_m = 0, W_f = 0;
    DevBuf<uint32_t> d_colmap;
    void create(const uint64_t* col, uint64_t S, uint64_t table_words) {
        W_m = (uint32_t)(2 * ((S + 127) / 128));  // the reference's m_hash_words, rounded to the 128-bit unit
        W_f = (uint32_t)table_words;
        std::vector<uint32_t> colmap(64ull * W_m, 0xFFFFFFFFu);
        for (uint64_t i = 0; i < S; i++) colmap[i] = (uint32_t)col[i];
        d_colmap.alloc(std::max<size_t>(colmap.size(), 1));  // (no column at all: still something to point at)
        KGWAS_HIP(hipMemcpy(d_colmap.p, colmap.data(), colmap.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    uint64_t words_per_row() const { return 2ull * W_m; }  // 32-bit words of a row of `out`
    // d_rows[count][stride] (word 0 of a row is its k-mer) -> out[count][words_per_row()]
    void run(const uint64_t* d_rows, uint64_t stride, uint64_t count, uint32_t* out, hipStream_t st) const {
        KGWAS_HIP(launch_squeeze(d_rows, stride, count, d_colmap.p, W_m, W_f, out, st));
    }
};

// The operands of the exact r^2 kernels for `pad` rows (a multiple of the kernels' tiles) over n accessions (kernels.h,
// launch_ld_prep): the owner of what an LdView points at. A view is of `count` rows padded to `pad` <= alloc's.
struct LdOperands {
    DevBuf<uint4> P;
    DevBuf<uint32_t> n1, pq;
    DevBuf<uint64_t> tq;
    uint32_t n_chunks = 0;
    void alloc(uint64_t pad, uint64_t n) {
        n_chunks = (uint32_t)((n + 511) / 512 * 4);
        P.alloc((size_t)n_chunks * pad), n1.alloc(pad), pq.alloc(pad), tq.alloc(pad);
    }
    LdView view(uint64_t count, uint64_t pad) const {
        if (pad > n1.n) throw Error(KGWAS_ERR_STATE, "LdOperands: a view of more rows than were allocated");
        return LdView{P.p, n1.p, pq.p, tq.p, count, pad, n_chunks};
    }
};

// The devices there are; throws when there is none.
inline int device_count(const char* detail = ": libkgwas has no CPU fallback") {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) throw Error(KGWAS_ERR_DEVICE, std::string("no HIP device available") + detail);
    return n;
}

// The check before an entry point first touches the GPU: a device exists, the ordinal names one, and it is made current.
inline void use_device(int device) {
    const int n = device_count();
    if (device < 0 || device >= n) throw Error(KGWAS_ERR_ARG, "device ordinal out of range");
    KGWAS_HIP(hipSetDevice(device));
}

}  // namespace kgwas
