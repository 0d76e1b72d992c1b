// heap_one_bench.cpp - ONE heap's replace-min through heap.h's BestHeap::add (the one-column scan's replay: a single thread,
// 101 k effective pushes per 100 M rows), against a literal std::priority_queue: time per push and identical pop order.
// build: g++ -O3 -std=c++17 -I kmersgwas_amd/csrc tools/heap_one_bench.cpp -o tools/bin/heap_one_bench
//
// heap_one_bench walk [N] [records] [rounds] [offset]: the hole walk of a late-tie column's replay, ONE level per load
// latency (the form heap.h had until the two-level walk) against TWO levels per load latency (children and grandchildren
// of the hole loaded together), both written out here on the same 16-byte entries with int64 compares, run alternating
// over `rounds` copies of one heap and one record stream. The stream is a column's: each record beats the heap's minimum
// with the odds the device's threshold leaves it (5 in 7; the rest fall in the 0.4 % between threshold and minimum), an
// accepted score is uniform above the minimum - N = 10001 and 140 000 records give ~10^5 effective pushes, the acceptance
// per table row falling as N / row. Then all N pops, one level against two. Both forms must leave identical arrays after
// the pushes and identical pop sequences, and the array must equal what BestHeap::add leaves (exit status 1 otherwise).
// offset: bytes added to a 64-byte aligned array base (16 puts the four grandchildren of every node into one cache line).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <queue>
#include <random>
#include <vector>

#include "heap.h"

struct QE {
    double score;
    uint64_t kmer, row;
};
struct QG {
    bool operator()(const QE& l, const QE& r) const { return l.score > r.score; }
};

namespace walk {

struct Ent {
    double score;
    uint32_t slot;
};
struct Pay {
    uint64_t kmer, row;
};
static inline int64_t key(const Ent& e) {
    int64_t k;
    memcpy(&k, &e.score, 8);
    return k;
}
static inline int64_t pick(bool c, int64_t t, int64_t f) {  // c ? t : f as arithmetic: a select, never a branch
    const int64_t m = -(int64_t)c;
    return (t & m) | (f & ~m);
}
static inline void prefetch_below(const Ent* a, ptrdiff_t c, ptrdiff_t n) {
    const ptrdiff_t d = 16 * c + 15;
    if (d + 15 < n) {
        __builtin_prefetch(a + d);
        __builtin_prefetch(a + d + 4);
        __builtin_prefetch(a + d + 8);
        __builtin_prefetch(a + d + 12);
        __builtin_prefetch(a + d + 15);
    }
}
constexpr ptrdiff_t BIG_HEAP = 1 << 16;

// pop-then-push on a full heap a[0..n), totally ordered scores: the hole stops at the first path node above `value`
template <bool TWO>
static inline void replace_top(Ent* a, ptrdiff_t n, Ent x) {
    const Ent value = a[n - 1];
    const int64_t kv = key(value);
    const ptrdiff_t len = n - 1;
    ptrdiff_t hole = 0, child = 0;
    bool open = true;
    const bool big = n > BIG_HEAP;
    if (TWO) {
        while (4 * child + 6 < len) {
            if (big) prefetch_below(a, child, n);
            const Ent* c = a + 2 * child + 1;
            const Ent* g = a + 4 * child + 3;
            const int64_t kl = key(c[0]), kr = key(c[1]);
            const int64_t k0 = key(g[0]), k1 = key(g[1]), k2 = key(g[2]), k3 = key(g[3]);
            const bool left = kr > kl;
            const ptrdiff_t dl = 4 * child + 4 - (k1 > k0 ? 1 : 0), dr = 4 * child + 6 - (k3 > k2 ? 1 : 0);
            const int64_t wl = k1 > k0 ? k0 : k1, wr = k3 > k2 ? k2 : k3;
            const ptrdiff_t cc = 2 * child + 2 - (left ? 1 : 0);
            const ptrdiff_t dd = pick(left, dl, dr);
            if (pick(left, kl, kr) > kv) {
                open = false;
                break;
            }
            if (big) prefetch_below(a, cc, n);
            a[hole] = a[cc];
            hole = child = cc;
            if (pick(left, wl, wr) > kv) {
                open = false;
                break;
            }
            a[hole] = a[dd];
            hole = child = dd;
        }
    }
    if (open) {
        while (child < (len - 1) / 2) {
            if (big) prefetch_below(a, child, n);
            ptrdiff_t cc = 2 * (child + 1);
            cc -= key(a[cc]) > key(a[cc - 1]) ? 1 : 0;
            if (key(a[cc]) > kv) {
                open = false;
                break;
            }
            a[hole] = a[cc];
            hole = child = cc;
        }
        if (open && (len & 1) == 0 && child == (len - 2) / 2) {
            const ptrdiff_t c2 = 2 * (child + 1);
            if (!(key(a[c2 - 1]) > kv)) {
                a[hole] = a[c2 - 1];
                hole = c2 - 1;
            }
        }
    }
    a[hole] = value;
    hole = n - 1;
    const int64_t kx = key(x);
    ptrdiff_t parent = (hole - 1) / 2;
    while (hole > 0 && key(a[parent]) > kx) {
        a[hole] = a[parent];
        hole = parent;
        parent = (hole - 1) / 2;
    }
    a[hole] = x;
}

// std::pop_heap minus the store of the old top: the hole walks to a leaf, `value` climbs back
template <bool TWO>
static inline void pop_top(Ent* a, ptrdiff_t n) {
    if (n <= 1) return;
    const Ent value = a[n - 1];
    const ptrdiff_t len = n - 1;
    ptrdiff_t hole = 0, child = 0;
    if (TWO) {
        while (4 * child + 6 < len) {
            const ptrdiff_t l = 2 * child + 1, g = 4 * child + 3;
            const int64_t kl = key(a[l]), kr = key(a[l + 1]);
            const int64_t k0 = key(a[g]), k1 = key(a[g + 1]), k2 = key(a[g + 2]), k3 = key(a[g + 3]);
            const bool left = kr > kl, left_l = k1 > k0, left_r = k3 > k2;
            const ptrdiff_t cc = l + 1 - (left ? 1 : 0);
            const ptrdiff_t dd = 2 * cc + 2 - pick(left, left_l, left_r);
            a[hole] = a[cc];
            a[cc] = a[dd];
            hole = child = dd;
        }
    }
    while (child < (len - 1) / 2) {
        child = 2 * (child + 1);
        child -= key(a[child]) > key(a[child - 1]) ? 1 : 0;
        a[hole] = a[child];
        hole = child;
    }
    if ((len & 1) == 0 && child == (len - 2) / 2) {
        child = 2 * (child + 1);
        a[hole] = a[child - 1];
        hole = child - 1;
    }
    const int64_t kv = key(value);
    ptrdiff_t parent = (hole - 1) / 2;
    while (hole > 0 && key(a[parent]) > kv) {
        a[hole] = a[parent];
        hole = parent;
        parent = (hole - 1) / 2;
    }
    a[hole] = value;
}

static double median(std::vector<double> v) {
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

static int run(size_t N, size_t records, int rounds, size_t offset) {
    std::mt19937_64 rng(7);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    struct Greater {
        bool operator()(const Ent& l, const Ent& r) const { return l.score > r.score; }
    };
    std::vector<Ent> start;
    for (size_t i = 0; i < N; i++) {
        start.push_back(Ent{U(rng), (uint32_t)i});
        std::push_heap(start.begin(), start.end(), Greater());
    }
    // the record stream, made against a heap that takes it (5 records in 7 beat the minimum of their moment)
    std::vector<double> sc(records);
    size_t effective = 0;
    {
        std::vector<Ent> h = start;
        for (size_t i = 0; i < records; i++) {
            const double low = h[0].score;
            double x = rng() % 7 < 5 ? low + (1.0 - low) * U(rng) : low * (1.0 - 0.004 * U(rng));
            sc[i] = x;
            if (x > low) {
                replace_top<false>(h.data(), (ptrdiff_t)N, Ent{x, h[0].slot});
                effective++;
            }
        }
    }
    const size_t bytes = N * sizeof(Ent) + 128;
    char* raw[2];
    Ent* a[2];
    for (int f = 0; f < 2; f++) {
        raw[f] = (char*)aligned_alloc(64, (bytes + 63) / 64 * 64);
        a[f] = (Ent*)(raw[f] + offset);
    }
    std::vector<Pay> pay(N);
    std::vector<uint32_t> order[2];
    std::vector<double> push_ns[2], pop_ns[2];
    for (int r = 0; r < rounds; r++)
        for (int f = 0; f < 2; f++) {
            memcpy((void*)a[f], start.data(), N * sizeof(Ent));
            Ent* h = a[f];
            auto t0 = std::chrono::steady_clock::now();
            for (size_t i = 0; i < records; i++) {
                if (sc[i] > h[0].score) {  // BestHeap::add on a full heap
                    const uint32_t slot = h[0].slot;
                    pay[slot] = Pay{i, i};
                    if (f) replace_top<true>(h, (ptrdiff_t)N, Ent{sc[i], slot}); else replace_top<false>(h, (ptrdiff_t)N, Ent{sc[i], slot});
                }
            }
            push_ns[f].push_back(std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count() / (double)effective);
            std::vector<Ent> tmp(h, h + N);
            order[f].assign(N, 0);
            Ent* p = tmp.data();
            t0 = std::chrono::steady_clock::now();
            for (size_t i = 0; i < N; i++) {
                order[f][i] = p[0].slot;
                if (f) pop_top<true>(p, (ptrdiff_t)(N - i)); else pop_top<false>(p, (ptrdiff_t)(N - i));
            }
            pop_ns[f].push_back(std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count() / (double)N);
        }
    bool same = memcmp((void*)a[0], (void*)a[1], N * sizeof(Ent)) == 0 && order[0] == order[1];
    // and the library's own form: BestHeap::add over the same fill and records leaves the same array
    {
        kgwas::BestHeap lib(N);
        std::vector<double> by_slot(N);
        for (const Ent& e : start) by_slot[e.slot] = e.score;
        for (size_t i = 0; i < N; i++) lib.add(i, by_slot[i], i);
        for (size_t i = 0; i < records; i++) lib.add(N + i, sc[i], N + i);
        std::vector<uint64_t> km(N), rw(N);
        std::vector<double> ss(N);
        lib.export_state(km.data(), ss.data(), rw.data());
        for (size_t i = 0; i < N && same; i++) same = memcmp(&ss[i], &a[1][i].score, 8) == 0;
        same = same && lib.pushes() == N + effective;
    }
    printf("walk: N %zu, %zu records, %zu effective pushes, %d rounds alternating, array base at %zu mod 64\n", N, records, effective, rounds, offset);
    printf("  push: one level per load %.1f ns (min %.1f), two levels per load %.1f ns (min %.1f): %+.1f %%\n", median(push_ns[0]),
           *std::min_element(push_ns[0].begin(), push_ns[0].end()), median(push_ns[1]), *std::min_element(push_ns[1].begin(), push_ns[1].end()),
           100.0 * (median(push_ns[1]) / median(push_ns[0]) - 1.0));
    printf("  pop : one level per load %.1f ns (min %.1f), two levels per load %.1f ns (min %.1f): %+.1f %%\n", median(pop_ns[0]),
           *std::min_element(pop_ns[0].begin(), pop_ns[0].end()), median(pop_ns[1]), *std::min_element(pop_ns[1].begin(), pop_ns[1].end()),
           100.0 * (median(pop_ns[1]) / median(pop_ns[0]) - 1.0));
    printf("  arrays after the pushes, pop sequences and BestHeap::add's array: %s\n", same ? "identical" : "DIFFERENT");
    for (int f = 0; f < 2; f++) free(raw[f]);
    return same ? 0 : 1;
}

}  // namespace walk

int main(int argc, char** argv) {
    if (argc > 1 && strcmp(argv[1], "walk") == 0) {
        const size_t N = argc > 2 ? atoi(argv[2]) : 10001;
        const size_t records = argc > 3 ? atoi(argv[3]) : 140000;
        const int rounds = argc > 4 ? atoi(argv[4]) : 31;
        const size_t offset = argc > 5 ? atoi(argv[5]) : 0;
        return walk::run(N, records, rounds, offset);
    }
    const size_t N = argc > 1 ? atoi(argv[1]) : 10001;
    const size_t pushes = argc > 2 ? atoi(argv[2]) : 2000000;
    const int ties = argc > 3 ? atoi(argv[3]) : 0;  // 1: scores on a coarse grid (ties everywhere)
    std::mt19937_64 rng(7);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    // the stream: every score above the current minimum (as the replay sees after the device's filter)
    std::vector<double> sc(N + pushes);
    for (size_t i = 0; i < N; i++) sc[i] = ties ? (double)(rng() % 512) : U(rng);
    kgwas::BestHeap h(N);
    std::priority_queue<QE, std::vector<QE>, QG> q;
    for (size_t i = 0; i < N; i++) {
        h.add(i, sc[i], i);
        q.push(QE{sc[i], i, i});
    }
    double low = h.lowest();
    for (size_t i = N; i < N + pushes; i++) {
        const double hi = ties ? 4096.0 : 1.0;
        double x = low + (hi - low) * U(rng);
        if (ties) x = (double)(long)x + 1.0;
        if (!(x > low)) x = low + 1e-9;
        sc[i] = x;
        // the reference's rule on the mirror
        if (x > q.top().score) {
            q.pop();
            q.push(QE{x, i, i});
        }
        low = q.top().score;
    }
    const auto t0 = std::chrono::steady_clock::now();
    for (size_t i = N; i < N + pushes; i++) h.add(i, sc[i], i);
    const double ns = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count() / (double)pushes;
    std::vector<uint64_t> km, rw;
    std::vector<double> ss;
    h.pop_all(km, ss, rw);
    std::vector<uint64_t> mk;
    while (!q.empty()) {
        mk.push_back(q.top().kmer);
        q.pop();
    }
    bool fwd = km.size() == mk.size(), rev = fwd;
    for (size_t i = 0; i < km.size() && (fwd || rev); i++) {
        fwd = fwd && km[i] == mk[i];
        rev = rev && km[i] == mk[mk.size() - 1 - i];
    }
    const bool same = fwd || rev;
    printf("N %zu, %zu pushes%s: %.1f ns per push (effective %llu), pop order %s\n", N, pushes, ties ? " (tie-heavy)" : "", ns,
           (unsigned long long)h.pushes(), same ? "as std::priority_queue" : "DIFFERENT");
    return same ? 0 : 1;
}
