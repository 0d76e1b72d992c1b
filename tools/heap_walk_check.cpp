// heap_walk_check.cpp - BestHeap's hole walks (heap.h: two levels per load latency while a hole has all four grandchildren)
// against a literal std::priority_queue, at the capacities where the walk changes its path and on streams that tie, and
// under the sanitizers: the grandchild loads are issued before the walk knows which child it takes, the one place where
// heap.h could read past its array. Every heap gets a memory resource, so its arrays are reserved at exactly N entries
// and a load of a[N] is a load past the allocation. Checked per record: size and the minimum's bits; at the end: the
// count of effective pushes, and identities, score bits and rows in pop order through pop_all and pop_all_classic.
// build: g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I kmersgwas_amd/csrc tools/heap_walk_check.cpp -o tools/bin/heap_walk_check
// (a host-only program: run it on the CPU, on its own)
#include <cmath>
#include <cstdio>
#include <limits>
#include <memory_resource>
#include <queue>
#include <random>
#include <string>
#include <tuple>
#include <vector>

#include "heap.h"

typedef std::tuple<uint64_t, double, size_t> RefEntry;  // the reference's shapes (src/kmer_general.h:113-128)
struct RefCmp {
    bool operator()(const RefEntry& a, const RefEntry& b) const { return std::get<1>(a) > std::get<1>(b); }
};

static bool same_bits(double a, double b) { return memcmp(&a, &b, 8) == 0; }

static const char* const kStreams[] = {"all_equal", "two_values", "ascending", "descending", "duplicates", "late_tie", "turns_negative", "turns_nan"};

static std::vector<double> make_stream(int kind, size_t N, size_t n, std::mt19937_64& rng) {
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::vector<double> s(n);
    switch (kind) {
        case 0: for (auto& x : s) x = 2.5; break;
        case 1: for (auto& x : s) x = rng() % 2 ? 1.0 : 3.0; break;
        case 2: for (size_t i = 0; i < n; i++) s[i] = 1.0 + (double)i * 0.125; break;
        case 3: for (size_t i = 0; i < n; i++) s[i] = 1.0 + (double)(n - i) * 0.125; break;
        case 4:
            for (auto& x : s) x = 10.0 + U(rng);
            for (size_t i = 1; i < n; i++)
                if (rng() % 10 < 3) s[i] = s[rng() % i];
            break;
        case 5: {  // distinct, but one of the N largest is repeated in the last 2 % of the stream
            for (size_t i = 0; i < n; i++) s[i] = 10.0 + U(rng) + (double)i * 1e-9;
            std::vector<double> sorted(s.begin(), s.end() - n / 50 - 1);
            std::sort(sorted.begin(), sorted.end());
            const size_t top = std::min(N, sorted.size());
            s[n - 1 - rng() % (n / 50 + 1)] = sorted[sorted.size() - 1 - rng() % top];
            break;
        }
        default:  // the int64 compares are switched off for good in mid-stream, on a heap they have built
            for (size_t i = 0; i < n; i++) {
                s[i] = (double)(rng() % 64) * 0.25 + (i >= n / 2 && rng() % 4 == 0 ? 100.0 : 0.0);
                if (i >= n / 2 && rng() % 8 == 0) s[i] = kind == 6 ? -(double)(rng() % 5) * 0.5 : std::numeric_limits<double>::quiet_NaN();
            }
    }
    return s;
}

int main() {
    const size_t caps[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 14, 15, 16, 17, 22, 23, 30, 31, 32, 33, 62, 63, 64, 10001};
    std::mt19937_64 rng(20240601);
    int bad = 0, cases = 0;
    for (size_t N : caps)
        for (int kind = 0; kind < 8; kind++) {
            const size_t n = 20 * N + 7;
            const std::vector<double> s = make_stream(kind, N, n, rng);
            kgwas::BestHeap h(N, std::pmr::new_delete_resource());
            std::priority_queue<RefEntry, std::vector<RefEntry>, RefCmp> q;
            double lowest = 0;
            uint64_t pushes = 0;
            std::string why;
            for (size_t i = 0; i < n && why.empty(); i++) {
                h.add(1000 + i, s[i], 3 * i);
                if (q.size() < N || s[i] > lowest) {  // add_association (src/best_associations_heap.cpp:43-59)
                    if (q.size() >= N) q.pop();
                    q.push(RefEntry(1000 + i, s[i], 3 * i));
                    lowest = std::get<1>(q.top());
                    pushes++;
                }
                if (h.size() != q.size() || !same_bits(h.lowest(), lowest)) why = "minimum differs after record " + std::to_string(i);
            }
            if (why.empty() && h.pushes() != pushes) why = "effective pushes differ";
            std::vector<uint64_t> k[2], r[2];
            std::vector<double> sc[2];
            h.pop_all(k[0], sc[0], r[0]);
            h.pop_all_classic(k[1], sc[1], r[1]);
            for (size_t i = 0; why.empty() && !q.empty(); i++) {
                const RefEntry e = q.top();
                q.pop();
                for (int f = 0; f < 2; f++)
                    if (i >= k[f].size() || std::get<0>(e) != k[f][i] || !same_bits(std::get<1>(e), sc[f][i]) || std::get<2>(e) != r[f][i])
                        why = std::string(f ? "pop_all_classic" : "pop_all") + ": pop " + std::to_string(i) + " differs";
            }
            cases++;
            if (!why.empty()) {
                bad++;
                printf("N %zu, stream %s: %s\n", N, kStreams[kind], why.c_str());
            }
        }
    printf("%d heaps (25 capacities x 8 streams) against std::priority_queue: %d differ\n", cases, bad);
    return bad ? 1 : 0;
}
