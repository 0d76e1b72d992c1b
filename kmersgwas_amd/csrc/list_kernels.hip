// list_kernels.hip — device side of list_kmers_found_in_multiple_samples (src/list_kmers_found_in_multiple_samples.cpp:146-201):
// the words of one piece counted per key, the MAC and strand decision, the statistics.
//
// A piece is a run of whole key windows of the reference. Its words lie in one device buffer as SEGMENTS (one read block of
// one accession's slice each, list_kmers.cpp); where no segment descends a word's window is decided by its key alone, so the
// reference's hash map per window is a count per key and its output order is key order. The words are not
// sorted. A regular sample of the buffer is sorted (hipcub) and cut into key ranges, the BUCKETS; one workgroup per bucket
// finds its range in every segment by binary search, streams those words into an LDS hash table (64-bit compare-and-swap on
// the key slot, 64-bit add of the packed counters), sorts the table's slots in LDS, decides and writes its passing keys and
// no-pass records to a staging range of its own, and adds its distinct keys to the statistics. A scan over the buckets' counts
// and a gather make the piece's outputs contiguous and in key order.
//
// LDS: a table of `slots` x 16 bytes (4096 slots = 64 KiB by default) plus about 3 KiB of scan state: two workgroups of 256
// threads per CU (160 KiB), eight waves - enough to hide the latency of the searches and of the 8-byte gathers of the stream,
// while a table of half a workgroup's LDS keeps the load factor of a bucket of 2048 words at or below one half.
#include <hipcub/hipcub.hpp>

#include "kernels.h"
#include "sorted_search.h"

namespace kgwas {

namespace {

constexpr uint32_t LL_BLOCK = 256;
constexpr uint64_t LL_KEY_MASK = 0x3FFFFFFFFFFFFFFFull;  // the top two bits of a word are strand flags (src/kmers_single_database.cpp:147)
constexpr uint64_t LL_EMPTY = ~0ull;                     // no masked key has this value
// the three counters of a key in one word, as the reference packs them (:137) but 21 bits wide: all | canonical << 21 | non-canonical << 42
constexpr uint32_t LL_BITS = 21;
constexpr uint64_t LL_FIELD = (1ull << LL_BITS) - 1;
constexpr uint32_t LL_HOT = 2;  // statistics cells with count_all <= LL_HOT are kept in LDS and flushed once per workgroup

struct MaskedWords {
    const uint64_t* p;
    __device__ __forceinline__ uint64_t operator[](uint64_t i) const { return p[i] & LL_KEY_MASK; }
};

// One read block of one accession's slice, as it lands in the piece buffer: flags[0] = 1 when a word is below the one before
// it (carry_key before word 0 when has_prev: the last word of the slice's previous block), flags[1] = the smallest index of a
// file that has a word with flag 0 (preset to 0xFFFFFFFF).
__global__ void __launch_bounds__(LL_BLOCK) ll_check_kernel(const uint64_t* w, uint32_t m, uint64_t carry_key, int has_prev, uint32_t file,
                                                            uint32_t* flags) {
    for (uint32_t j = blockIdx.x * LL_BLOCK + threadIdx.x; j < m; j += gridDim.x * LL_BLOCK) {
        const uint64_t v = w[j], x = v & LL_KEY_MASK;
        if (j > 0 || has_prev) {
            const uint64_t px = j > 0 ? (w[j - 1] & LL_KEY_MASK) : carry_key;
            if (x < px) flags[0] = 1u;
        }
        if ((v >> 62) == 0) atomicMin(flags + 1, file);
    }
}

// sample[i] = the key of word floor(i * total / m), i < m <= total
__global__ void __launch_bounds__(LL_BLOCK) ll_sample_kernel(const uint64_t* words, uint64_t total, uint32_t m, uint64_t* sample) {
    const uint32_t i = blockIdx.x * LL_BLOCK + threadIdx.x;
    if (i < m) sample[i] = words[(uint64_t)i * total / m] & LL_KEY_MASK;
}

__device__ __forceinline__ uint32_t ll_slot(uint64_t key, uint32_t mask) { return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 40) & mask; }

// Bucket b = keys in [sample[b m / nb], sample[(b + 1) m / nb]) (from 0 for the first, unbounded for the last).
__global__ void __launch_bounds__(LL_BLOCK) ll_count_kernel(const ListArgs a) {
    extern __shared__ uint64_t ll_table[];
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(ll_table);
    unsigned long long* cnts = keys + a.slots;
    using Scan = hipcub::BlockScan<uint32_t, LL_BLOCK>;
    using Reduce = hipcub::BlockReduce<unsigned long long, LL_BLOCK>;
    __shared__ union {
        typename Scan::TempStorage scan;
        typename Reduce::TempStorage reduce;
    } tmp;
    __shared__ uint32_t s_excl[LL_BLOCK], s_start[LL_BLOCK];
    __shared__ unsigned long long s_base, s_low;
    __shared__ uint32_t s_over, s_d;
    __shared__ uint32_t hot[3][LL_HOT + 1][LL_HOT + 1], hot_share[LL_HOT + 1];

    const uint32_t b = blockIdx.x, tid = threadIdx.x, mask = a.slots - 1;
    const uint64_t lo_key = b ? a.sample[(uint64_t)b * a.m / a.nb] : 0;
    const uint64_t hi_key = b + 1 < a.nb ? a.sample[(uint64_t)(b + 1) * a.m / a.nb] : LL_EMPTY;
    if (lo_key >= hi_key) return;  // (equal splitters: an empty range; the bucket's counts were zeroed by the host)

    for (uint32_t i = tid; i < a.slots; i += LL_BLOCK) keys[i] = LL_EMPTY, cnts[i] = 0;
    if (tid < 3 * (LL_HOT + 1) * (LL_HOT + 1)) (&hot[0][0][0])[tid] = 0;
    if (tid <= LL_HOT) hot_share[tid] = 0;
    if (tid == 0) s_over = 0, s_d = 0;
    __syncthreads();

    // ---- count: the bucket's range of every segment, 256 segments at a time, streamed into the table -----------------------------
    unsigned long long before = 0;  // words of this thread's segments below the bucket: summed, the bucket's place in the staging arrays
    uint64_t in_bucket = 0;
    for (uint32_t s0 = 0; s0 < a.n_seg; s0 += LL_BLOCK) {
        const uint32_t s = s0 + tid;
        uint32_t lo = 0, n = 0, off = 0;
        if (s < a.n_seg) {
            off = a.seg_off[s];
            const uint32_t len = a.seg_len[s];
            const MaskedWords seg{a.words + off};
            lo = (uint32_t)fk_bound<false>(seg, 0, len, lo_key);
            n = (hi_key == LL_EMPTY ? len : (uint32_t)fk_bound<false>(seg, lo, len, hi_key)) - lo;
            before += lo;
        }
        uint32_t excl, total;
        Scan(tmp.scan).ExclusiveSum(n, excl, total);
        s_excl[tid] = excl;
        s_start[tid] = off + lo;
        __syncthreads();
        for (uint32_t i = tid; i < total; i += LL_BLOCK) {
            uint32_t l = 0, r = LL_BLOCK - 1;  // the last segment whose first word is at or before i (it is not empty)
            while (l < r) {
                const uint32_t mid = (l + r + 1) >> 1;
                if (s_excl[mid] <= i)
                    l = mid;
                else
                    r = mid - 1;
            }
            const uint64_t v = a.words[(uint64_t)s_start[l] + (i - s_excl[l])];
            const uint64_t key = v & LL_KEY_MASK, f = v >> 62;
            if (f == 0) continue;  // (ll_check_kernel has reported it: the piece is refused)
            const unsigned long long adder = f == 1 ? 1ull | 1ull << LL_BITS : f == 2 ? 1ull | 1ull << (2 * LL_BITS) : 1ull;
            uint32_t h = ll_slot(key, mask), probes = 0;
            for (; probes < a.slots; probes++, h = (h + 1) & mask) {
                const unsigned long long prev = atomicCAS(keys + h, (unsigned long long)LL_EMPTY, (unsigned long long)key);
                if (prev == LL_EMPTY || prev == key) {
                    atomicAdd(cnts + h, adder);
                    break;
                }
            }
            if (probes == a.slots) s_over = 1;  // the table is full: the host counts this piece
        }
        in_bucket += total;
        __syncthreads();
    }
    const unsigned long long base = Reduce(tmp.reduce).Sum(before);
    if (tid == 0) {
        s_base = base;
        s_low = 0;
        if (in_bucket > LL_FIELD) s_over = 1;  // (a counter could have wrapped)
    }
    __syncthreads();
    if (s_over) {
        if (tid == 0) a.flags[2] = 1u;
        return;
    }

    // ---- sort the slots by key (bitonic, the empty slots go last) -------------------------------------------------------------------
    for (uint32_t k = 2; k <= a.slots; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t i = tid; i < a.slots; i += LL_BLOCK) {
                const uint32_t p = i ^ j;
                if (p > i) {
                    const unsigned long long x = keys[i], y = keys[p];
                    if ((x > y) == ((i & k) == 0)) {
                        keys[i] = y;
                        keys[p] = x;
                        const unsigned long long c = cnts[i];
                        cnts[i] = cnts[p];
                        cnts[p] = c;
                    }
                }
            }
            __syncthreads();
        }
    }
    for (uint32_t i = tid; i < a.slots; i += LL_BLOCK)
        if (keys[i] != LL_EMPTY && (i + 1 == a.slots || keys[i + 1] == LL_EMPTY)) s_d = i + 1;
    __syncthreads();
    const uint32_t d = s_d;

    // ---- decide, write, count (main()'s loop over unique_kmers, :171-200) ---------------------------------------------------------------
    const uint64_t N1 = a.N + 1, NN = N1 * N1;
    unsigned long long low = 0;
    uint32_t n_pass = 0, n_np = 0;
    for (uint32_t r0 = 0; r0 < d; r0 += LL_BLOCK) {
        const uint32_t i = r0 + tid;
        uint32_t pass = 0, np = 0;
        unsigned long long key = 0, c = 0;
        if (i < d) {
            key = keys[i];
            c = cnts[i];
            const uint64_t all = c & LL_FIELD, canon = (c >> LL_BITS) & LL_FIELD, non = (c >> (2 * LL_BITS)) & LL_FIELD;
            const uint64_t both = all - canon - non;
            if (all > a.N) {  // (the reference would write outside its matrices)
                atomicMin(a.err_key, key);
                a.flags[3] = 1u;
            } else {
                if (all >= a.mac) {
                    const uint32_t need = a.need[all];
                    pass = need != LL_NEED_NONE && canon + both >= need && non + both >= need;
                    np = !pass;
                } else
                    low++;
                if (all <= LL_HOT) {
                    atomicAdd(&hot[0][all][canon], 1u);
                    atomicAdd(&hot[1][all][non], 1u);
                    atomicAdd(&hot[2][all][both], 1u);
                    if (pass) atomicAdd(&hot_share[all], 1u);
                } else {
                    atomicAdd(a.stats + all * N1 + canon, 1ull);
                    atomicAdd(a.stats + NN + all * N1 + non, 1ull);
                    atomicAdd(a.stats + 2 * NN + all * N1 + both, 1ull);
                    if (pass) atomicAdd(a.stats + 3 * NN + all, 1ull);
                }
            }
        }
        uint32_t excl, total;
        Scan(tmp.scan).ExclusiveSum(pass | np << 16, excl, total);
        if (pass) a.stage_pass[s_base + n_pass + (excl & 0xFFFFu)] = key;
        if (np) {
            const uint64_t o = s_base + n_np + (excl >> 16);
            a.stage_np_key[o] = key;
            a.stage_np_cnt[o] = c;
        }
        n_pass += total & 0xFFFFu;
        n_np += total >> 16;
        __syncthreads();
    }
    if (low) atomicAdd(&s_low, low);
    __syncthreads();
    if (tid < 3 * (LL_HOT + 1) * (LL_HOT + 1)) {
        const uint32_t mat = tid / ((LL_HOT + 1) * (LL_HOT + 1)), all = tid / (LL_HOT + 1) % (LL_HOT + 1), col = tid % (LL_HOT + 1);
        const uint32_t v = hot[mat][all][col];
        if (v) atomicAdd(a.stats + mat * NN + all * N1 + col, (unsigned long long)v);  // (a cell that was counted lies inside the matrix)
    } else if (tid < 3 * (LL_HOT + 1) * (LL_HOT + 1) + LL_HOT + 1) {
        const uint32_t all = tid - 3 * (LL_HOT + 1) * (LL_HOT + 1);
        if (hot_share[all]) atomicAdd(a.stats + 3 * NN + all, (unsigned long long)hot_share[all]);
    }
    if (tid == 0) {
        if (s_low) atomicAdd(a.stats + 3 * NN + N1 + b % TESTED_SHARDS, s_low);
        a.bk_base[b] = (uint32_t)s_base;
        a.bk_pass[b] = n_pass;
        a.bk_np[b] = n_np;
    }
}

// The buckets' staged records, bucket after bucket, into the piece's outputs (off_*: exclusive scans of bk_*).
__global__ void __launch_bounds__(LL_BLOCK) ll_gather_kernel(const ListArgs a, const uint32_t* off_pass, const uint32_t* off_np,
                                                             uint64_t* out_pass, uint64_t* out_np_key, uint64_t* out_np_cnt) {
    const uint32_t b = blockIdx.x;
    const uint64_t base = a.bk_base[b];
    const uint32_t np = a.bk_pass[b], nn = a.bk_np[b], op = off_pass[b], on = off_np[b];
    for (uint32_t i = threadIdx.x; i < np; i += LL_BLOCK) out_pass[op + i] = a.stage_pass[base + i];
    for (uint32_t i = threadIdx.x; i < nn; i += LL_BLOCK) {
        out_np_key[on + i] = a.stage_np_key[base + i];
        out_np_cnt[on + i] = a.stage_np_cnt[base + i];
    }
}

// total[i] += piece[i]; piece[i] = 0
__global__ void __launch_bounds__(LL_BLOCK) ll_commit_kernel(unsigned long long* total, unsigned long long* piece, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * LL_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * LL_BLOCK) {
        const unsigned long long v = piece[i];
        if (v) {
            total[i] += v;
            piece[i] = 0;
        }
    }
}

uint32_t ll_grid(uint64_t n) { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + LL_BLOCK - 1) / LL_BLOCK, 2048)); }

}  // namespace

hipError_t launch_ll_check(const uint64_t* words, uint32_t m, uint64_t carry_key, bool has_prev, uint32_t file, uint32_t* flags,
                           hipStream_t st) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(ll_check_kernel, dim3(ll_grid(m)), dim3(LL_BLOCK), 0, st, words, m, carry_key, has_prev ? 1 : 0, file, flags);
    return hipGetLastError();
}

size_t ll_temp_bytes(uint32_t max_sample, uint32_t max_buckets) {
    size_t a = 0, b = 0;
    if (hipcub::DeviceRadixSort::SortKeys(nullptr, a, (const uint64_t*)nullptr, (uint64_t*)nullptr, max_sample, 0, 62) != hipSuccess ||
        hipcub::DeviceScan::ExclusiveSum(nullptr, b, (const uint32_t*)nullptr, (uint32_t*)nullptr, max_buckets + 1) != hipSuccess)
        return 0;
    return std::max<size_t>(std::max(a, b), 16);
}

hipError_t launch_ll_splitters(const uint64_t* words, uint64_t total, uint32_t m, uint64_t* sample_raw, uint64_t* sample, void* temp,
                               size_t temp_bytes, hipStream_t st) {
    if (m == 0 || m > total) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ll_sample_kernel, dim3((m + LL_BLOCK - 1) / LL_BLOCK), dim3(LL_BLOCK), 0, st, words, total, m, sample_raw);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t tb = temp_bytes;
    return hipcub::DeviceRadixSort::SortKeys(temp, tb, sample_raw, sample, m, 0, 62, st);
}

size_t ll_count_lds_bytes(uint32_t slots) { return (size_t)slots * 16; }

hipError_t launch_ll_count(const ListArgs& a, hipStream_t st) {
    if (a.nb == 0 || a.m == 0 || a.m < a.nb || a.slots < 2 || (a.slots & (a.slots - 1)) || a.slots > LL_MAX_SLOTS || a.N >= (1ull << 20))
        return hipErrorInvalidValue;
    const size_t lds = ll_count_lds_bytes(a.slots);
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)ll_count_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(ll_count_kernel, dim3(a.nb), dim3(LL_BLOCK), lds, st, a);
    return hipGetLastError();
}

hipError_t launch_ll_gather(const ListArgs& a, uint32_t* off_pass, uint32_t* off_np, uint64_t* out_pass, uint64_t* out_np_key,
                            uint64_t* out_np_cnt, void* temp, size_t temp_bytes, hipStream_t st) {
    hipError_t e;
    size_t tb = temp_bytes;
    if ((e = hipcub::DeviceScan::ExclusiveSum(temp, tb, a.bk_pass, off_pass, a.nb + 1, st)) != hipSuccess) return e;
    tb = temp_bytes;
    if ((e = hipcub::DeviceScan::ExclusiveSum(temp, tb, a.bk_np, off_np, a.nb + 1, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(ll_gather_kernel, dim3(a.nb), dim3(LL_BLOCK), 0, st, a, off_pass, off_np, out_pass, out_np_key, out_np_cnt);
    return hipGetLastError();
}

hipError_t launch_ll_commit(unsigned long long* total, unsigned long long* piece, uint64_t n, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(ll_commit_kernel, dim3(ll_grid(n)), dim3(LL_BLOCK), 0, st, total, piece, n);
    return hipGetLastError();
}

}  // namespace kgwas
