// count_kernels.hip — device side of count_kmers_with_strand (count_kmers.cpp): the k-mers of a resident
// base stream counted under their canonical form, one key range (a PASS) at a time.
//
// The base stream is bytes; A C G T (either case) are bases, every other byte separates reads. ck_encode turns the windows of
// the pass's key range into SORT WORDS (key << 1) | orient, orient 0 where the window itself is the canonical form; the words
// are radix-sorted on bits [0, 2k + 1) (hipcub), so a key's words are one run with the orient-0 words first. ck_heads finds
// the run heads, ck_reduce turns a run into count (distance to the next head) and flags (orient of its first and of its last
// word) and decides, ck_compact writes the kept key | flags words in order. No lane walks along a run.
//
// ck_encode: a workgroup of 256 lanes takes a tile of 4096 positions (kmer_windows.h: the tile, the packing and the codes, which
// locate_kernels.hip shares). The first window's code is a funnel shift, its reverse complement a bit reversal; the other
// 15 follow by rolling both codes one base on. The words of the tile are compacted in LDS (32 KiB) and written with ONE slot
// claim per workgroup (per-wave device-scope atomics on one address: DESIGN.md §0 row f-2, §4.1b) and coalesced stores.
#include <hipcub/hipcub.hpp>

#include "kernels.h"
#include "kmer_windows.h"

namespace kgwas {

namespace {

constexpr uint32_t CK_ITEMS = 8;                   // words per lane of the heads / reduce / compact kernels
constexpr uint32_t CK_RTILE = CK_BLOCK * CK_ITEMS;
constexpr uint64_t CK_FLAG_CANON = 0x4000000000000000ull, CK_FLAG_NON = 0x8000000000000000ull;

__global__ void __launch_bounds__(CK_BLOCK) ck_encode_kernel(const uint8_t* __restrict__ bases, uint64_t n, uint32_t k, uint64_t lo, uint64_t hi,
                                                             uint64_t* __restrict__ words, uint64_t cap, unsigned long long* ctr, int aligned) {
    __shared__ uint32_t s_codes[CK_PACKS], s_valid[CK_PACKS];
    __shared__ uint64_t s_words[CK_TILE];
    using Scan = hipcub::BlockScan<uint32_t, CK_BLOCK>;
    __shared__ typename Scan::TempStorage s_scan;
    __shared__ unsigned long long s_base;
    __shared__ uint32_t s_n1;

    const uint32_t tid = threadIdx.x;
    const uint64_t n_tiles = (n + CK_TILE - 1) / CK_TILE;
    const uint64_t kmask = (1ull << k) - 1, cmask = (1ull << (2 * k)) - 1;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t t0 = tile * CK_TILE;
        uint32_t c0, v0;
        ck_pack(bases, n, t0 + (uint64_t)tid * CK_RUN, aligned, c0, v0);
        s_codes[tid] = c0, s_valid[tid] = v0;
        if (tid < 2) {
            uint32_t ch, vh;
            ck_pack(bases, n, t0 + CK_TILE + (uint64_t)tid * CK_RUN, aligned, ch, vh);
            s_codes[CK_BLOCK + tid] = ch, s_valid[CK_BLOCK + tid] = vh;
        }
        if (tid == 0) s_n1 = 0;
        __syncthreads();
        // positions 0-31 of this lane's stretch in X_hi (first base in the top bits), 32-47 in the top half of X_lo
        const uint64_t X_hi = ((uint64_t)c0 << 32) | s_codes[tid + 1], X_lo = (uint64_t)s_codes[tid + 2] << 32;
        const uint64_t V = (uint64_t)v0 | ((uint64_t)s_valid[tid + 1] << 16) | ((uint64_t)s_valid[tid + 2] << 32);

        uint64_t w[CK_RUN];
        uint32_t emit = 0, n1 = 0;
        uint64_t a = X_hi >> (64 - 2 * k), b = ck_revcomp(a, k);
#pragma unroll
        for (uint32_t j = 0; j < CK_RUN; j++) {
            const bool ok = ((V >> j) & kmask) == kmask;
            const bool canon = a < b;
            const uint64_t key = canon ? a : b;
            w[j] = (key << 1) | (canon ? 0u : 1u);
            if (ok && key >= lo && key < hi) emit |= 1u << j, n1 += !canon;
            // the base at position j + k comes in
            const uint64_t c = ck_base_at(X_hi, X_lo, j + k);
            a = ((a << 2) | c) & cmask;
            b = (b >> 2) | ((3 - c) << (2 * k - 2));
        }
        const uint32_t cnt = __popc(emit);
        uint32_t excl, total;
        Scan(s_scan).ExclusiveSum(cnt, excl, total);
        if (n1) atomicAdd(&s_n1, n1);
#pragma unroll
        for (uint32_t j = 0; j < CK_RUN; j++)
            if (emit >> j & 1u) s_words[excl++] = w[j];
        __syncthreads();
        if (tid == 0) {
            s_base = total ? atomicAdd(ctr, (unsigned long long)total) : 0ull;
            if (s_n1) atomicAdd(ctr + 1, (unsigned long long)s_n1);
        }
        __syncthreads();
        const uint64_t base = s_base;
        if (base + total <= cap)  // (a pass that does not fit is redone on half of its range: nothing of it is used)
            for (uint32_t i = tid; i < total; i += CK_BLOCK) words[base + i] = s_words[i];
        __syncthreads();
    }
}

// sample[i] = the canonical key of the window at position floor(i n / m), all ones where that window is not counted
__global__ void __launch_bounds__(CK_BLOCK) ck_sample_kernel(const uint8_t* __restrict__ bases, uint64_t n, uint32_t k, uint32_t m, uint64_t* sample) {
    const uint32_t i = blockIdx.x * CK_BLOCK + threadIdx.x;
    if (i >= m) return;
    const uint64_t p = (uint64_t)i * n / m;
    uint64_t a = 0;
    bool ok = p + k <= n;
    for (uint32_t j = 0; ok && j < k; j++) {
        const uint32_t c = ck_code(bases[p + j]);
        ok = c < 4u;
        a = (a << 2) | (c & 3u);
    }
    const uint64_t b = ck_revcomp(a, k);
    sample[i] = ok ? (a < b ? a : b) : ~0ull;
}

// ---- heads: blk[b] = run heads among the sorted words of tile b (pass 0); heads[off[b] ...] = their positions (pass 1) ----------
template <int PASS>
__global__ void __launch_bounds__(CK_BLOCK) ck_heads_kernel(const uint64_t* __restrict__ s, uint64_t n, uint32_t* blk, const uint32_t* off,
                                                            uint32_t* __restrict__ heads) {
    using Scan = hipcub::BlockScan<uint32_t, CK_BLOCK>;
    __shared__ typename Scan::TempStorage s_scan;
    const uint64_t i0 = (uint64_t)blockIdx.x * CK_RTILE + (uint64_t)threadIdx.x * CK_ITEMS;
    uint32_t mask = 0;
    if (i0 < n) {
        uint64_t prev = i0 ? s[i0 - 1] >> 1 : 0;
#pragma unroll
        for (uint32_t j = 0; j < CK_ITEMS; j++) {
            if (i0 + j < n) {
                const uint64_t key = s[i0 + j] >> 1;
                if (i0 + j == 0 || key != prev) mask |= 1u << j;
                prev = key;
            }
        }
    }
    uint32_t excl, total;
    Scan(s_scan).ExclusiveSum((uint32_t)__popc(mask), excl, total);
    if (PASS == 0) {
        if (threadIdx.x == 0) blk[blockIdx.x] = total;
    } else {
        uint32_t o = off[blockIdx.x] + excl;
#pragma unroll
        for (uint32_t j = 0; j < CK_ITEMS; j++)
            if (mask >> j & 1u) heads[o++] = (uint32_t)(i0 + j);
    }
}

// ---- reduce: run r = sorted words [heads[r], heads[r + 1]) (to n for the last) -> res[r] = key | flags if kept, else 0;
// blk[b] = kept runs of tile b; the counters of the tile's runs are added to counts[0..6] once per workgroup ---------------------
__global__ void __launch_bounds__(CK_BLOCK) ck_reduce_kernel(const uint64_t* __restrict__ s, uint64_t n, const uint32_t* __restrict__ heads,
                                                             uint32_t n_runs, uint64_t ci, uint64_t cx, uint64_t* __restrict__ res, uint32_t* blk,
                                                             unsigned long long* counts) {
    __shared__ uint32_t s_cnt[8];
    const uint32_t tid = threadIdx.x;
    if (tid < 8) s_cnt[tid] = 0;
    __syncthreads();
    uint32_t kept = 0, oheads = 0, oheads_kept = 0, by_flag[3] = {0, 0, 0};
    for (uint32_t j = 0; j < CK_ITEMS; j++) {
        const uint64_t r = (uint64_t)blockIdx.x * CK_RTILE + j * CK_BLOCK + tid;  // (coalesced over the lanes)
        if (r >= n_runs) break;
        const uint64_t i = heads[r], e = r + 1 < n_runs ? heads[r + 1] : n;
        const uint64_t first = s[i], last = s[e - 1];
        const uint32_t has0 = !(first & 1), has1 = (uint32_t)(last & 1);
        const uint64_t count = e - i;
        const bool keep = count >= ci && count <= cx;
        res[r] = keep ? (first >> 1) | (has0 ? CK_FLAG_CANON : 0) | (has1 ? CK_FLAG_NON : 0) : 0;
        oheads += has0 + has1;
        if (keep) kept++, oheads_kept += has0 + has1, by_flag[has0 + 2 * has1 - 1]++;
    }
    if (kept) atomicAdd(&s_cnt[0], kept);
    if (oheads) atomicAdd(&s_cnt[1], oheads);
    if (oheads_kept) atomicAdd(&s_cnt[2], oheads_kept);
    for (int f = 0; f < 3; f++)
        if (by_flag[f]) atomicAdd(&s_cnt[4 + f], by_flag[f]);
    __syncthreads();
    if (tid < 7 && s_cnt[tid]) atomicAdd(counts + tid, (unsigned long long)s_cnt[tid]);
    if (tid == 0) blk[blockIdx.x] = s_cnt[0];
}

// ---- compact: the non-zero res of tile b, in order, to out[off[b] ...] --------------------------------------------------------------
__global__ void __launch_bounds__(CK_BLOCK) ck_compact_kernel(const uint64_t* __restrict__ res, uint32_t n_runs, const uint32_t* off,
                                                              uint64_t* __restrict__ out) {
    using Scan = hipcub::BlockScan<uint32_t, CK_BLOCK>;
    __shared__ typename Scan::TempStorage s_scan;
    const uint64_t r0 = (uint64_t)blockIdx.x * CK_RTILE + (uint64_t)threadIdx.x * CK_ITEMS;
    uint64_t v[CK_ITEMS];
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t j = 0; j < CK_ITEMS; j++) {
        v[j] = r0 + j < n_runs ? res[r0 + j] : 0;
        cnt += v[j] != 0;
    }
    uint32_t excl;
    Scan(s_scan).ExclusiveSum(cnt, excl);
    uint64_t o = (uint64_t)off[blockIdx.x] + excl;
#pragma unroll
    for (uint32_t j = 0; j < CK_ITEMS; j++)
        if (v[j]) out[o++] = v[j];
}

uint32_t ck_tiles(uint64_t n) { return (uint32_t)((n + CK_RTILE - 1) / CK_RTILE); }

}  // namespace

uint32_t ck_blocks(uint64_t max_words) { return ck_tiles(max_words) + 1; }

size_t ck_temp_bytes(uint64_t max_words, uint32_t max_sample, uint32_t kmer_len) {
    size_t a = 0, b = 0, c = 0;
    if (hipcub::DeviceRadixSort::SortKeys(nullptr, a, (const uint64_t*)nullptr, (uint64_t*)nullptr, max_words, 0, (int)(2 * kmer_len + 1)) != hipSuccess ||
        hipcub::DeviceRadixSort::SortKeys(nullptr, b, (const uint64_t*)nullptr, (uint64_t*)nullptr, max_sample, 0, 64) != hipSuccess ||
        hipcub::DeviceScan::ExclusiveSum(nullptr, c, (const uint32_t*)nullptr, (uint32_t*)nullptr, ck_blocks(max_words)) != hipSuccess)
        return 0;
    return std::max<size_t>(std::max(std::max(a, b), c), 16);
}

hipError_t launch_ck_encode(const uint8_t* bases, uint64_t n, uint32_t kmer_len, uint64_t lo, uint64_t hi, uint64_t* words, uint64_t cap,
                            unsigned long long* ctr, hipStream_t st) {
    if (kmer_len < 1 || kmer_len > 31) return hipErrorInvalidValue;
    if (n < kmer_len) return hipSuccess;
    const uint64_t tiles = (n + CK_TILE - 1) / CK_TILE;
    const int aligned = (reinterpret_cast<uintptr_t>(bases) & 15) == 0;
    hipLaunchKernelGGL(ck_encode_kernel, dim3((uint32_t)std::min<uint64_t>(tiles, 2048)), dim3(CK_BLOCK), 0, st, bases, n, kmer_len, lo, hi,
                       words, cap, ctr, aligned);
    return hipGetLastError();
}

hipError_t launch_ck_sample(const uint8_t* bases, uint64_t n, uint32_t kmer_len, uint32_t m, uint64_t* sample, hipStream_t st) {
    if (m == 0) return hipSuccess;
    if (kmer_len < 1 || kmer_len > 31 || n == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ck_sample_kernel, dim3((m + CK_BLOCK - 1) / CK_BLOCK), dim3(CK_BLOCK), 0, st, bases, n, kmer_len, m, sample);
    return hipGetLastError();
}

hipError_t launch_ck_sort_sample(const uint64_t* raw, uint64_t* sorted, uint32_t m, void* temp, size_t temp_bytes, hipStream_t st) {
    size_t tb = temp_bytes;
    return hipcub::DeviceRadixSort::SortKeys(temp, tb, raw, sorted, m, 0, 64, st);
}

hipError_t launch_ck_sort(const uint64_t* words, uint64_t* sorted, uint64_t n, uint32_t kmer_len, void* temp, size_t temp_bytes, hipStream_t st) {
    size_t tb = temp_bytes;
    return hipcub::DeviceRadixSort::SortKeys(temp, tb, words, sorted, n, 0, (int)(2 * kmer_len + 1), st);
}

hipError_t launch_ck_heads(const uint64_t* sorted, uint64_t n, uint32_t* blk, uint32_t* off, uint32_t* heads, void* temp, size_t temp_bytes,
                           hipStream_t st) {
    if (n == 0 || n > CK_MAX_PASS_WORDS) return hipErrorInvalidValue;
    const uint32_t nb = ck_tiles(n);
    hipError_t e = hipMemsetAsync(blk + nb, 0, 4, st);  // (the scan's last entry is the total)
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ck_heads_kernel<0>, dim3(nb), dim3(CK_BLOCK), 0, st, sorted, n, blk, off, heads);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    size_t tb = temp_bytes;
    if ((e = hipcub::DeviceScan::ExclusiveSum(temp, tb, blk, off, nb + 1, st)) != hipSuccess) return e;  // (off[nb]: the runs)
    hipLaunchKernelGGL(ck_heads_kernel<1>, dim3(nb), dim3(CK_BLOCK), 0, st, sorted, n, blk, off, heads);
    return hipGetLastError();
}

hipError_t launch_ck_reduce(const uint64_t* sorted, uint64_t n, const uint32_t* heads, uint32_t n_runs, uint64_t ci, uint64_t cx, uint64_t* res,
                            uint32_t* blk, uint32_t* off, uint64_t* out, unsigned long long* counts, void* temp, size_t temp_bytes, hipStream_t st) {
    if (n_runs == 0 || n_runs > n) return hipErrorInvalidValue;
    const uint32_t nb = ck_tiles(n_runs);
    hipError_t e = hipMemsetAsync(blk + nb, 0, 4, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ck_reduce_kernel, dim3(nb), dim3(CK_BLOCK), 0, st, sorted, n, heads, n_runs, ci, cx, res, blk, counts);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    size_t tb = temp_bytes;
    if ((e = hipcub::DeviceScan::ExclusiveSum(temp, tb, blk, off, nb + 1, st)) != hipSuccess) return e;  // (off[nb]: the kept runs)
    hipLaunchKernelGGL(ck_compact_kernel, dim3(nb), dim3(CK_BLOCK), 0, st, res, n_runs, off, out);
    return hipGetLastError();
}

}  // namespace kgwas
