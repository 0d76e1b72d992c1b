// survivors.hip — a sparse chunk's path behind its filter, whichever filter that was: the survivors' bitmap becomes row-ordered
// key lists per column (no sort), the listed pairs are re-scored in the exact reference order and leave as candidate records,
// and one prep launch readies the counters, the bitmap and - for the narrow scans - the thresholds of the chunk that follows.
//
//   bitmap -> keys   launch_bitmap_keys (the wide filters' nibble-transposed words: count, scan, scatter) or launch_narrow_keys
//                    (the narrow filter has counted its survivors per segment already: one launch)
//   keys -> records  launch_rescore (rescore_kernel, then compact_kernel: the candidates, compacted) or launch_rescore_direct
//                    (scans of a few columns: every survivor's record at its place in the key order)
//   next chunk       launch_chunk_prep
// The re-scoring repeats calculate_kmer_score (src/kmers_multiple_databases.cpp:327-363) bit for bit - the select-and-add
// chains of score_valu.hip, then the same exact test against the threshold, the threshold histogram, the candidate record - so
// the results are the exact scorers'; a filter only decides what is worth looking at.
#include <algorithm>

#include "block_prims.h"
#include "score_common.h"

namespace kgwas {

// ---- bitmap -> row-ordered survivor keys, column by column ------------------------------------------------------------
// Blocks of 1024 words (65 536 rows): counts, a scan of the block counts per column, then every block writes its keys
// (column << row_bits | row) at its offset, ascending rows: keys_sorted, surv_off[p], surv_cnt[p], key_count.
constexpr uint32_t BM_WORDS = 1024;

// The two key kernels' common tail. x: the thread's four words of block b, bit = row (word b * BM_WORDS + 4 * threadIdx.x + i).
// Their set bits become keys from base + (the set bits of the threads below) on, up to key_cap. part: 4 words of LDS.
__device__ __forceinline__ void emit_keys(const unsigned long long (&x)[4], uint32_t base, uint32_t p, uint32_t b, uint32_t* part,
                                          uint32_t* keys, uint32_t key_cap, uint32_t row_bits) {
    const uint32_t c = __popcll(x[0]) + __popcll(x[1]) + __popcll(x[2]) + __popcll(x[3]);
    uint32_t o = block_scan_excl(c, base, part);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        unsigned long long v = x[i];
        const uint32_t row0 = (b * BM_WORDS + threadIdx.x * 4u + i) * 64u;
        while (v) {
            const uint32_t bit = __ffsll((long long)v) - 1u;
            v &= v - 1ull;
            if (o < key_cap) keys[o] = (p << row_bits) | (row0 + bit);
            o++;
        }
    }
}

__global__ void __launch_bounds__(256) bitmap_count_kernel(const unsigned long long* bm, uint64_t words_per_col, uint32_t n_words,
                                                           uint32_t n_blocks, uint32_t* blk_cnt, unsigned long long* blk_mask) {
    __shared__ uint32_t red[4];
    const uint32_t p = blockIdx.y, b = blockIdx.x;
    const unsigned long long* w = bm + (uint64_t)p * words_per_col;
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t x = b * BM_WORDS + threadIdx.x * 4u + i;
        if (x < n_words) c += __popcll(w[x]);
    }
    // which threads' words hold anything: the scatter kernel reads (and clears) only those - a steady chunk has a survivor
    // in one word of thirty, so its pass over the bitmap touches an eighth of the lines and the chunk's prep launch has
    // nothing to zero
    const unsigned long long m = __ballot(c != 0u);
    if ((threadIdx.x & 63u) == 0u) blk_mask[((uint64_t)p * n_blocks + b) * 4u + (threadIdx.x >> 6)] = m;
    c = block_sum(c, red);
    if (threadIdx.x == 0) blk_cnt[p * n_blocks + b] = c;
}

// block p: exclusive scan of column p's block counts (in place) and the column's total
__global__ void __launch_bounds__(256) bitmap_scan_kernel(uint32_t* blk_cnt, uint32_t n_blocks, uint32_t* col_total) {
    __shared__ uint32_t part[4];
    const uint32_t p = blockIdx.x;
    uint32_t carry = 0;
    for (uint32_t b0 = 0; b0 < n_blocks; b0 += 256u) {
        const uint32_t b = b0 + threadIdx.x;
        if (b0) __syncthreads();
        const uint32_t o = block_scan_excl(b < n_blocks ? blk_cnt[p * n_blocks + b] : 0u, carry, part);
        if (b < n_blocks) blk_cnt[p * n_blocks + b] = o;  // offset inside the column's range
    }
    if (threadIdx.x == 0) col_total[p] = carry;
}

// each column's range in the key list and the total: the work of one 256-thread block (block (0, 0) of the scatter launch - a
// launch of its own for these few microseconds cost the stream as much again)
__device__ __forceinline__ void bitmap_bases_block(const uint32_t* col_total, uint32_t n_pheno, uint32_t key_cap, uint32_t* surv_off,
                                                   uint32_t* surv_cnt, uint32_t* key_count, uint32_t* tile_pref) {
    __shared__ uint32_t part[4];
    uint32_t total = 0;
    for (uint32_t p0 = 0; p0 < n_pheno; p0 += 256u) {
        const uint32_t p = p0 + threadIdx.x;
        const uint32_t v = p < n_pheno ? col_total[p] : 0u;
        if (p0) __syncthreads();
        const uint32_t o = block_scan_excl(v, total, part);
        if (p < n_pheno) {
            surv_off[p] = o;
            surv_cnt[p] = v;
        }
    }
    if (threadIdx.x == 0) *key_count = total;  // the host compares it with the capacity
    const bool over = total > key_cap;  // overflow: the chunk is redone in halves; leave nothing for the re-score kernels to walk
    if (over)
        for (uint32_t p = threadIdx.x; p < n_pheno; p += 256u) surv_cnt[p] = 0u;  // (each thread the words it wrote above)
    // the re-score kernels' tiles of 256 survivors, never straddling a column: tile_pref[p] = first tile of column p
    uint32_t tiles = 0;
    for (uint32_t p0 = 0; p0 < n_pheno; p0 += 256u) {
        const uint32_t p = p0 + threadIdx.x;
        __syncthreads();
        const uint32_t o = block_scan_excl((p < n_pheno && !over) ? (col_total[p] + 255u) / 256u : 0u, tiles, part);
        if (p < n_pheno) tile_pref[p] = o;
    }
    if (threadIdx.x == 0) tile_pref[n_pheno] = tiles;
}

// blk_off: the scanned block counts (bitmap_scan_kernel), col_total: the columns' totals - a block's own count is the
// difference to the next offset. Only the threads the count kernel marked load their words, and they store zeros back: the
// bitmap is all zero again when the launch ends (scan_gpu.cpp: bitmap_clean), whatever the key list could hold.
__global__ void __launch_bounds__(256) bitmap_scatter_kernel(unsigned long long* bm, uint64_t words_per_col, uint32_t n_words,
                                                             uint32_t n_blocks, const uint32_t* blk_off, const uint32_t* col_total,
                                                             const unsigned long long* blk_mask, uint32_t n_pheno, uint32_t* surv_off,
                                                             uint32_t* surv_cnt, uint32_t* key_count, uint32_t* tile_pref, uint32_t* keys,
                                                             uint32_t key_cap, uint32_t row_bits) {
    __shared__ uint32_t part[4];
    __shared__ uint32_t basep[4];
    const uint32_t p = blockIdx.y, b = blockIdx.x;
    // block (0, 0) writes what the kernels behind this one read: the columns' ranges, the total, the re-score tiles' table
    if (p == 0u && b == 0u) bitmap_bases_block(col_total, n_pheno, key_cap, surv_off, surv_cnt, key_count, tile_pref);
    const uint32_t my_off = blk_off[p * n_blocks + b];
    const uint32_t next_off = b + 1u < n_blocks ? blk_off[p * n_blocks + b + 1u] : col_total[p];
    if (next_off == my_off) return;  // nothing in this block (block-uniform)
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    // where column p's keys begin: the totals of the columns before it, added up by the block itself (surv_off[p] is block
    // (0, 0)'s to write, in this same launch)
    uint32_t col_base = 0;
    for (uint32_t q = threadIdx.x; q < p; q += 256u) col_base += col_total[q];
    col_base = block_sum(col_base, basep);
    const bool mine = (blk_mask[((uint64_t)p * n_blocks + b) * 4u + wave] >> lane) & 1ull;
    unsigned long long* w = bm + (uint64_t)p * words_per_col;
    unsigned long long x[4] = {0ull, 0ull, 0ull, 0ull};
    if (mine) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t idx = b * BM_WORDS + threadIdx.x * 4u + i;
            if (idx < n_words) {
                x[i] = w[idx];
                if (x[i]) w[idx] = 0ull;
            }
        }
        // the wide filters write nibble 4 kg + rt for rows 16 rt + 4 kg ..+3 (filter_common.h, filter_emit): back to row order
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (!x[i]) continue;
            unsigned long long y = 0;
#pragma unroll
            for (int kg = 0; kg < 4; kg++)
#pragma unroll
                for (int rt = 0; rt < 4; rt++) y |= ((x[i] >> (4 * (4 * kg + rt))) & 0xFull) << (4 * (4 * rt + kg));
            x[i] = y;
        }
    }
    emit_keys(x, col_base + my_off, p, b, part, keys, key_cap, row_bits);
}

hipError_t launch_bitmap_keys(unsigned long long* bitmap, uint64_t words_per_col, uint64_t n_rows, uint32_t n_pheno, uint32_t* blk_scratch,
                              unsigned long long* blk_mask, uint32_t* keys_sorted, uint32_t key_cap, uint32_t row_bits, uint32_t* surv_off,
                              uint32_t* surv_cnt, uint32_t* key_count, uint32_t* tile_pref, hipStream_t st) {
    const uint32_t n_words = (uint32_t)((n_rows + 63) / 64);
    const uint32_t n_blocks = (n_words + BM_WORDS - 1) / BM_WORDS;
    hipLaunchKernelGGL(bitmap_count_kernel, dim3(n_blocks, n_pheno), dim3(256), 0, st, bitmap, words_per_col, n_words, n_blocks, blk_scratch, blk_mask);
    uint32_t* col_total = blk_scratch + (size_t)n_pheno * n_blocks;
    hipLaunchKernelGGL(bitmap_scan_kernel, dim3(n_pheno), dim3(256), 0, st, blk_scratch, n_blocks, col_total);
    hipLaunchKernelGGL(bitmap_scatter_kernel, dim3(n_blocks, n_pheno), dim3(256), 0, st, bitmap, words_per_col, n_words, n_blocks, blk_scratch,
                       col_total, blk_mask, n_pheno, surv_off, surv_cnt, key_count, tile_pref, keys_sorted, key_cap, row_bits);
    return hipGetLastError();
}

// The narrow filter's keys in one launch: block (b, p) = segment b (1024 bitmap words, in row order as they are) of column p.
// The survivors per (column, segment) are already counted (NarrowArgs::seg_cnt), so a block's place in the key list -
// everything of the columns before it and of its own column's earlier segments - is a sum over at most a few thousand
// counters that every block forms for itself: no scan kernel, no inter-block dependency. Block (0, 0) also writes the
// columns' ranges, the re-score tiles' table and meta.
__global__ void __launch_bounds__(256) narrow_keys_kernel(const unsigned long long* bm, uint64_t words_per_col, uint32_t n_words, uint32_t n_segs,
                                                          uint32_t n_pheno, const uint32_t* seg_cnt, uint32_t* keys, uint32_t key_cap,
                                                          uint32_t row_bits, uint32_t* surv_off, uint32_t* surv_cnt, uint32_t* key_count,
                                                          uint32_t* tile_pref, uint32_t* meta, const unsigned long long* tested_shards) {
    __shared__ uint32_t red[4 * (NARROW_MAX_COLS + 1)];
    __shared__ uint32_t part[4];
    const uint32_t p = blockIdx.y, b = blockIdx.x;
    // tot[q] = survivors of column q; tot[NARROW_MAX_COLS] = those of column p's segments before b
    // (columns at or beyond n_pheno stay 0; the loops over them are unrolled: tot lives in registers)
    uint32_t tot[NARROW_MAX_COLS + 1] = {0u, 0u, 0u, 0u, 0u};
#pragma unroll
    for (uint32_t q = 0; q < NARROW_MAX_COLS; q++)
        for (uint32_t k = threadIdx.x; q < n_pheno && k < n_segs; k += 256u) {
            const uint32_t v = seg_cnt[q * n_segs + k];
            tot[q] += v;
            if (q == p && k < b) tot[NARROW_MAX_COLS] += v;
        }
    block_sum(tot, red);
    uint32_t total = 0, off_p = 0;
#pragma unroll
    for (uint32_t q = 0; q < NARROW_MAX_COLS; q++) {
        if (q < p) off_p += tot[q];
        total += tot[q];
    }
    const bool over = total > key_cap;  // the chunk is redone in halves: nothing for the re-score kernel to walk
    if (b == 0u && p == 0u) {
        // the filter's MAC-passing-row counters -> meta[2 P + 2 .. 3]: one copy closes the chunk
        __shared__ unsigned long long tsum[4];
        const unsigned long long tt = block_sum(tested_shards[threadIdx.x], tsum);  // TESTED_SHARDS == 256 == blockDim.x
        if (threadIdx.x == 0u) {
            meta[2u * n_pheno + 2u] = (uint32_t)tt;
            meta[2u * n_pheno + 3u] = (uint32_t)(tt >> 32);
            uint32_t o = 0, t = 0;
#pragma unroll
            for (uint32_t q = 0; q < NARROW_MAX_COLS; q++) {
                if (q >= n_pheno) break;
                const uint32_t c = over ? 0u : tot[q];
                surv_off[q] = o;
                surv_cnt[q] = c;
                tile_pref[q] = t;
                meta[q] = c;             // records of column q: its survivors (a survivor that is no candidate carries -inf)
                meta[n_pheno + q] = o;
                o += tot[q];
                t += (c + 255u) / 256u;
            }
            tile_pref[n_pheno] = t;
            *key_count = total;
            meta[2u * n_pheno] = over ? 0u : total;
            meta[2u * n_pheno + 1u] = total;
        }
    }
    if (over || seg_cnt[p * n_segs + b] == 0u) return;  // block-uniform
    const unsigned long long* w = bm + (uint64_t)p * words_per_col;
    unsigned long long x[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t idx = b * BM_WORDS + threadIdx.x * 4u + i;
        x[i] = idx < n_words ? w[idx] : 0ull;
    }
    emit_keys(x, off_p + tot[NARROW_MAX_COLS], p, b, part, keys, key_cap, row_bits);
}

hipError_t launch_narrow_keys(const unsigned long long* bitmap, uint64_t words_per_col, uint64_t n_rows, uint32_t n_pheno, const uint32_t* seg_cnt,
                              uint32_t* keys_sorted, uint32_t key_cap, uint32_t row_bits, uint32_t* surv_off, uint32_t* surv_cnt,
                              uint32_t* key_count, uint32_t* tile_pref, uint32_t* meta, const unsigned long long* tested_shards, hipStream_t st) {
    static_assert(TESTED_SHARDS == 256, "block (0, 0) sums one counter per thread");
    if (n_pheno < 1 || n_pheno > NARROW_MAX_COLS) return hipErrorInvalidValue;
    const uint32_t n_words = (uint32_t)((n_rows + 63) / 64);
    const uint32_t n_segs = (n_words + BM_WORDS - 1) / BM_WORDS;
    hipLaunchKernelGGL(narrow_keys_kernel, dim3(n_segs, n_pheno), dim3(256), 0, st, bitmap, words_per_col, n_words, n_segs, n_pheno, seg_cnt,
                       keys_sorted, key_cap, row_bits, surv_off, surv_cnt, key_count, tile_pref, meta, tested_shards);
    return hipGetLastError();
}

// ---- survivors -> exact candidates, in (column, row) order --------------------------------------------------------------
// The sorted key list is cut into tiles of 256 survivors that never straddle a column (the key kernels fill tile_pref); the two
// kernels below walk the tiles with a fixed grid:
//   rescore_kernel      exact re-scoring of a tile's survivors (one lane each, the column wave-uniform), exact test
//                       against thr, threshold histogram; score (or -inf: not a candidate) to HBM, candidates per tile
//   compact_kernel      candidates to their final place: score f64 | kmer u64 | chunk-local row u32, three arrays (a tile's
//                       place = the candidates of the tiles before it, summed by the block itself; the grid's last block
//                       writes each column's range in the compacted list and their total: meta)
// The compacted arrays live in HBM; the host copies exactly `total` records per array over PCIe on a copy stream
// (the first version wrote every survivor, candidate or not, from the kernel into mapped host memory: 20 B per
// survivor over PCIe inside the compute stream, 7 ms of a 22 ms pass).
__device__ __forceinline__ uint32_t tile_column(const uint32_t* tile_pref, uint32_t n_pheno, uint32_t t) {
    uint32_t lo = 0, hi = n_pheno;  // last p with tile_pref[p] <= t
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tile_pref[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}

// Same arithmetic as score_valu_kernel: the reference's select-and-add chains, then the exact candidate test.
// One 128-sample block of the four float32 chains of calculate_kmer_score (src/kmer_general.cpp:155-167): lane l of the
// reference's SSE register adds `bit ? y : +0.0f` for samples 128 b + 32 l + 31 - s, s = 0..31, and
//   acc + (bit ? y : +0) == fma((float)bit, y, acc) for finite y (the filters only run on finite phenotypes):
// the bits of a dword become bytes 0 / 1 eight at a time ((w >> j) & 0x01010101: two lane-ops per four bits),
// v_cvt_f32_ubyteK makes 0.0f / 1.0f of one, and v_pk_fma_f32 advances two chains: 2.0 lane-ops per sample.
// The column's values are the same for every lane. YLDS: yb points into LDS (the tile's column staged there by
// rescore_kernel) and one broadcast ds_read_b128 per sample brings the four chains' values, in order. Otherwise (a column
// beyond 16 KB) they are read through the constant address space, i.e. by scalar loads into SGPRs (yb is wave-uniform).
// DESIGN.md 4.1b has what was measured about both and about the forms that are no longer here.
typedef __attribute__((address_space(4))) const float* kconst_f32p;
template <bool YLDS>
__device__ __forceinline__ void rescore_block(const uint32_t (&w)[4], const float* yb, float (&acc)[4]) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    kconst_f32p yc = (kconst_f32p)yb;
    const float4* yl = reinterpret_cast<const float4*>(yb);
    (void)yc;
    (void)yl;
    uint32_t e[4][8];
#pragma unroll
    for (int l = 0; l < 4; l++)
#pragma unroll
        for (int j = 0; j < 8; j++) e[l][j] = (w[l] >> j) & 0x01010101u;
    f32x2 a01 = {acc[0], acc[1]}, a23 = {acc[2], acc[3]};
#pragma unroll
    for (int s = 0; s < 32; s++) {
        const int b = 31 - s, j = b & 7, k = b >> 3;
        f32x2 y01, y23;
        if (YLDS) {
            const float4 yv = yl[s];
            y01 = (f32x2){yv.x, yv.y};
            y23 = (f32x2){yv.z, yv.w};
        } else {
            y01 = (f32x2){yc[4 * s], yc[4 * s + 1]};
            y23 = (f32x2){yc[4 * s + 2], yc[4 * s + 3]};
        }
        auto byte_f32 = [&](uint32_t x) {  // v_cvt_f32_ubyteK (the compiler shifts first and converts byte 0: two more ops per bit)
            float f;
            if (k == 0) asm("v_cvt_f32_ubyte0 %0, %1" : "=v"(f) : "v"(x));
            if (k == 1) asm("v_cvt_f32_ubyte1 %0, %1" : "=v"(f) : "v"(x));
            if (k == 2) asm("v_cvt_f32_ubyte2 %0, %1" : "=v"(f) : "v"(x));
            if (k == 3) asm("v_cvt_f32_ubyte3 %0, %1" : "=v"(f) : "v"(x));
            return f;
        };
        const f32x2 g01 = {byte_f32(e[0][j]), byte_f32(e[1][j])};
        const f32x2 g23 = {byte_f32(e[2][j]), byte_f32(e[3][j])};
        a01 = __builtin_elementwise_fma(g01, y01, a01);
        a23 = __builtin_elementwise_fma(g23, y23, a23);
    }
    acc[0] = a01.x;
    acc[1] = a01.y;
    acc[2] = a23.x;
    acc[3] = a23.y;
}

// a survivor's exact score from its chain sums, or -inf: not a candidate (a candidate is counted in its column's histogram)
__device__ __forceinline__ double survivor_score(const ScoreArgs& a, uint32_t p, bool valid, const float (&acc)[4], uint32_t n1) {
    const float yf = ((acc[0] + acc[1]) + acc[2]) + acc[3];
    double q, d, sc, out = -__builtin_huge_val();
    score_terms(a, yf, n1, a.sums[p], q, d);
    if (valid && mac_pass(a, n1) && candidate_score(a, p, q, d, a.thr[p], sc)) out = sc;
    return out;
}

// Rows are read in place by their own lane, 8 bytes x 2 per 128-sample block, the words of block b + 1 asked for before block
// b's lane-ops start; tiles go to the blocks round-robin. (What else was tried on the gathers, the tile order, the occupancy
// and the LDS reads, with its figures: DESIGN.md 4.1b. Left as it is.)
// DIRECT (scans of a few columns, launch_rescore_direct): the survivor's record is written at its place in the key order -
// score or -inf, k-mer, row - and nothing is counted or compacted afterwards.
template <bool YLDS, bool DIRECT>
__global__ void __launch_bounds__(256) rescore_kernel(ScoreArgs a, const uint32_t* keys, const uint32_t* surv_off, const uint32_t* surv_cnt,
                                                      const uint32_t* tile_pref, uint32_t row_mask, double* tmp_score, uint32_t* tile_cnt) {
    __shared__ uint32_t wcnt[4];
    extern __shared__ float4 ytile[];  // YLDS: the tile's column, 64 * W_m floats

    const uint32_t n_tiles = tile_pref[a.n_pheno];
    const uint32_t L = 64u * a.W_m;
    const uint32_t nblk = a.W_m / 2u;
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint32_t p = __builtin_amdgcn_readfirstlane(tile_column(tile_pref, a.n_pheno, t));
        const uint32_t i = (t - tile_pref[p]) * 256u + threadIdx.x;
        const bool valid = i < surv_cnt[p];
        const uint32_t gi = surv_off[p] + (valid ? i : 0u);
        const uint64_t r = keys[gi] & row_mask;
        const uint32_t* rp = a.src.base + r * a.src.stride_dw + a.src.off_dw;
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        uint32_t n1 = 0;
        if (YLDS) {  // (the previous tile's readers are past the barriers at the end of the turn)
            const float4* ysrc = reinterpret_cast<const float4*>(a.Yperm + (size_t)p * L);
            for (uint32_t k = threadIdx.x; k < L / 4u; k += 256u) ytile[k] = ysrc[k];
            __syncthreads();
        }
        uint2 nx[2];
        auto fetch = [&](uint32_t b) {
#pragma unroll
            for (int h = 0; h < 2; h++) {
                nx[h] = make_uint2(0u, 0u);
                if (4u * b + 2u * h + 1u < a.src.avail_dw) nx[h] = *reinterpret_cast<const uint2*>(rp + 4u * b + 2u * h);
            }
        };
        if (nblk) fetch(0);
        for (uint32_t b = 0; b < nblk; b++) {
            uint32_t w[4];
#pragma unroll
            for (int h = 0; h < 2; h++) {
                w[2 * h] = nx[h].x & a.dmask[4 * b + 2 * h];
                w[2 * h + 1] = nx[h].y & a.dmask[4 * b + 2 * h + 1];
            }
            n1 += __popc(w[0]) + __popc(w[1]) + __popc(w[2]) + __popc(w[3]);
            if (b + 1u < nblk) fetch(b + 1u);
            if (YLDS)
                rescore_block<true>(w, reinterpret_cast<const float*>(ytile) + 128u * b, acc);
            else
                rescore_block<false>(w, a.Yperm + (size_t)p * L + 128u * b, acc);
        }
        const double out = survivor_score(a, p, valid, acc, n1);
        if (DIRECT) {
            if (valid) {
                a.so_score[gi] = out;
                a.so_kmer[gi] = a.file_rows[r * a.file_stride_w];
                a.so_row[gi] = (uint32_t)r;
            }
            if (YLDS) __syncthreads();  // the next tile's column overwrites ytile
        } else {
            if (valid) tmp_score[gi] = out;
            const uint32_t c = __popcll(__ballot(out != -__builtin_huge_val()));  // the tile's candidates
            if ((threadIdx.x & 63u) == 0u) wcnt[threadIdx.x >> 6] = c;
            __syncthreads();
            if (threadIdx.x == 0) tile_cnt[t] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
            __syncthreads();
        }
    }
}

// Candidates to their final place. A tile's place in the compacted arrays is the number of candidates in the tiles before
// it: every block adds those up for itself - its first tile's prefix over tile_cnt[0 .. t), then gridDim.x - 1 more counts
// per further tile - instead of waiting for a one-block scan launch between the re-score and this kernel (16 us per chunk,
// 0.4 ms of a 100 M-row pass). The grid's extra last block writes meta: [0 .. P) candidates per column, [P .. 2P) each
// column's offset in the compacted arrays, [2P] their total, [2P + 1] the survivor keys the filter emitted (> key_cap: the
// list overflowed).
__global__ void __launch_bounds__(256) compact_kernel(ScoreArgs a, const uint32_t* keys, const uint32_t* surv_off,
                                                      const uint32_t* surv_cnt, const uint32_t* tile_pref, uint32_t row_mask,
                                                      const double* tmp_score, const uint32_t* tile_cnt, const uint32_t* key_count,
                                                      uint32_t* meta) {
    __shared__ uint32_t wcnt[4];
    __shared__ uint32_t red[4];
    __shared__ uint32_t cpre[257];
    const uint32_t n_tiles = tile_pref[a.n_pheno];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t n_workers = gridDim.x - 1u;
    if (blockIdx.x == n_workers) {
        // meta. Thread i sums the counts of tiles [i * per, (i + 1) * per); an exclusive scan over the 256 sums; a column's
        // offset is the prefix at its first tile.
        const uint32_t per = (n_tiles + 255u) / 256u;
        const uint32_t lo = threadIdx.x * per < n_tiles ? threadIdx.x * per : n_tiles;
        const uint32_t hi = lo + per < n_tiles ? lo + per : n_tiles;
        uint32_t sm = 0, all = 0;
        for (uint32_t i = lo; i < hi; i++) sm += tile_cnt[i];
        cpre[threadIdx.x] = block_scan_excl(sm, all, red);
        if (threadIdx.x == 0u) cpre[256] = all;
        __syncthreads();
        auto prefix_at = [&](uint32_t x) {  // candidates in tiles [0, x)
            if (x >= n_tiles) return cpre[256];
            const uint32_t seg = per ? x / per : 0u;
            uint32_t v = cpre[seg];
            for (uint32_t i = seg * per; i < x; i++) v += tile_cnt[i];
            return v;
        };
        for (uint32_t p = threadIdx.x; p < a.n_pheno; p += 256u) {
            const uint32_t o0 = prefix_at(tile_pref[p]), o1 = prefix_at(tile_pref[p + 1u]);
            meta[p] = o1 - o0;
            meta[a.n_pheno + p] = o0;
        }
        if (threadIdx.x == 0u) {
            meta[2u * a.n_pheno] = cpre[256];
            meta[2u * a.n_pheno + 1u] = *key_count;
        }
        return;
    }
    uint32_t base = 0, done = 0;  // candidates in tiles [0, done)
    for (uint32_t t = blockIdx.x; t < n_tiles; t += n_workers) {
        uint32_t part = 0;
        for (uint32_t i = done + threadIdx.x; i < t; i += 256u) part += tile_cnt[i];
        __syncthreads();  // (the previous turn's readers are done with red)
        base += block_sum(part, red);
        done = t;
        if (tile_cnt[t] == 0u) continue;  // block-uniform: no candidate in this tile
        const uint32_t p = __builtin_amdgcn_readfirstlane(tile_column(tile_pref, a.n_pheno, t));  // the column's values come by scalar loads
        const uint32_t i = (t - tile_pref[p]) * 256u + threadIdx.x;
        const bool valid = i < surv_cnt[p];
        const uint32_t gi = surv_off[p] + (valid ? i : 0u);
        const double sc = valid ? tmp_score[gi] : -__builtin_huge_val();
        const bool is_cand = sc != -__builtin_huge_val();
        const unsigned long long bal = __ballot(is_cand);
        if (lane == 0) wcnt[wave] = __popcll(bal);
        __syncthreads();
        uint32_t before = __popcll(bal & ((1ull << lane) - 1ull));
        for (uint32_t w = 0; w < wave; w++) before += wcnt[w];
        if (is_cand) {
            const uint32_t r = keys[gi] & row_mask;
            const uint32_t o = base + before;
            a.so_score[o] = sc;
            a.so_kmer[o] = a.file_rows[(uint64_t)r * a.file_stride_w];
            a.so_row[o] = r;
        }
        __syncthreads();
    }
}

// The re-score kernel of a launch and its dynamic LDS: the tile's column goes through LDS while it fits beside eight blocks per
// CU (16 KB: 4096 samples); beyond, scalar loads. The grids are fixed, tiles handed out round-robin (the tile count is only
// known on the device).
using RescoreKernel = void (*)(ScoreArgs, const uint32_t*, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t, double*, uint32_t*);
template <bool DIRECT>
static RescoreKernel pick_rescore(const ScoreArgs& a, size_t& lds) {
    const size_t ybytes = 64u * (size_t)a.W_m * sizeof(float);
    const bool ylds = ybytes <= 16384u;
    lds = ylds ? ybytes : 0;
    return ylds ? rescore_kernel<true, DIRECT> : rescore_kernel<false, DIRECT>;
}

hipError_t launch_rescore(const ScoreArgs& a, const uint32_t* keys, const uint32_t* surv_off, const uint32_t* surv_cnt,
                          uint32_t row_bits, uint32_t* tile_pref, uint32_t* tile_cnt, double* tmp_score,
                          const uint32_t* key_count, uint32_t* meta, hipStream_t st) {
    if (a.n_pheno == 0) return hipSuccess;
    const uint32_t row_mask = row_bits >= 32 ? 0xFFFFFFFFu : ((1u << row_bits) - 1u);
    size_t lds;
    const RescoreKernel k = pick_rescore<false>(a, lds);
    hipLaunchKernelGGL(k, dim3(2048), dim3(256), lds, st, a, keys, surv_off, surv_cnt, tile_pref, row_mask, tmp_score, tile_cnt);  // 8 blocks of 256 per CU
    launch_last(compact_kernel, dim3(2048 + 1), dim3(256), 0, st, a, keys, surv_off, surv_cnt, tile_pref, row_mask, tmp_score,
                       tile_cnt, key_count, meta);
    return hipGetLastError();
}

hipError_t launch_rescore_direct(const ScoreArgs& a, const uint32_t* keys, const uint32_t* surv_off, const uint32_t* surv_cnt,
                                 uint32_t row_bits, const uint32_t* tile_pref, hipStream_t st) {
    if (a.n_pheno == 0) return hipSuccess;
    const uint32_t row_mask = row_bits >= 32 ? 0xFFFFFFFFu : ((1u << row_bits) - 1u);
    size_t lds;
    const RescoreKernel k = pick_rescore<true>(a, lds);
    // (a few tiles per launch: a small grid - an empty block costs its launch slot, and a scan of a few columns is made of
    // these launches)
    launch_last(k, dim3(512), dim3(256), lds, st, a, keys, surv_off, surv_cnt, tile_pref, row_mask, (double*)nullptr, (uint32_t*)nullptr);
    return hipGetLastError();
}

// One launch instead of a handful of small memsets per chunk: counters of the next chunk, its survivors' bitmap, the narrow
// filter's per-segment counts.
__global__ void __launch_bounds__(256) chunk_prep_kernel(uint32_t* cand_cnt, uint32_t n_pheno, unsigned long long* tested, uint32_t* key_count,
                                                         unsigned long long* bitmap, uint64_t bitmap_words, uint32_t* seg_cnt, uint32_t n_seg_words,
                                                         PrepThr tu) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_pheno) cand_cnt[i] = 0u;
    if (i < TESTED_SHARDS) tested[i] = 0ull;
    if (i == 0 && key_count) *key_count = 0u;
    if (i < n_seg_words) seg_cnt[i] = 0u;
    // the bitmap, two words (16 bytes) per thread and turn
    ulonglong2* b2 = reinterpret_cast<ulonglong2*>(bitmap);
    const uint64_t pairs = bitmap_words / 2u;
    for (uint64_t k = i; k < pairs; k += (uint64_t)gridDim.x * blockDim.x) b2[k] = make_ulonglong2(0ull, 0ull);
    if (i == 0 && (bitmap_words & 1u)) bitmap[bitmap_words - 1u] = 0ull;
    // the thresholds the chunk is filtered against, raised from the histograms of everything counted so far
    if (tu.hist)
        for (uint32_t p = blockIdx.x; p < n_pheno; p += gridDim.x) thr_update_block(tu.hist, tu.hist_base, tu.bins, tu.topn, tu.thr_host, tu.thr, p);
}

hipError_t launch_chunk_prep(uint32_t* cand_cnt, uint32_t n_pheno, unsigned long long* tested, uint32_t* key_count,
                             unsigned long long* bitmap, uint64_t bitmap_words, uint32_t* seg_cnt, uint32_t n_seg_words, const PrepThr& tu,
                             hipStream_t st) {
    uint64_t n = n_pheno > TESTED_SHARDS ? n_pheno : TESTED_SHARDS;
    if (n_seg_words > n) n = n_seg_words;
    if (bitmap_words / 8u > n) n = bitmap_words / 8u;  // (four turns per thread on a large bitmap)
    const uint64_t blocks = std::min<uint64_t>((n + 255u) / 256u, 8192u);
    if (blocks * 256u < std::max<uint64_t>(std::max<uint64_t>(n_pheno, TESTED_SHARDS), n_seg_words)) return hipErrorInvalidValue;
    if (tu.hist && (tu.bins % 1024u || tu.bins / 256u > 64u)) return hipErrorInvalidValue;
    launch_last(chunk_prep_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, cand_cnt, n_pheno, tested, key_count, bitmap, bitmap_words,
                       seg_cnt, n_seg_words, tu);
    return hipGetLastError();
}

}  // namespace kgwas
