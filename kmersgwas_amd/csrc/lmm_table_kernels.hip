// lmm_table_kernels.hip — the front end of lmm_lrt --kmers_table: rows of a k-mers table, squeezed to phenotype order
// (squeeze_kernel, aux_kernels.hip), become what lmm_rotate_kernel / lmm_grid_kernel / lmm_refine_kernel consume - for the
// tested rows alone, compacted ("The table front end").
//
// A row is tested iff kmers_table_to_bed would write it AND lmm_prep_kernel would then test it:
//     S >= min_count && n1 >= min_count && n1 <= S - min_count                         (table_to_bed.cpp's MAC filter)
//     mean = (double)(2 (S - n1)) / (double)S, af = 0.5 mean, not constant, fmin(af, 1 - af) >= maf   (lmm_prep_kernel, its own
//     expressions: presence is code 11, absence code 00, so c[0] = S - n1, c[1] = c[2] = 0, c[3] = n1 and no call is missing)
//
//   lmm_table_flag_kernel  one lane per row: n1 (popcount of the squeezed row), the flag, and per block of 256 rows the number
//                          of tested rows (wave ballots, then four LDS values);
//   lmm_table_scan_kernel  one block: the exclusive prefix sum of the block counts, and the piece's total;
//   lmm_table_emit_kernel  per block of 256 rows: a tested row's slot is its block's offset plus its rank in the block (ballot
//                          and popcount below the lane), so slots follow the row order - the same content in every run. The row's
//                          lane writes the LmmVariant, the table row index and the k-mer word; then the block writes the padded
//                          2-bit code rows, one dword (16 accessions, every presence bit doubled) per lane and step.
// Wherever flags are only counted, lmm_table_count_kernel<P> stands for the flag kernel: per block of 256 elements the number that
// meet the predicate P, and the scan kernel behind it (count_and_scan).
// And the first stage of the selection of the multi-phenotype pass (kgwas_lmm_test_table_multi), by the same scheme:
//   lmm_table_count_kernel<lmm_table_select_count>, lmm_table_scan_kernel   one lane per (column, row) pair of a refined block:
//                              does it pass its column's threshold; the offsets and the number of survivors;
//   lmm_table_select_kernel    a surviving pair's lane writes its record at offset + rank, so records follow the (column, row)
//                              order and are the same in every run.
// And the pattern table, the set of the code rows met so far in a call (launch_lmm_pattern_lookup, once per piece):
//   lmm_pattern_hash_kernel      one wave per tested row: its 64-bit tag;
//   lmm_pattern_claim_kernel     one lane per row: the slot of its tag (atomicCAS along a linear probe sequence of 16 slots) and, by
//                                atomicMin, the slot's owner - the smallest row of the piece that reached it;
//   lmm_pattern_publish_kernel   an owner's code row goes into its new slot;
//   lmm_pattern_classify_kernel  one wave per row: owner, equal (the whole code row equals the slot's), collided or rejected;
//   lmm_table_count_kernel<lmm_pattern_count>, lmm_table_scan_kernel, lmm_pattern_emit_kernel   the rows to compute - every row
//                                but the equal ones (of a dead slot, where slots have a state) - compacted in row order.
// To which the pattern cache of kgwas_lmm_test_table_unique adds a result per slot, so that each distinct code row goes through the
// back end once:
//   lmm_cache_scatter_kernel   a sub-chunk's results go back to the rows' places and into the owners' slots;
//   lmm_cache_fanout_kernel    the rows from cache take their slot's result; the piece's new slots get owner 0.
// And the dead-pattern skip of kgwas_lmm_test_table_multi_skip a state word per slot, by which an equal row is dead or live:
//   lmm_skip_gather_kernel     a row to compute takes its table row index and k-mer word along;
//   lmm_skip_flag_kernel       after a column block's refinement: the rows of which the select kernel ships a pair;
//   lmm_skip_mark_kernel       after a sub-chunk's last column block: the slot of an owner or live row that shipped nothing is dead;
//   lmm_table_count_kernel<lmm_skip_dead_count>, lmm_table_scan_kernel   the number of dead slots, once per call.
// No scalar memory write: every value goes out through a vector store from plain C++. The two atomics of lmm_pattern_claim_kernel
// are the only ones.
#include "lmm_kernels.h"

namespace kgwas {

namespace {

constexpr uint32_t TB = LMM_TABLE_BLOCK;  // rows per block of the flag and emit kernels
constexpr uint32_t FLAG_BIT = 0x80000000u;

// 16 presence bits -> 16 two-bit codes (11 / 00), accession k of the 16 at bits 2k, 2k + 1: the bytes of bed_bytes_kernel
__device__ inline uint32_t spread16(uint32_t x) {
    x = (x | (x << 8)) & 0x00FF00FFu;
    x = (x | (x << 4)) & 0x0F0F0F0Fu;
    x = (x | (x << 2)) & 0x33333333u;
    x = (x | (x << 1)) & 0x55555555u;
    return x | (x << 1);
}

// the number of set flags in the block's lanes below this one; s_wave: 4 values of LDS. Every lane of the block must call it.
__device__ inline uint32_t block_rank(bool flag, uint32_t* s_wave, uint32_t& block_total) {
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned long long mask = __ballot(flag);
    if (lane == 0) s_wave[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (uint32_t w = 0; w < TB / 64; w++) {
        before += w < wave ? s_wave[w] : 0u;
        total += s_wave[w];
    }
    block_total = total;
    return before + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
}

__global__ void __launch_bounds__(TB) lmm_table_flag_kernel(const uint32_t* __restrict__ sq, uint32_t n_rows, uint32_t ndw, uint32_t S,
                                                            uint32_t min_count, double maf, uint32_t* __restrict__ n1flag,
                                                            uint32_t* __restrict__ block_cnt) {
    __shared__ uint32_t s_wave[TB / 64];
    const uint32_t r = blockIdx.x * TB + threadIdx.x;
    bool tested = false;
    if (r < n_rows) {
        const uint4* row = reinterpret_cast<const uint4*>(sq + (uint64_t)r * ndw);  // (ndw is a multiple of 4: 16-byte rows)
        uint32_t n1 = 0;
        for (uint32_t k = 0; k < ndw / 4; k++) {
            const uint4 w = row[k];
            n1 += __popc(w.x) + __popc(w.y) + __popc(w.z) + __popc(w.w);
        }
        const bool written = S >= min_count && n1 >= min_count && n1 <= S - min_count;  // kmers_table_to_bed
        const double mean = (double)(2u * (S - n1)) / (double)S;                          // lmm_prep_kernel: nn = S, c[2] = 0
        const double af = 0.5 * mean;
        const bool constant = S == 0 || n1 == 0 || n1 == S;
        tested = written && !constant && fmin(af, 1.0 - af) >= maf;
        n1flag[r] = n1 | (tested ? FLAG_BIT : 0u);
    }
    uint32_t total;
    (void)block_rank(tested, s_wave, total);
    if (threadIdx.x == 0) block_cnt[blockIdx.x] = total;
}

// block_off[b] = sum of block_cnt[0 .. b), total[0] = the sum of all n_blocks counts. One block of 256 lanes.
__global__ void __launch_bounds__(256) lmm_table_scan_kernel(const uint32_t* __restrict__ block_cnt, uint32_t n_blocks,
                                                             uint32_t* __restrict__ block_off, uint32_t* __restrict__ total) {
    __shared__ uint32_t s_wave[4];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t carry = 0;
    for (uint32_t b0 = 0; b0 < n_blocks; b0 += 256) {
        const uint32_t b = b0 + threadIdx.x;
        const uint32_t v = b < n_blocks ? block_cnt[b] : 0u;
        uint32_t incl = v;  // inclusive scan within the wave
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        uint32_t before = carry, tile = 0;
        for (uint32_t w = 0; w < 4; w++) {
            before += w < wave ? s_wave[w] : 0u;
            tile += s_wave[w];
        }
        if (b < n_blocks) block_off[b] = before + incl - v;
        carry += tile;
        __syncthreads();  // (s_wave is written again in the next round)
    }
    if (threadIdx.x == 0) total[0] = carry;
}

// block_cnt[b] = the number of elements e of block b, e < n, with pred(e)
template <class Pred>
__global__ void __launch_bounds__(TB) lmm_table_count_kernel(Pred pred, uint32_t n, uint32_t* __restrict__ block_cnt) {
    __shared__ uint32_t s_wave[TB / 64];
    const uint32_t e = blockIdx.x * TB + threadIdx.x;
    const bool keep = e < n && pred(e);
    uint32_t total;
    (void)block_rank(keep, s_wave, total);
    if (threadIdx.x == 0) block_cnt[blockIdx.x] = total;
}

// the count and the scan over n > 0 elements: block_off for an emit kernel with the same predicate, total[0] = how many meet it
template <class Pred>
void count_and_scan(Pred pred, uint32_t n, uint32_t* block_cnt, uint32_t* block_off, uint32_t* total, hipStream_t st) {
    const uint32_t n_blocks = (n + TB - 1) / TB;
    hipLaunchKernelGGL(lmm_table_count_kernel<Pred>, dim3(n_blocks), dim3(TB), 0, st, pred, n, block_cnt);
    hipLaunchKernelGGL(lmm_table_scan_kernel, dim3(1), dim3(256), 0, st, block_cnt, n_blocks, block_off, total);
}

__global__ void __launch_bounds__(TB) lmm_table_emit_kernel(const uint64_t* __restrict__ rows, uint64_t stride,
                                                            const uint32_t* __restrict__ sq, uint32_t n_rows, uint32_t ndw, uint32_t S,
                                                            uint64_t first_row, const uint32_t* __restrict__ n1flag,
                                                            const uint32_t* __restrict__ block_off, uint32_t bpsp,
                                                            uint32_t* __restrict__ codes, LmmVariant* __restrict__ vars,
                                                            uint64_t* __restrict__ row_out, uint64_t* __restrict__ kmer_out) {
    __shared__ uint32_t s_wave[TB / 64];
    __shared__ uint32_t s_slot[TB];
    const uint32_t row0 = blockIdx.x * TB, r = row0 + threadIdx.x;
    const uint32_t nf = r < n_rows ? n1flag[r] : 0u;
    const bool tested = (nf & FLAG_BIT) != 0u;
    uint32_t total;
    const uint32_t slot = block_off[blockIdx.x] + block_rank(tested, s_wave, total);
    s_slot[threadIdx.x] = tested ? slot : 0xFFFFFFFFu;
    if (tested) {
        const uint32_t n1 = nf & ~FLAG_BIT;
        const double mean = (double)(2u * (S - n1)) / (double)S;  // as lmm_prep_kernel: (2 c[0] + c[2]) / nn
        LmmVariant o;
        o.val[0] = 2.0 - mean;
        o.val[1] = 0.0;
        o.val[2] = 1.0 - mean;
        o.val[3] = 0.0 - mean;
        o.af = 0.5 * mean;
        o.n_miss = 0;
        o.tested = 1;
        vars[slot] = o;
        row_out[slot] = first_row + r;
        kmer_out[slot] = rows[(uint64_t)r * stride];
    }
    __syncthreads();
    if (total == 0) return;  // (block-uniform)
    const uint32_t ndc = bpsp / 4;  // code dwords per row; dword j holds accessions 16 j .. 16 j + 15 (zero past S: the squeeze pads)
    for (uint32_t e = threadIdx.x; e < TB * ndc; e += TB) {
        const uint32_t rr = e / ndc, j = e - rr * ndc;
        const uint32_t s = s_slot[rr];
        if (s == 0xFFFFFFFFu) continue;
        const uint32_t bits = (sq[(uint64_t)(row0 + rr) * ndw + (j >> 1)] >> (16u * (j & 1u))) & 0xFFFFu;
        codes[(uint64_t)s * ndc + j] = spread16(bits);
    }
}

// ---- the selection's first stage of the multi-phenotype pass ("The multi-phenotype table pass") ----
// Element e = c cc + v is the pair (column c of the block, compacted row v), so the element order is the (column, row) order.

// does element e < n survive? The comparison is false for a NaN lrt, which therefore survives only into an open heap.
__device__ inline bool select_survives(const double* __restrict__ lrt, const LmmSelectCol* __restrict__ cols, uint32_t cc, uint32_t e,
                                       uint32_t n) {
    if (e >= n) return false;
    const LmmSelectCol sc = cols[e / cc];
    return sc.open != 0u || lrt[e] > sc.thr;
}

struct lmm_table_select_count {
    const double* lrt;
    const LmmSelectCol* cols;
    uint32_t cc, n;
    __device__ bool operator()(uint32_t e) const { return select_survives(lrt, cols, cc, e, n); }
};

// a survivor's slot is its block's offset plus its rank in the block: slots follow the element order. Its lane writes the record.
__global__ void __launch_bounds__(TB) lmm_table_select_kernel(const double* __restrict__ lrt, const double* __restrict__ lam,
                                                              const double* __restrict__ p, const LmmSelectCol* __restrict__ cols,
                                                              uint32_t cc, uint32_t n, const LmmVariant* __restrict__ vars,
                                                              const uint64_t* __restrict__ row, const uint64_t* __restrict__ kmer,
                                                              const uint32_t* __restrict__ block_off, LmmTableRecord* __restrict__ rec,
                                                              uint32_t cap) {
    __shared__ uint32_t s_wave[TB / 64];
    const uint32_t e = blockIdx.x * TB + threadIdx.x;
    const bool keep = select_survives(lrt, cols, cc, e, n);
    uint32_t total;
    const uint32_t slot = block_off[blockIdx.x] + block_rank(keep, s_wave, total);
    if (!keep || slot >= cap) return;
    const uint32_t c = e / cc, v = e - c * cc;
    LmmTableRecord o;
    o.lrt = lrt[e];
    o.lam = lam[e];
    o.p = p[e];
    o.af = vars[v].af;
    o.row = row[v];
    o.kmer = kmer[v];
    o.col = c;
    o.pad = 0;
    rec[slot] = o;
}

// ---- the pattern table of the pattern cache and of the dead-pattern skip ("The pattern table") ----
// Atomics stand in lmm_pattern_claim_kernel alone, and there a word an atomic touches is never loaded plainly; everything else one
// kernel leaves for another crosses a kernel boundary on the one stream. Every loop has a bound no other thread can move. A state
// word is written by lmm_skip_mark_kernel (only ever the value 1) and read by the classify of the NEXT piece.

__device__ inline uint64_t mix64(uint64_t x) {  // the finaliser of splitmix64
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// One wave per row: the tag is a mix of the sum, over the row's dwords, of a mix of (place, dword); a sum of integers, so the same
// in any order. Never 0, which marks an empty slot.
__global__ void __launch_bounds__(TB) lmm_pattern_hash_kernel(const uint32_t* __restrict__ codes, uint32_t total, uint32_t ndc,
                                                              uint64_t tag_mask, unsigned long long* __restrict__ row_tag) {
    const uint32_t t = blockIdx.x * (TB / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (t >= total) return;  // (wave-uniform)
    unsigned long long acc = 0;
    for (uint32_t j = lane; j < ndc; j += 64) acc += mix64(((uint64_t)(j + 1) << 32) | codes[(uint64_t)t * ndc + j]);
#pragma unroll
    for (uint32_t d = 32; d; d >>= 1) acc += __shfl_xor(acc, d, 64);
    const unsigned long long tag = mix64(acc) & tag_mask;
    if (lane == 0) row_tag[t] = tag ? tag : 1ull;
}

// One lane per row. The probe sequence is a function of the tag alone, and a slot's tag never changes once set, so a tag ends in
// the same slot all through a call. The owner of a slot new in this piece is the smallest row that reached it; a slot of an
// earlier piece has owner 0, which the min leaves.
__global__ void __launch_bounds__(TB) lmm_pattern_claim_kernel(const unsigned long long* __restrict__ row_tag, uint32_t total, LmmCache c,
                                                               uint32_t* __restrict__ slot_of) {
    const uint32_t t = blockIdx.x * TB + threadIdx.x;
    if (t >= total) return;
    const unsigned long long mine = row_tag[t];
    const uint32_t mask = c.slots - 1u, first = (uint32_t)(mix64(mine) >> 32) & mask;
    uint32_t found = LMM_CACHE_NONE;
    for (uint32_t i = 0; i < LMM_CACHE_PROBES && found == LMM_CACHE_NONE; i++) {
        const uint32_t s = (first + i) & mask;
        const unsigned long long old = atomicCAS(&c.tag[s], 0ull, mine);
        if (old == 0ull || old == mine) found = s;
    }
    if (found != LMM_CACHE_NONE) (void)atomicMin(&c.owner[found], t + 1u);
    slot_of[t] = found;
}

// One lane per (row, dword): an owner's code row goes into its slot.
__global__ void __launch_bounds__(TB) lmm_pattern_publish_kernel(const uint32_t* __restrict__ codes, uint32_t total, uint32_t ndc,
                                                                 const uint32_t* __restrict__ slot_of, LmmCache c) {
    const uint64_t e = (uint64_t)blockIdx.x * TB + threadIdx.x;
    const uint64_t t = e / ndc;
    if (t >= total) return;
    const uint32_t s = slot_of[t];
    if (s >= c.slots || c.owner[s] != (uint32_t)t + 1u) return;
    c.key[(uint64_t)s * ndc + (e - t * ndc)] = codes[e];
}

// One wave per row: every row that reached a slot and is not its owner compares its whole code row with the slot's. Where slots
// have a state it is read as it was when the piece began: no kernel between this one and the piece before writes it.
__global__ void __launch_bounds__(TB) lmm_pattern_classify_kernel(const uint32_t* __restrict__ codes, uint32_t total, uint32_t ndc,
                                                                  const uint32_t* __restrict__ slot_of, LmmCache c,
                                                                  uint32_t* __restrict__ cls) {
    const uint32_t t = blockIdx.x * (TB / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (t >= total) return;  // (wave-uniform, as every branch below)
    const uint32_t s = slot_of[t];
    uint32_t kind;
    if (s >= c.slots) {
        kind = LMM_ROW_REJECTED;
    } else if (c.owner[s] == t + 1u) {
        kind = LMM_ROW_OWNER;
    } else {
        uint32_t diff = 0;
        for (uint32_t j = lane; j < ndc; j += 64) diff |= codes[(uint64_t)t * ndc + j] ^ c.key[(uint64_t)s * ndc + j];
        if (__ballot(diff != 0u))
            kind = LMM_ROW_COLLIDED;
        else if (!c.state)  // (a kernel argument)
            kind = LMM_ROW_CACHED;
        else
            kind = c.state[s] != 0u ? LMM_ROW_DEAD : LMM_ROW_LIVE;
    }
    if (lane == 0) cls[t] = kind;
}

// The rows to compute, compacted by the scheme of the front end: the count per block of 256 rows, lmm_table_scan_kernel, the emit.
struct lmm_pattern_count {
    const uint32_t* cls;
    __device__ bool operator()(uint32_t t) const { return cls[t] != LMM_ROW_CACHED; }  // (LMM_ROW_DEAD is the same value)
};

__global__ void __launch_bounds__(TB) lmm_pattern_emit_kernel(const uint32_t* __restrict__ codes, const LmmVariant* __restrict__ vars,
                                                              const uint32_t* __restrict__ cls, uint32_t total, uint32_t ndc,
                                                              const uint32_t* __restrict__ block_off, uint32_t* __restrict__ codes2,
                                                              LmmVariant* __restrict__ vars2, uint32_t* __restrict__ back) {
    __shared__ uint32_t s_wave[TB / 64];
    __shared__ uint32_t s_slot[TB];
    const uint32_t row0 = blockIdx.x * TB, t = row0 + threadIdx.x;
    const bool rotate = t < total && lmm_pattern_count{cls}(t);
    uint32_t n;
    const uint32_t slot = block_off[blockIdx.x] + block_rank(rotate, s_wave, n);  // (<= t: at most t rows stand before row t)
    s_slot[threadIdx.x] = rotate && slot < total ? slot : LMM_CACHE_NONE;
    if (rotate && slot < total) {
        vars2[slot] = vars[t];
        back[slot] = t;
    }
    __syncthreads();
    if (n == 0) return;  // (block-uniform)
    for (uint32_t e = threadIdx.x; e < TB * ndc; e += TB) {
        const uint32_t rr = e / ndc, j = e - rr * ndc;
        const uint32_t s = s_slot[rr];
        if (s == LMM_CACHE_NONE) continue;
        codes2[(uint64_t)s * ndc + j] = codes[(uint64_t)(row0 + rr) * ndc + j];
    }
}

// One lane per row of a sub-chunk that went through the back end.
__global__ void __launch_bounds__(TB) lmm_cache_scatter_kernel(const double* __restrict__ lrt, const double* __restrict__ lam,
                                                               const double* __restrict__ p, uint32_t cc, const uint32_t* __restrict__ back,
                                                               const uint32_t* __restrict__ slot_of, const uint32_t* __restrict__ cls,
                                                               uint32_t total, LmmCache c, double* __restrict__ r_lrt,
                                                               double* __restrict__ r_lam, double* __restrict__ r_p) {
    const uint32_t v = blockIdx.x * TB + threadIdx.x;
    if (v >= cc) return;
    const uint32_t t = back[v];
    if (t >= total) return;
    const double a = lrt[v], b = lam[v], q = p[v];
    r_lrt[t] = a;
    r_lam[t] = b;
    r_p[t] = q;
    const uint32_t s = slot_of[t];
    if (cls[t] != LMM_ROW_OWNER || s >= c.slots) return;
    c.res[3ull * s] = a;
    c.res[3ull * s + 1] = b;
    c.res[3ull * s + 2] = q;
}

// One lane per row of the piece, after its last sub-chunk (an owner may stand in a later sub-chunk than its copies).
__global__ void __launch_bounds__(TB) lmm_cache_fanout_kernel(const uint32_t* __restrict__ slot_of, const uint32_t* __restrict__ cls,
                                                              uint32_t total, LmmCache c, double* __restrict__ r_lrt,
                                                              double* __restrict__ r_lam, double* __restrict__ r_p) {
    const uint32_t t = blockIdx.x * TB + threadIdx.x;
    if (t >= total) return;
    const uint32_t s = slot_of[t], kind = cls[t];
    if (s >= c.slots) return;
    if (kind == LMM_ROW_CACHED) {
        r_lrt[t] = c.res[3ull * s];
        r_lam[t] = c.res[3ull * s + 1];
        r_p[t] = c.res[3ull * s + 2];
    } else if (kind == LMM_ROW_OWNER) {
        c.owner[s] = 0u;
    }
}

// ---- the dead-pattern skip of kgwas_lmm_test_table_multi_skip ("The dead-pattern skip") ----
// The rules of the pattern table hold; the state words of the table are this section's.

// One lane per compacted row: the table row index and the k-mer word follow the row (lmm_pattern_emit_kernel left back[v] <= v).
__global__ void __launch_bounds__(TB) lmm_skip_gather_kernel(const uint32_t* __restrict__ back, const uint32_t* __restrict__ total2,
                                                             uint32_t total, const uint64_t* __restrict__ row,
                                                             const uint64_t* __restrict__ kmer, uint64_t* __restrict__ row2,
                                                             uint64_t* __restrict__ kmer2) {
    const uint32_t v = blockIdx.x * TB + threadIdx.x;
    if (v >= total || v >= total2[0]) return;
    const uint32_t t = back[v];
    if (t >= total) return;
    row2[v] = row[t];
    kmer2[v] = kmer[t];
}

// One lane per row of the sub-chunk: does lmm_table_select_kernel ship a pair of it in this block of pb columns? The lanes that
// store all store 1.
__global__ void __launch_bounds__(TB) lmm_skip_flag_kernel(const double* __restrict__ lrt, const LmmSelectCol* __restrict__ cols,
                                                           uint32_t cc, uint32_t pb, uint32_t* __restrict__ shipped) {
    const uint32_t v = blockIdx.x * TB + threadIdx.x;
    if (v >= cc) return;
    bool any = false;
    for (uint32_t k = 0; k < LMM_PBLOCK; k++)
        if (k < pb) any |= select_survives(lrt, cols, cc, k * cc + v, pb * cc);
    if (any) shipped[v] = 1u;
}

// One lane per row of a sub-chunk after its last column block.
__global__ void __launch_bounds__(TB) lmm_skip_mark_kernel(const uint32_t* __restrict__ shipped, uint32_t cc,
                                                           const uint32_t* __restrict__ back, const uint32_t* __restrict__ slot_of,
                                                           const uint32_t* __restrict__ cls, uint32_t total, LmmCache c) {
    const uint32_t v = blockIdx.x * TB + threadIdx.x;
    if (v >= cc) return;
    const uint32_t t = back[v];
    if (t >= total) return;
    const uint32_t s = slot_of[t], kind = cls[t];
    if (s >= c.slots || (kind != LMM_ROW_OWNER && kind != LMM_ROW_LIVE)) return;  // (a collided or rejected row has no slot of its own)
    if (kind == LMM_ROW_OWNER) c.owner[s] = 0u;
    if (shipped[v] == 0u) c.state[s] = 1u;
}

struct lmm_skip_dead_count {  // is slot s dead
    const uint32_t* state;
    __device__ bool operator()(uint32_t s) const { return state[s] != 0u; }
};

}  // namespace

hipError_t launch_lmm_pattern_lookup(const uint8_t* codes, const LmmVariant* vars, const uint64_t* row, const uint64_t* kmer, uint32_t total,
                                     LmmDims dm, uint64_t tag_mask, LmmCache c, LmmPiece pc, hipStream_t st) {
    // (total2 would stay unwritten; a slot index must fit 31 bits; an empty mask would leave the one tag 1)
    if (!total || total >= (1u << 31) || dm.bpsp % 4u || !dm.bpsp || c.slots < 64u || c.slots > (1u << 30) || (c.slots & (c.slots - 1u)) ||
        !tag_mask)
        return hipErrorInvalidValue;
    const bool gather = pc.row2 || pc.kmer2;
    if (gather && !(pc.row2 && pc.kmer2 && row && kmer)) return hipErrorInvalidValue;
    const uint32_t ndc = dm.bpsp / 4, n_blocks = (total + TB - 1) / TB, n_waves = (total + TB / 64 - 1) / (TB / 64);
    const uint64_t n_words = ((uint64_t)total * ndc + TB - 1) / TB;
    if (n_words >= (1ull << 31)) return hipErrorInvalidValue;
    const uint32_t* cw = reinterpret_cast<const uint32_t*>(codes);
    hipLaunchKernelGGL(lmm_pattern_hash_kernel, dim3(n_waves), dim3(TB), 0, st, cw, total, ndc, tag_mask, pc.row_tag);
    hipLaunchKernelGGL(lmm_pattern_claim_kernel, dim3(n_blocks), dim3(TB), 0, st, pc.row_tag, total, c, pc.slot_of);
    hipLaunchKernelGGL(lmm_pattern_publish_kernel, dim3((uint32_t)n_words), dim3(TB), 0, st, cw, total, ndc, pc.slot_of, c);
    hipLaunchKernelGGL(lmm_pattern_classify_kernel, dim3(n_waves), dim3(TB), 0, st, cw, total, ndc, pc.slot_of, c, pc.cls);
    count_and_scan(lmm_pattern_count{pc.cls}, total, pc.block_cnt, pc.block_off, pc.total2, st);
    hipLaunchKernelGGL(lmm_pattern_emit_kernel, dim3(n_blocks), dim3(TB), 0, st, cw, vars, pc.cls, total, ndc, pc.block_off,
                       reinterpret_cast<uint32_t*>(pc.codes2), pc.vars2, pc.back);
    if (gather)
        hipLaunchKernelGGL(lmm_skip_gather_kernel, dim3(n_blocks), dim3(TB), 0, st, pc.back, pc.total2, total, row, kmer, pc.row2, pc.kmer2);
    return hipGetLastError();
}

hipError_t launch_lmm_cache_scatter(const double* lrt, const double* lam, const double* p, uint32_t first, uint32_t cc, uint32_t total,
                                    LmmCache c, LmmPiece pc, double* r_lrt, double* r_lam, double* r_p, hipStream_t st) {
    if (!cc || cc > total || first > total - cc || !c.res) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lmm_cache_scatter_kernel, dim3((cc + TB - 1) / TB), dim3(TB), 0, st, lrt, lam, p, cc, pc.back + first, pc.slot_of,
                       pc.cls, total, c, r_lrt, r_lam, r_p);
    return hipGetLastError();
}

hipError_t launch_lmm_cache_fanout(uint32_t total, LmmCache c, LmmPiece pc, double* r_lrt, double* r_lam, double* r_p, hipStream_t st) {
    if (!total || !c.res) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lmm_cache_fanout_kernel, dim3((total + TB - 1) / TB), dim3(TB), 0, st, pc.slot_of, pc.cls, total, c, r_lrt, r_lam, r_p);
    return hipGetLastError();
}

hipError_t launch_lmm_skip_flag(const double* lrt, const LmmSelectCol* cols, uint32_t cc, uint32_t pb, uint32_t* shipped, hipStream_t st) {
    if (!cc || !pb || pb > LMM_PBLOCK || (uint64_t)pb * cc >= (1ull << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lmm_skip_flag_kernel, dim3((cc + TB - 1) / TB), dim3(TB), 0, st, lrt, cols, cc, pb, shipped);
    return hipGetLastError();
}

hipError_t launch_lmm_skip_mark(const uint32_t* shipped, uint32_t first, uint32_t cc, uint32_t total, LmmCache c, LmmPiece pc,
                                hipStream_t st) {
    if (!cc || cc > total || first > total - cc || !c.state) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lmm_skip_mark_kernel, dim3((cc + TB - 1) / TB), dim3(TB), 0, st, shipped, cc, pc.back + first, pc.slot_of, pc.cls, total,
                       c);
    return hipGetLastError();
}

hipError_t launch_lmm_skip_count_dead(LmmCache c, uint32_t* block_cnt, uint32_t* block_off, uint32_t* dead, hipStream_t st) {
    if (c.slots < 64u || c.slots > (1u << 30) || !c.state) return hipErrorInvalidValue;
    count_and_scan(lmm_skip_dead_count{c.state}, c.slots, block_cnt, block_off, dead, st);
    return hipGetLastError();
}

hipError_t launch_lmm_table_select(const double* lrt, const double* lam, const double* p, uint32_t cc, uint32_t pb, const LmmVariant* vars,
                                   const uint64_t* row, const uint64_t* kmer, const LmmSelectCol* cols, uint32_t* block_cnt,
                                   uint32_t* block_off, uint32_t* count, LmmTableRecord* rec, uint32_t cap, hipStream_t st) {
    if (!cc || !pb || pb > LMM_PBLOCK || (uint64_t)pb * cc >= (1ull << 31)) return hipErrorInvalidValue;  // (count would stay unwritten)
    const uint32_t n = pb * cc, n_blocks = (n + TB - 1) / TB;
    count_and_scan(lmm_table_select_count{lrt, cols, cc, n}, n, block_cnt, block_off, count, st);
    hipLaunchKernelGGL(lmm_table_select_kernel, dim3(n_blocks), dim3(TB), 0, st, lrt, lam, p, cols, cc, n, vars, row, kmer, block_off, rec,
                       cap);
    return hipGetLastError();
}

hipError_t launch_lmm_table_front(const uint64_t* rows, uint64_t stride, const uint32_t* sq, uint32_t n_rows, uint32_t W_m, LmmDims dm,
                                  uint64_t first_row, uint32_t min_count, double maf, uint32_t* n1flag, uint32_t* block_cnt,
                                  uint32_t* block_off, uint32_t* total, uint8_t* codes, LmmVariant* vars, uint64_t* row_out,
                                  uint64_t* kmer_out, hipStream_t st) {
    if (!n_rows) return hipErrorInvalidValue;  // (total would stay unwritten)
    const uint32_t ndw = 2u * W_m, n_blocks = (n_rows + TB - 1) / TB;
    // the squeezed row must hold every accession the code row covers, and be read in 16-byte steps
    if (ndw % 4u || dm.bpsp % 4u || (uint64_t)ndw * 32u < (uint64_t)dm.bpsp * 4u || dm.n > 32u * ndw) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lmm_table_flag_kernel, dim3(n_blocks), dim3(TB), 0, st, sq, n_rows, ndw, dm.n, min_count, maf, n1flag, block_cnt);
    hipLaunchKernelGGL(lmm_table_scan_kernel, dim3(1), dim3(256), 0, st, block_cnt, n_blocks, block_off, total);
    hipLaunchKernelGGL(lmm_table_emit_kernel, dim3(n_blocks), dim3(TB), 0, st, rows, stride, sq, n_rows, ndw, dm.n, first_row, n1flag,
                       block_off, dm.bpsp, reinterpret_cast<uint32_t*>(codes), vars, row_out, kmer_out);
    return hipGetLastError();
}

}  // namespace kgwas
