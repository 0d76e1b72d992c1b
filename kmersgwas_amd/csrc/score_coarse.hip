// score_coarse.hip — coarse int8-MFMA filter (XDL matrix pipe); its survivors are listed and re-scored exactly in survivors.hip.
//
// The exact scorers (score_mfma.hip / score_valu.hip) reproduce calculate_kmer_score
// (src/kmers_multiple_databases.cpp:327-363) bit for bit, but the exact float32 order is capped by the
// vector-rate f32 MFMA (157 TFLOP/s). Once the heaps are full only ~1e-4 of the (k-mer, column) pairs
// can beat a column's threshold, so the sparse phase is split in two:
//
//  1. coarse_kernel — for EVERY pair, an integer approximation of yigi = sum_i g_i*y_i on
//     v_mfma_i32_16x16x64_i8 (XDL pipe, ~25x the f32 rate, runs beside the VALU):
//        y_i ~ s0*q0_i + s1*q1_i,  q0, q1 in [-127, 127]  (two int8 slices per phenotype column)
//        yc  = s0*D0 + s1*D1,      D0, D1 = exact int32 dot products of the bit row with q0, q1
//     and a RIGOROUS bound E_p >= |yigi_ref - yc|, where yigi_ref is the value the reference's float32
//     chain produces:   |yigi_ref - sum g_i y_i| <= gamma_{L/4+3} * sum|y_i|   (float32 summation)
//                       |sum g_i y_i  - yc|      <= sum_i |y_i - s0 q0_i - s1 q1_i|   (quantisation)
//     With r = N*yigi - N1*sum (same `sum` as the reference), |r_ref| <= |r_c| + N*E_p, so a pair can
//     only satisfy score_ref > thr if (|r_c| + N*E_p)^2 >= thr*d. Everything else is provably below the
//     threshold and is dropped; the rest ("survivors", true candidates plus a ~1e-6 fringe) is listed.
//  2. rescore_kernel (survivors.hip) — the survivors are re-scored in the exact reference order on the VALU (one lane per
//     survivor, y wave-uniform) and go through the same finish_pair as the exact scorers: exact test
//     against thr, threshold histogram, candidate record. Results are therefore bit-identical to the
//     exact path; the coarse pass only decides what is worth looking at.
//
// Coarse mode does not care about accumulation order, so the k-index of the MFMA is mapped to samples in
// the way that needs no data exchange and the fewest lane-ops: in a 512-sample group g, lane (m = lane&15,
// kg = lane>>4) loads ITS OWN 16 bytes (dwords q = 0..3) of row m (samples 512g+128kg .. +127), and MFMA step
// j = 0..7 takes bit 8e + j of dword q as k-element 4q + e of that lane, i.e.
//        k = 16*kg + 4q + e   <->   sample 512g + 128kg + 32q + 8e + j.
// The four kg-lanes of a row thus fetch 64 contiguous bytes per instruction, every byte is used by the lane that
// loaded it, and an operand dword is (dword >> j) & 0x01010101: two lane-ops per 4 operand bytes (the earlier
// nibble * 0x00204081 & 0x01010101 needed three, and the vector instructions beside the MFMAs are what bounds this
// kernel); each expanded operand feeds T column tiles, each B operand (ds_read_b128) four row tiles.
#include <algorithm>
#include <type_traits>

#include "filter_common.h"
#include "score_common.h"

#ifndef KGWAS_COARSE_PHASES
#define KGWAS_COARSE_PHASES 1  // pin the per-step order: LDS reads, operand expansion, MFMAs
#endif
// Timing experiments only (wrong results; tools/coarse_variants.sh builds the variants). Bits: 1 the tests are replaced by
// an XOR over all accumulators (every MFMA stays alive), 2 no operand expansion, 4 no LDS operand reads, 8 no row loads,
// 16 constant row terms, 32 a token side effect instead of the survivor emission (1, 16 and 32 act in filter_common.h).
#ifndef KGWAS_COARSE_ABLATE
#define KGWAS_COARSE_ABLATE 0
#endif

namespace kgwas {

typedef int i32x4 __attribute__((ext_vector_type(4)));

#ifdef KGWAS_COARSE_TIMELINE  // diagnostics build (tools/coarse_timeline.py): cycle stamps of waves 0 and 4 of one block
__device__ unsigned long long g_coarse_tl[2 * 16 * 64];
#define TL_STAMP(idx)                                                                       \
    do {                                                                                    \
        if (tl_on) {                                                                        \
            const unsigned long long t_ = clock64();                                        \
            if (lane == 0) g_coarse_tl[tl_base + (idx)] = t_;                               \
        }                                                                                   \
    } while (0)
#else
#define TL_STAMP(idx) do { } while (0)
#endif

// A operand of step j from the lane's four row dwords: byte e of operand dword q = bit 8e + j of row dword q,
// i.e. k-element 4q + e <-> sample 32q + 8e + j of the lane's 128 (two lane-ops per dword, one for j = 0).
__device__ __forceinline__ i32x4 expand_step(const uint32_t (&w)[4], int j) {
    i32x4 r;
#pragma unroll
    for (int q = 0; q < 4; q++) r[q] = (int)((w[q] >> j) & 0x01010101u);
    return r;
}

// T  = operand tiles (16 columns of one int8 slice each) per LDS group,
// NS = int8 slices per column (1: tile t of a group = column tile; 2: tiles 2g, 2g+1 = the two slices of column group g).
//
// The conservative test. The host centres the quantisation at c = sum/N (sum = the reference's float32 sum), so
//   r_c = N*yc - N1*sum = N*u*Dc            Dc = D0 (one slice) or 254*D0 + D1 (two slices, s0 = 254*s1), u = s0 or s1,
// an exact integer times a column constant. A pair can only have score_ref > thr if
//   |Dc| >= alpha_p * sqrt(d(N1)) - E_p(N1)/u_p,    alpha_p = sqrt(thr_p)/(N*u_p),  E_p(N1) = Eg_p + min(Rall_p, N1*rmax_p).
// The error terms are taken in units of Dc (Eg_p/u_p, ... : the quantisation residual is at most half a unit per
// sample whatever the column's scale) and as their maxima over all columns, so E/u is a per-ROW term and the test is
//   margin = |Dc| - alpha_p * sqrt(d)   (float(Dc), then one float32 fma),    survivor iff margin + E >= 0
// evaluated from constants the host rounded in the safe direction (alpha down by 2^-19 relative, sqrt(d) down by
// 2^-20, the error terms up by 1e-6): the slack 2.8e-6 * alpha * sqrt(d) dominates the roundings of float(Dc) and of
// the fma (6e-8 relative each), and the final addition cannot change the sign of an exact non-negative sum - so no
// possible candidate is dropped. The maximum of the margins of a lane's pairs of one row is tested once.
//
// N1 comes out of the matrix pipe as well: the last operand column of every LDS group holds 1 for each phenotyped
// sample (0 elsewhere), so its dot product IS the masked popcount - no masks, no popcounts, no mask loads in the
// main loop, and bits of unphenotyped samples or row padding meet zeros in every operand column.
template <int T, int NS, int TH = 512>
__global__ void __launch_bounds__(TH) coarse_kernel(CoarseArgs a, uint32_t rows_per_block, uint32_t n_rowblocks, uint32_t grid_lg) {
    extern __shared__ i32x4 blds[];  // [n_kgroups][8][T][64] x 16 bytes, colc[3][PG*16] (alpha, 1/u, column index), survivor buffer
    constexpr int PG = T / NS;       // column groups (of 16) per LDS group
    constexpr int RT = 4;
    constexpr int SLOTS = PG * 16;
    // Several LDS groups: either this block walks them one after the other over its rows (grid_lg = 0: every pass over
    // the rows re-reads them, 1 MB per block and pass, far more than the L2 keeps across a pass) or every (row block,
    // group) pair is a block of its own (grid_lg = 1, see filter_block).
    const FilterBlock fb = filter_block(a.n_lgroups, grid_lg);
    if (fb.rb >= n_rowblocks) return;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t kg = lane >> 4, m = lane & 15u;
    const uint32_t n_kgroups = a.n_kgroups;
    const uint32_t group_vec = n_kgroups * 8u * T * 64u;  // i32x4 elements per LDS group
    float* colc = reinterpret_cast<float*>(blds + group_vec);
    const int* colp = reinterpret_cast<const int*>(colc + 2 * SLOTS);
    // Survivors leave as a bitmap: one 64-bit word per (phenotype column, 64 rows of a wave pass), bit = row of the pass
    // (the chunk's bitmap is zeroed beforehand; only non-zero words are stored). Row order is then a property of the
    // bitmap and the ordered per-column key lists come out of a popcount scan (launch_bitmap_keys) - the first version
    // appended keys to one global list (per-block LDS buffering, one device atomic per block) that a radix sort then
    // had to put in (column, row) order: 4.6 ms of a 22 ms pass at 101 columns.
    float* wscr = colc + 3 * SLOTS + wave * 192u;  // wave-private: 64 x N1, 64 x (sqrt(d), E)
    const uint32_t rows_per_pass = (blockDim.x >> 6) * (RT * 16u);
    const uint64_t blk_row0 = (uint64_t)fb.rb * rows_per_block;
    const char* rows_base = reinterpret_cast<const char*>(a.src.base);
    const uint32_t avail_b = a.src.avail_dw * 4u;
    uint32_t tested_local = 0;

    for (uint32_t lg = fb.lg0; lg < fb.lg1; lg++) {
        if (lg != fb.lg0) __syncthreads();
        {
            const i32x4* src = reinterpret_cast<const i32x4*>(a.Bq) + (size_t)lg * group_vec;
            for (uint32_t i = threadIdx.x; i < group_vec; i += blockDim.x) blds[i] = src[i];
            filter_col_consts(a, lg * SLOTS, SLOTS, colc);
        }
        __syncthreads();

        // piece[rt][q] = dword q of this lane's 16 bytes of row tile rt for the current (pass, sample group) unit
        // (bytes 64g + 16kg .. +15 of the row's bits; beyond the row's data the load is clamped onto its last 8 bytes:
        // whatever bits arrive there meet zero operands, sample slots >= S are zero in every column). The pieces of
        // the NEXT unit - the next sample group, or group 0 of the wave's next 64 rows - are fetched into the same
        // registers as soon as the current unit has expanded them: 4-5 steps (2000+ cycles) ahead of their use, and
        // across the epilogue.
        uint32_t piece[RT][4];
        uint32_t ro[RT];  // byte offsets of the rows to fetch next
        auto load_half = [&](uint32_t g, int h) {
            uint32_t b0 = 64u * g + 8u * h + 16u * kg;
            b0 = b0 + 8u <= avail_b ? b0 : avail_b - 8u;  // unconditional load (a branch here splits the scheduling region)
#pragma unroll
            for (int rt = 0; rt < RT; rt++) {
                uint2 v;
                if (KGWAS_COARSE_ABLATE & 8)
                    v = make_uint2(ro[rt] + b0, lane * 2654435761u);
                else
                    v = *reinterpret_cast<const uint2*>(rows_base + (ro[rt] + b0));
                piece[rt][2 * h] = v.x;
                piece[rt][2 * h + 1] = v.y;
            }
        };
        const uint64_t wave_row0 = blk_row0 + wave * (RT * 16u);

        for (uint32_t ps = 0; ps * rows_per_pass < rows_per_block; ps++) {
            const uint64_t rbase = wave_row0 + (uint64_t)ps * rows_per_pass;
            if (rbase >= a.n_rows) break;  // wave-uniform
            i32x4 acc[RT][T];
#ifdef KGWAS_COARSE_TIMELINE
            const bool tl_on = blockIdx.x == KGWAS_COARSE_TIMELINE && (wave & 3u) == 0u && ps < 16u && lg == 0;
            const uint32_t tl_base = ((wave >> 2) * 16u + ps) * 64u;
#endif
            TL_STAMP(0);

            // One step = one bit position of every byte of the lane's 16 row bytes = 64 MFMA k-elements, T x RT MFMAs.
            // Per step the B operands are requested from LDS first, the A operands are expanded while those reads are in
            // flight, then the MFMAs issue back to back. What was measured on gfx950 about this loop (tools/issue_model.hip,
            // tools/coarse_variants.sh): beside each 16-cycle MFMA a SIMD issues two other vector instructions for free
            // and pays ~4 cycles for every further one; a long run of vector instructions in one wave (the epilogue) is
            // NOT hidden behind its partner's MFMAs, with or without s_setprio or a start offset between the two waves;
            // software-pipelined variants (A operands double-buffered and interleaved with the MFMAs, B operands reloaded
            // in place behind their tile, next row dwords prefetched) all measured 5-25 % slower than this plain order.
            auto run_group = [&](uint32_t g, auto first_tag) {
                constexpr bool FIRST = decltype(first_tag)::value;  // first sample group: the accumulators start at zero
                const i32x4* bg = blds + (size_t)g * 8u * T * 64u + lane;
                if (FIRST) filter_set_rows(a, ro, rbase, m);
                load_half(g, 0);
                load_half(g, 1);
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    if (g < 2) TL_STAMP(1 + (g * 8 + j) * 3);  // step start
                    i32x4 B[T];
#pragma unroll
                    for (int t = 0; t < T; t++) B[t] = (KGWAS_COARSE_ABLATE & 4) ? (i32x4){(int)(lane & 1u), 0, 1, 0} : bg[(j * T + t) * 64];
#if KGWAS_COARSE_PHASES
                    __builtin_amdgcn_sched_barrier(0);
#endif
                    i32x4 A[RT];
#pragma unroll
                    for (int rt = 0; rt < RT; rt++) {
                        if (KGWAS_COARSE_ABLATE & 2)
                            A[rt] = (i32x4){(int)(piece[rt][0] & 0x01010101u), (int)(piece[rt][1] & 0x01010101u),
                                            (int)(piece[rt][2] & 0x01010101u), (int)(piece[rt][3] & 0x01010101u)};
                        else
                            A[rt] = expand_step(piece[rt], j);
                    }
#if KGWAS_COARSE_PHASES
                    __builtin_amdgcn_sched_barrier(0);
#endif
#ifdef KGWAS_COARSE_TIMELINE
                    __builtin_amdgcn_s_waitcnt(0);  // operands arrived (vmcnt 0, lgkmcnt 0)
                    if (g < 2) TL_STAMP(2 + (g * 8 + j) * 3);  // operands ready, MFMAs start
                    __builtin_amdgcn_sched_barrier(0);
#endif
#pragma unroll
                    for (int t = 0; t < T; t++) {
#pragma unroll
                        for (int rt = 0; rt < RT; rt++) {
                            if (FIRST && j == 0)
                                acc[rt][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[rt], B[t], (i32x4){0, 0, 0, 0}, 0, 0, 0);
                            else
                                acc[rt][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[rt], B[t], acc[rt][t], 0, 0, 0);
                        }
                    }
#if KGWAS_COARSE_PHASES
                    __builtin_amdgcn_sched_barrier(0);
#endif
                    if (g < 2) TL_STAMP(3 + (g * 8 + j) * 3);  // MFMAs issued
                }
            };
            run_group(0u, std::true_type{});
            for (uint32_t g = 1; g < n_kgroups; g++) run_group(g, std::false_type{});

            TL_STAMP(50);  // main loop done
            // Per-row terms (filter_row_terms): N1 from the ones column, sqrt(d) rounded down, E(N1) in units of Dc rounded
            // up, one row per lane through the wave-private exchange area (the same terms computed 16 times per lane were a
            // quarter of the kernel's vector work).
            float sqd[RT * 4], er[RT * 4];
            {
                const uint32_t tested = filter_row_terms<int, KGWAS_COARSE_ABLATE>(a, acc, wscr, rbase, lane, sqd, er);
                if (lg == 0) tested_local += tested;
                __builtin_amdgcn_wave_barrier();
            }
            TL_STAMP(51);  // row terms exchanged
            // The test, ~2.5 lane-ops per pair: margin = |Dc| - alpha_p * sqrt(d) (float(Dc), one fma with |.| and
            // negation as operand modifiers), a running maximum per row slot (max3), and ONE compare per row slot:
            // the slot has a survivor iff max margin + E >= 0. Which pairs passed is only worked out for row slots
            // with a hit (steady state: ~2 of the 1024 (lane, slot) units of a pass).
            auto pair_margin = [&](int i, int g, float al) {
                int dc = acc[i >> 2][NS * g][i & 3];
                if (NS == 2) dc = __mul24(dc, 254) + acc[i >> 2][NS * g + NS - 1][i & 3];  // |D0| <= 127 * S < 2^23
                return fmaf(-al, sqd[i], fabsf((float)dc));  // NaN (frozen column) never wins a maximum
            };
            float alc[PG];
#pragma unroll
            for (int g = 0; g < PG; g++) alc[g] = colc[g * 16 + m];
            uint64_t hit[RT * 4];
            if (!(KGWAS_COARSE_ABLATE & 1)) {
                float mx[RT * 4];
#pragma unroll
                for (int i = 0; i < RT * 4; i++) mx[i] = -__builtin_huge_valf();
#pragma unroll
                for (int g = 0; g < PG; g++)
#pragma unroll
                    for (int i = 0; i < RT * 4; i++) mx[i] = fmaxf(mx[i], pair_margin(i, g, alc[g]));
#pragma unroll
                for (int i = 0; i < RT * 4; i++) hit[i] = __ballot(mx[i] + er[i] >= 0.0f);
            } else {
                filter_xor_hits(acc, hit);
            }
            TL_STAMP(52);  // tests done
            // which pairs of the hit row slots passed, and their bits into the bitmap
            filter_emit<KGWAS_COARSE_ABLATE, PG, RT>(a, hit, alc, er, colp, rbase, lane, pair_margin);
            TL_STAMP(53);  // hits resolved, survivors emitted
        }
    }
    filter_add_tested(a.tested, tested_local, lane);  // every lane counted one row per pass
}

// B operands of one LDS group + the group's per-column constants (3 x up to 128 words) + the eight waves' row-term
// exchange areas
size_t coarse_lds_bytes(uint32_t n_kgroups, uint32_t T) { return (size_t)n_kgroups * 8u * T * 1024u + 1536u + 8u * 768u; }

template <int T, int NS, int TH = 512>
static hipError_t launch_coarse_t(const CoarseArgs& a, uint32_t rows_per_block, size_t lds, hipStream_t st) {
    lds += (size_t)(TH / 64 - 8) * 768u;  // per-wave scratch of the waves beyond eight
    static const int grid_env = (int)exp_int("KGWAS_COARSE_GRIDLG", -1);  // experiments
    const uint32_t grid_lg = (grid_env >= 0 ? grid_env != 0 : true) && a.n_lgroups > 1 ? 1u : 0u;
    FilterGrid g;
    const hipError_t e = filter_grid((const void*)coarse_kernel<T, NS, TH>, a, (TH / 64) * 64u, rows_per_block, grid_lg != 0u, lds, g);
    if (e != hipSuccess) return e;
    launch_last(coarse_kernel<T, NS, TH>, dim3(g.grid), dim3(TH), lds, st, a, g.rows_per_block, g.n_rowblocks, grid_lg);
    return hipGetLastError();
}

hipError_t launch_coarse(const CoarseArgs& a, uint32_t T, uint32_t rows_per_block, hipStream_t st) {
    if (a.n_rows == 0) return hipSuccess;
    const size_t lds = coarse_lds_bytes(a.n_kgroups, T);
#ifdef KGWAS_COARSE_BENCH_ONLY  // experiments: only the two shapes of the 1024 x 101 bench (fast compiles)
    if (a.n_slices == 1 && T == 7) return launch_coarse_t<7, 1>(a, rows_per_block, lds, st);
    if (a.n_slices == 2 && T == 8) return launch_coarse_t<8, 2>(a, rows_per_block, lds, st);
    return hipErrorInvalidValue;
#else
    // Few tiles per LDS group leave registers for a third wave per SIMD (T <= 4: <= 168 VGPRs at 768 threads)
    static const int th_env = (int)exp_int("KGWAS_COARSE_TH", 768);  // experiments (512: eight waves as for T > 4)
    if (th_env == 768 && a.n_slices == 1 && T <= 4 && lds + 4u * 768u <= 160u * 1024u) {
        switch (T) {
            case 1: return launch_coarse_t<1, 1, 768>(a, rows_per_block, lds, st);
            case 2: return launch_coarse_t<2, 1, 768>(a, rows_per_block, lds, st);
            case 3: return launch_coarse_t<3, 1, 768>(a, rows_per_block, lds, st);
            case 4: return launch_coarse_t<4, 1, 768>(a, rows_per_block, lds, st);
        }
    }
    if (a.n_slices == 1) {
        switch (T) {
            case 1: return launch_coarse_t<1, 1>(a, rows_per_block, lds, st);
            case 2: return launch_coarse_t<2, 1>(a, rows_per_block, lds, st);
            case 3: return launch_coarse_t<3, 1>(a, rows_per_block, lds, st);
            case 4: return launch_coarse_t<4, 1>(a, rows_per_block, lds, st);
            case 5: return launch_coarse_t<5, 1>(a, rows_per_block, lds, st);
            case 6: return launch_coarse_t<6, 1>(a, rows_per_block, lds, st);
            case 7: return launch_coarse_t<7, 1>(a, rows_per_block, lds, st);
            case 8: return launch_coarse_t<8, 1>(a, rows_per_block, lds, st);
        }
    } else if (a.n_slices == 2) {
        switch (T) {
            case 2: return launch_coarse_t<2, 2>(a, rows_per_block, lds, st);
            case 4: return launch_coarse_t<4, 2>(a, rows_per_block, lds, st);
            case 6: return launch_coarse_t<6, 2>(a, rows_per_block, lds, st);
            case 8: return launch_coarse_t<8, 2>(a, rows_per_block, lds, st);
        }
    }
    return hipErrorInvalidValue;
#endif
}

#ifdef KGWAS_COARSE_TIMELINE
extern "C" int kgwas_debug_coarse_timeline(unsigned long long* out, unsigned long long n) {
    if (n > 2 * 16 * 64) n = 2 * 16 * 64;
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_coarse_tl), n * sizeof(unsigned long long), 0, hipMemcpyDeviceToHost);
}
#endif

}  // namespace kgwas
