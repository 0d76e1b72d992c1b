// score_mx.hip — the coarse filter of the sparse phase on gfx950's block-scaled matrix instruction
// (v_mfma_scale_f32_16x16x128_f8f6f4): FP4 table bits x FP6 / FP4 phenotype slices, both slices of a column accumulated
// into ONE float32 accumulator through the block scales. Same contract as the int8 filter of score_coarse.hip (which it
// replaces by default): for EVERY (k-mer, column) pair an approximation of yigi = sum_i g_i*y_i of
// calculate_kmer_score (src/kmers_multiple_databases.cpp:327-363) with a RIGOROUS bound, survivors as bits of the
// chunk's [column][row] bitmap, exact re-scoring of the survivors by rescore_kernel - results bit-identical to the
// exact scorers'.
//
//  * table bits as FP4 (E2M1). A nibble with only bit 0, 1 or 2 set is 0.5, 1.0 or 2.0, so `dword & (0x11111111 << j)`
//    IS an operand of eight table bits for j = 0, 1, 2 (bit 3, the FP4 sign, is shifted down first), and the operand's
//    block scale 2^0 / 2^-1 / 2^-2 (exact) makes every set bit 0.5: five lane-ops per 32 table bits (int8: 16), and one
//    K = 128 instruction does the work of two K = 64 int8 ones in the same 16 pipe cycles.
//  * phenotype slices as FP6 (E2M3) + FP4 (or FP6 + FP6), NOT uniformly quantised: with the integer grids
//        A6 = {0..15, 16..30 step 2, 32..60 step 4}   (E2M3 values x 8)      A4 = {0, 1, 2, 3, 4, 6, 8, 12}  (E2M1 x 2)
//    a column is  y_i - c ~ w * t_i,  t_i = 2^s * a6_i + a_i  (s = 3 with an FP4 second slice, 5 with an FP6 one),
//    c = sum / N. The second slice's block scale is 2^0 and the first one's 2^5, so that BOTH products land in the same
//    accumulator in the same unit: acc = kappa * sum_i g_i t_i, kappa = 1/4 (FP4 second slice) or 1/16 - every partial
//    sum a multiple of kappa far below 2^24 * kappa, i.e. exact in float32 in any order. One accumulator per (row tile,
//    16 columns) instead of one per slice, one fma per pair in the test instead of a combine + fma, and a residual of
//    at most half a unit near zero (where most of a phenotype's values are), a unit up to twice that, two units at the
//    extremes: 2.5x tighter than the uniform 961-level grid the same two operands would give.
//  * the operands (the B side: 1.25 bytes per sample and column with an FP4 second slice, 2560 bytes per MFMA step and
//    16 columns) sit in LDS for the whole block, as before; a wave owns 4 x 16 rows and CT column tiles' accumulators
//    (eight waves per block with 4..7 column tiles, twelve - three per SIMD, 168 registers - with up to three: the
//    2048-sample shapes, whose operands only fit three tiles at a time).
//  * samples beyond the last full 512-sample group are taken in QUARTER groups of 128 (one MFMA step each, the lane's own
//    dword shifted by 0..3; up to four of them) instead of a whole padded group: 1135 samples are 9 steps, not 12.
//
// Sample <-> k maps (tools/probe_mx6.hip checks the FP6 operand's element order and the exactness of E2M3 subnormals
// and of the two-scale accumulation on the device):
//   full group g, step j:   lane (m = lane & 15, kb = lane >> 4) holds bytes 64 g + 16 kb .. +15 of row m's bits as
//                           dwords q = 0..3; nibble e' of operand dword q = bit 4 e' + j of dword q, k = 32 kb + 8 q + e'
//                           <-> sample 512 g + 128 kb + 32 q + 4 e' + j
//   quarter step x:         the lane holds dword kb of the 16 bytes at 64 G + 16 x; operand dword q = (dword >> q) &
//                           0x11111111, k = 32 kb + 8 q + e' <-> sample 512 G + 128 x + 32 kb + 4 e' + q
//   slice operands:         lane (n = lane & 15, kb) holds column n's values for k = 32 kb + e, e = 0..31, in 6-bit
//                           (FP6: 6 dwords) or 4-bit (FP4: 4 dwords) fields, little-endian
//   accumulators:           lane (n, kb): rows 4 kb + i of the row tile, column n
//
// The block map, the column constants, the operand expansion and reads, the MFMA unit and the whole epilogue (row terms,
// test, survivor bits) are filter_common.h's; what is this kernel's own is the resident operands and the pass loop.
#include <stdlib.h>

#include <algorithm>

#include "filter_common.h"

// Timing experiments only (wrong results). Bits: 1 the tests are replaced by an XOR over all accumulators (every MFMA
// stays alive), 2 no operand expansion, 4 no LDS operand reads, 8 no row loads, 16 constant row terms, 32 no survivor
// emission (all but 8 act in filter_common.h).
#ifndef KGWAS_MX_ABLATE
#define KGWAS_MX_ABLATE 0
#endif

// KGWAS_MX_PERSIST=1 (shapes with ONE LDS group; the default since round 6): as many blocks as the chip holds at once (one per
// CU: the operands fill the LDS), each taking the 512-row passes b, b + grid, b + 2 grid, ... of the chunk - the operands are
// copied into the LDS once per block and LAUNCH instead of once per 4096 rows, every CU gets the same number of passes, and no
// CU waits for a last long block while others are done: 9.0 against 9.5 ms per 100 M rows x 1024 x 101 in alternating runs
// (tools/mx_ab.sh). 0: one block per 512 .. 4096 rows, as in rounds 3-5.
#ifndef KGWAS_MX_PERSIST
#define KGWAS_MX_PERSIST 1
#endif

namespace kgwas {

// S1F: format of the second slice (4 = FP4 E2M1, 2 = FP6 E2M3); NS = 1: first slice only.
template <int CT, int RT, int NS, int S1F, int TH>
__global__ void __launch_bounds__(TH) mx_kernel(MxArgs a, uint32_t rows_per_block, uint32_t n_rowblocks, uint32_t grid_lg) {
    extern __shared__ uint4 mlds[];  // [n_steps][CT][step bytes], colc[3][CT*16] (alpha, -, column index), per-wave row-term exchange
    typedef MxOperands<CT, NS, S1F> Ops;
    static_assert(RT == 4, "four row tiles per wave: 64 rows, one bitmap word per pass");
    constexpr uint32_t SB = Ops::SB;
    constexpr int SLOTS = CT * 16;
    constexpr int NU = Ops::NU;
    const FilterBlock fb = filter_block(a.n_lgroups, grid_lg);
    const bool persist = KGWAS_MX_PERSIST && !grid_lg;
    if (!persist && fb.rb >= n_rowblocks) return;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t kb = lane >> 4, m = lane & 15u;
    const uint32_t n_steps = 4u * a.n_full + a.n_quarter;
    const uint32_t group_bytes = n_steps * CT * SB;
    char* lds = reinterpret_cast<char*>(mlds);
    float* colc = reinterpret_cast<float*>(lds + group_bytes);
    const int* colp = reinterpret_cast<const int*>(colc + 2 * SLOTS);
    float* wscr = colc + 3 * SLOTS + wave * (RT * 48u);  // wave-private: RT*16 x N1, RT*16 x (sqrt(d), E)
    const uint32_t rows_per_pass = (TH / 64) * (RT * 16u);
    const uint64_t blk_row0 = (uint64_t)fb.rb * rows_per_block;
    const char* rows_base = reinterpret_cast<const char*>(a.src.base);
    const uint32_t avail_b = a.src.avail_dw * 4u;
    const int sc0 = (int)a.scale0;  // block scale of the first slice (E8M0 byte in every byte)
    uint32_t tested_local = 0;

    for (uint32_t lg = fb.lg0; lg < fb.lg1; lg++) {
        if (lg != fb.lg0) __syncthreads();
        {
            const uint4* src = reinterpret_cast<const uint4*>(a.Bq + (size_t)lg * group_bytes);
            for (uint32_t i = threadIdx.x; i < group_bytes / 16u; i += TH) mlds[i] = src[i];
            filter_col_consts(a, lg * SLOTS, SLOTS, colc);
        }
        __syncthreads();

        uint32_t ro[RT];  // byte offsets of this lane's rows
        const uint64_t wave_row0 = blk_row0 + wave * (RT * 16u);
        // This lane's 16 bytes of full group g of each of its RT rows: ONE 16-byte load per row tile (the four kb-lanes of a
        // row fetch the group's 64 bytes as one contiguous piece; rows are 8-byte aligned). A full group's bytes always
        // exist in the row: the host counts only whole 512-sample groups as full (n_full = S / 512).
        struct __attribute__((aligned(8))) U4 {
            uint32_t x, y, z, w;
        };
        auto load_group = [&](uint32_t (&pc)[RT][4], const uint32_t (&o)[RT], uint32_t g) {
            const uint32_t b0 = 64u * g + 16u * kb;
#pragma unroll
            for (int rt = 0; rt < RT; rt++) {
                uint32_t off = o[rt] + b0;
                asm volatile("" : "+v"(off));  // a 32-bit offset on the scalar base, made here: not a hoisted (and spilled) 64-bit pointer
                U4 v;
                if (KGWAS_MX_ABLATE & 8)
                    v = U4{off, lane * 2654435761u, lane, b0};
                else
                    v = *reinterpret_cast<const U4*>(rows_base + off);
                pc[rt][0] = v.x;
                pc[rt][1] = v.y;
                pc[rt][2] = v.z;
                pc[rt][3] = v.w;
            }
        };
        // The slice operands of the column tiles, read from LDS one unit ahead of their MFMAs (MxOperands): the next two
        // tiles of the step or the first two of the next step. No MFMA waits for a read issued just before it, and only
        // four tiles' operands (40 registers) are live at a time.
        Ops B;
        B.clear();
        auto step_addr = [&](const char* bstep) { return Ops::step_addr((uint32_t)(bstep - lds), lane); };
        uint32_t piece[RT][4];
        // the rows of this wave's pass ps: consecutive passes of a block, or - persistent blocks - every gridDim.x-th pass of the chunk
        const uint64_t pass_stride = persist ? (uint64_t)gridDim.x * rows_per_pass : rows_per_pass;
        const uint64_t wave_row00 = persist ? (uint64_t)blockIdx.x * rows_per_pass + wave * (RT * 16u) : wave_row0;
        const uint64_t n_pass_blk = persist ? ~0ull : (rows_per_block + rows_per_pass - 1) / rows_per_pass;
        filter_set_rows(a, ro, wave_row00, m);
        if (a.n_full && wave_row00 < a.n_rows) load_group(piece, ro, 0);
        MxStepAddr sadr = step_addr(lds);
        B.template read_unit<KGWAS_MX_ABLATE>(0, sadr, lds, lane);  // step 0 of the first pass; every pass's last step fetches it for the next
        for (uint64_t ps = 0; ps < n_pass_blk; ps++) {
            const uint64_t rbase = wave_row00 + ps * pass_stride;
            if (rbase >= a.n_rows) break;  // wave-uniform
            uint32_t ro_next[RT];
            filter_set_rows(a, ro_next, rbase + pass_stride, m);
            mxv4f acc[RT][CT];
#pragma unroll
            for (int rt = 0; rt < RT; rt++)
#pragma unroll
                for (int t = 0; t < CT; t++) acc[rt][t] = (mxv4f){0.0f, 0.0f, 0.0f, 0.0f};

            // step = [reads of unit 1 | MFMAs of unit 0 | reads of unit 2 | MFMAs of unit 1 | ... | reads of the next step's unit 0 | MFMAs of the last unit]
            auto run_step = [&](const mxv8i (&A)[RT], const char* bs_next, int sa) {
                const MxStepAddr nadr = step_addr(bs_next);
                if (NU == 1) {
                    // one unit per step: the next step's operands cannot land in the registers this step still multiplies
                    // with - they go to a second set (at most two tiles) and move over afterwards
                    Ops next;
                    next.clear();
                    next.template read_unit<KGWAS_MX_ABLATE>(0, nadr, lds, lane);
                    __builtin_amdgcn_sched_barrier(0);
                    B.mfma_unit(0, A, acc, sa, sc0);
                    __builtin_amdgcn_sched_barrier(0);
                    B.take(next);
                } else {
#pragma unroll
                    for (int u = 0; u < NU; u++) {
                        if (u + 1 < NU)
                            B.template read_unit<KGWAS_MX_ABLATE>(u + 1, sadr, lds, lane);
                        else
                            B.template read_unit<KGWAS_MX_ABLATE>(0, nadr, lds, lane);
                        __builtin_amdgcn_sched_barrier(0);
                        B.mfma_unit(u, A, acc, sa, sc0);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                sadr = nadr;
            };

            // full 512-sample groups: four steps over this lane's 16 bytes of each of its RT rows. The pieces of the NEXT
            // group - the next one of this pass or, from the last one, group 0 of the wave's next rows - are requested as
            // soon as step 3 has expanded the current ones: a whole step (and, across passes, the epilogue) ahead.
            __builtin_amdgcn_s_setprio(0);
            for (uint32_t g = 0; g < a.n_full; g++) {
                const char* bg = lds + (size_t)g * 4u * CT * SB;
                const bool last_g = g + 1u == a.n_full;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    mxv8i A[RT];
                    mx_expand_step<KGWAS_MX_ABLATE>(A, piece, j);
                    const char* bs = bg + j * CT * SB;
                    const char* bs_next = bs + CT * SB;
                    if (j == 3) {
                        // (selects, not branches: a branch here splits the loop body, the MFMAs of steps 0-2 sink below it
                        // and their operands - three steps' worth - are all live across it)
                        __builtin_amdgcn_sched_barrier(0);
                        uint32_t on[RT];
#pragma unroll
                        for (int rt = 0; rt < RT; rt++) on[rt] = last_g ? ro_next[rt] : ro[rt];
                        load_group(piece, on, last_g ? 0u : g + 1u);
                        if (last_g && a.n_quarter == 0) bs_next = lds;  // the pass's last step: step 0 of the next pass
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    run_step(A, bs_next, mx_step_scale(j));
                }
            }
            // quarter groups: 128 samples per step, the lane's own dword shifted by 0..3
            for (uint32_t x = 0; x < a.n_quarter; x++) {
                uint32_t b0 = 64u * a.n_full + 16u * x + 4u * kb;
                b0 = b0 + 4u <= avail_b ? b0 : avail_b - 4u;
                mxv8i A[RT];
#pragma unroll
                for (int rt = 0; rt < RT; rt++)
                    A[rt] = mx_expand_quarter((KGWAS_MX_ABLATE & 8) ? ro[rt] + b0 : *reinterpret_cast<const uint32_t*>(rows_base + (ro[rt] + b0)));
                const char* bs = lds + (size_t)(4u * a.n_full + x) * CT * SB;
                run_step(A, x + 1u == a.n_quarter ? lds : bs + CT * SB, mx_step_scale(0));
            }

            // The pass's epilogue at raised priority, the main loop at the default one: a wave in its epilogue issues vector
            // instructions only, and the sooner it is through them the sooner the SIMD has two MFMA streams again
            // (-1.8 % in alternating runs, tools/mx_ab.sh; raising the MAIN loop's priority instead: +-0).
            __builtin_amdgcn_s_setprio(3);
            const uint32_t tested = mx_epilogue<KGWAS_MX_ABLATE>(a, acc, wscr, colc, colp, rbase, lane);
            if (lg == 0) tested_local += tested;
#pragma unroll
            for (int rt = 0; rt < RT; rt++) ro[rt] = ro_next[rt];
        }
    }
    filter_add_tested(a.tested, tested_local, lane);
}

// slice operands of one LDS group + the group's per-column constants (3 x up to 112 words) + the waves' row-term
// exchange areas (768 B each; twelve waves where CT <= 3)
size_t mx_lds_bytes(uint32_t n_steps, uint32_t CT, uint32_t n_slices, uint32_t s1_fp6) {
    return (size_t)n_steps * CT * mx_step_bytes(n_slices, s1_fp6) + 3u * 112u * 4u + 12u * 768u;
}

template <int CT, int NS, int S1F, int TH = 512>
static hipError_t launch_mx_t(const MxArgs& a, uint32_t rows_per_block, size_t lds, hipStream_t st) {
    const uint32_t rpp = (TH / 64) * 64u;
    const bool grid_lg = a.n_lgroups > 1;
    FilterGrid g;
    const hipError_t e = filter_grid((const void*)mx_kernel<CT, 4, NS, S1F, TH>, a, rpp, rows_per_block, grid_lg, lds, g);
    if (e != hipSuccess) return e;
    if (KGWAS_MX_PERSIST && !grid_lg) {
        static int n_cu = 0;
        if (!n_cu) {
            int dev = 0;
            hipDeviceProp_t pr;
            n_cu = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0) ? pr.multiProcessorCount : 256;
        }
        const uint64_t n_pass = (a.n_rows + rpp - 1) / rpp;
        g.grid = (uint32_t)std::min<uint64_t>(n_pass, (uint64_t)n_cu);
    }
    launch_last(mx_kernel<CT, 4, NS, S1F, TH>, dim3(g.grid), dim3(TH), lds, st, a, g.rows_per_block, g.n_rowblocks, grid_lg ? 1u : 0u);
    return hipGetLastError();
}

template <int NS, int S1F>
static hipError_t launch_mx_ct(const MxArgs& a, uint32_t CT, uint32_t rows_per_block, size_t lds, hipStream_t st) {
    switch (CT) {
        // up to three column tiles (48 accumulator registers with four row tiles): 168 registers, three waves per SIMD
        case 1: return launch_mx_t<1, NS, S1F, 768>(a, rows_per_block, lds, st);
        case 2: return launch_mx_t<2, NS, S1F, 768>(a, rows_per_block, lds, st);
        case 3: return launch_mx_t<3, NS, S1F, 768>(a, rows_per_block, lds, st);
        case 4: return launch_mx_t<4, NS, S1F>(a, rows_per_block, lds, st);
        case 5: return launch_mx_t<5, NS, S1F>(a, rows_per_block, lds, st);
        case 6: return launch_mx_t<6, NS, S1F>(a, rows_per_block, lds, st);
        case 7: return launch_mx_t<7, NS, S1F>(a, rows_per_block, lds, st);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_mx(const MxArgs& a, uint32_t CT, uint32_t rows_per_block, hipStream_t st) {
    if (a.n_rows == 0) return hipSuccess;
    const size_t lds = mx_lds_bytes(4u * a.n_full + a.n_quarter, CT, a.n_slices, a.s1_fp6);
#ifdef KGWAS_MX_BENCH_ONLY  // experiments: only the shape of the 1024 x 101 bench (fast compiles)
    if (a.n_slices == 2 && !a.s1_fp6 && CT == 7) return launch_mx_t<7, 2, 4>(a, rows_per_block, lds, st);
    return hipErrorInvalidValue;
#else
    if (a.n_slices == 1) return launch_mx_ct<1, 4>(a, CT, rows_per_block, lds, st);
    if (a.n_slices == 2 && !a.s1_fp6) return launch_mx_ct<2, 4>(a, CT, rows_per_block, lds, st);
    if (a.n_slices == 2 && a.s1_fp6) return launch_mx_ct<2, 2>(a, CT, rows_per_block, lds, st);
    return hipErrorInvalidValue;
#endif
}

}  // namespace kgwas
