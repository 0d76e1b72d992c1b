// filter_common.h — the pieces the three matrix filters of the sparse phase share: coarse_kernel (int8, score_coarse.hip),
// mx_kernel (block-scaled, operands resident in LDS, score_mx.hip) and mxs_kernel (block-scaled, operands streamed,
// score_mxs.hip). Each piece exists here once: the block map, the per-slot column constants, the row offsets, the per-row
// terms with their rounding constants, the survivor test's rare path and the bitmap store that launch_bitmap_keys undoes,
// the tested-row count, and - for the two block-scaled kernels - the operand expansion, the LDS operand reads and the
// MFMA unit. Everything is __forceinline__ and works on the caller's registers: the kernels stay one function each.
//
// ABLATE (timing experiments, wrong results) is the including kernel's KGWAS_*_ABLATE word; the bits that fall in here:
// 1 the tests are replaced by an XOR over all accumulators (every MFMA stays alive), 2 no operand expansion, 4 no LDS
// operand reads, 16 constant row terms, 32 a token side effect instead of the survivor emission.
#pragma once
#include "block_prims.h"  // filter_add_tested: the tested-row count, shared with the narrow filter
#include "kernels.h"

namespace kgwas {

// ---- block -> (row block, LDS / operand groups) ---------------------------------------------------------------------
// grid_lg = 0: the block walks the groups [0, n_lgroups) one after the other over its rows. grid_lg = 1: every (row
// block, group) pair is a block of its own. Blocks go to XCD (id % 8) in id order, so the groups of a row block get
// consecutive ids on ONE XCD: they start within a few per cent of a block's run time of each other and stream through
// the same rows together - one of them fetches a row from HBM, the others find it in the L2.
struct FilterBlock {
    uint32_t rb, lg0, lg1;
};
__device__ __forceinline__ FilterBlock filter_block(uint32_t n_lgroups, bool grid_lg) {
    FilterBlock b = {blockIdx.x, 0u, n_lgroups};
    if (grid_lg) {
        const uint32_t idx = blockIdx.x >> 3;
        b.rb = (idx / n_lgroups) * 8u + (blockIdx.x & 7u);
        b.lg0 = idx % n_lgroups;
        b.lg1 = b.lg0 + 1u;
    }
    return b;
}

// Per-slot constants of one group into LDS: colc[0 .. n_slots) alpha, [n_slots .. 2 n_slots) 1/u, [2 n_slots .. ) the
// phenotype column (int). The first n_slots threads of the block write; the caller's barrier publishes them.
template <class Args>
__device__ __forceinline__ void filter_col_consts(const Args& a, uint32_t first_slot, int n_slots, float* colc) {
    if (threadIdx.x < (uint32_t)n_slots) {
        const CoarseCol cc = a.cols[first_slot + threadIdx.x];
        float al = __builtin_huge_valf();  // padding / N1 column: nothing survives
        if (cc.pheno >= 0) al = (float)(sqrt(a.thr[cc.pheno]) * cc.kalpha);  // NaN threshold (frozen column) -> NaN -> nothing survives
        colc[threadIdx.x] = al;
        colc[n_slots + threadIdx.x] = cc.iu;
        reinterpret_cast<int*>(colc + 2 * n_slots)[threadIdx.x] = cc.pheno;
    }
}

// 32-bit byte offsets of this lane's rows rb0 + 16 rt + (lane & 15), clamped onto the chunk's last row (the launcher
// guarantees that the chunk spans < 4 GiB).
template <int RT, class Args>
__device__ __forceinline__ void filter_set_rows(const Args& a, uint32_t (&o)[RT], uint64_t rb0, uint32_t m) {
#pragma unroll
    for (int rt = 0; rt < RT; rt++) {
        uint64_t r = rb0 + rt * 16u + m;
        if (r >= a.n_rows) r = a.n_rows - 1;
        o[rt] = ((uint32_t)r * (uint32_t)a.src.stride_dw + a.src.off_dw) * 4u;
    }
}

// ---- per-row terms ---------------------------------------------------------------------------------------------------
// Lane (kb = lane >> 4, m = lane & 15) holds accumulator registers of the rows 4 kb + jj of its RT row tiles ("row slot"
// i = 4 rt + jj); the 16 m-lanes of a kb share them. N1 comes out of the matrix pipe: the ones column is slot 15 of the
// last operand tile, so lane (kb, 15) holds it for all its slots. Through the wave-private exchange area wscr (RT*16 x N1,
// then RT*16 x (sqrt(d), E)) every lane computes the terms of ONE row - entry e = lane = (kb' = e / (4 RT), slot i =
// e % (4 RT)): row 16 (i / 4) + 4 kb' + i % 4 - and reads back the ones of its own slots:
//   sqd[i]  sqrt(d), d = N1 (N - N1), rounded DOWN: d < 2^24 is exact, the sqrt is good to 1 ulp, (1 - 2^-20) covers it;
//           +inf for a row that does not exist or fails the MAC filter (nothing survives)
//   er[i]   the row's error term E(N1) = eg_max + min(rall_max, N1 * rmax_max), rounded UP
// E: the accumulators' element type (int or float). Returns 1 if this lane's row exists and passes the MAC filter.
// The next pass rewrites the exchange area: the caller puts a wave barrier between this call and the next.
template <class E, int ABLATE, int RT, int NT, class V4, class Args>
__device__ __forceinline__ uint32_t filter_row_terms(const Args& a, const V4 (&acc)[RT][NT], float* wscr, uint64_t rbase, uint32_t lane,
                                                     float (&sqd)[RT * 4], float (&er)[RT * 4]) {
    constexpr uint32_t NSL = RT * 4;
    const uint32_t kb = lane >> 4, m = lane & 15u;
    E* n1s = reinterpret_cast<E*>(wscr);
    float2* trm = reinterpret_cast<float2*>(wscr + RT * 16);
    if (m == 15u) {
#pragma unroll
        for (int rt = 0; rt < RT; rt++) *reinterpret_cast<V4*>(n1s + kb * NSL + rt * 4) = acc[rt][NT - 1];
    }
    __builtin_amdgcn_wave_barrier();
    bool ok = false;
    if (RT == 4 || lane < RT * 16u) {
        const uint64_t left = rbase < a.n_rows ? a.n_rows - rbase : 0;
        const uint32_t rows_here = left < RT * 16u ? (uint32_t)left : RT * 16u;
        const bool mac_any = a.S >= 2u * a.min_count;  // else no N1 can satisfy mc <= N1 <= S - mc
        const uint32_t span = a.S - 2u * a.min_count;
        const uint32_t kbe = lane / NSL, ie = lane % NSL;
        const uint32_t row = 16u * (ie >> 2) + 4u * kbe + (ie & 3u);
        const E n1 = n1s[lane];
        const float f = (float)n1, Nf = (float)a.S;
        ok = mac_any & (row < rows_here) & (((uint32_t)n1 - a.min_count) <= span);
        const float sq = __builtin_amdgcn_sqrtf(f * (Nf - f)) * 0.99999905f;
        float2 tm;
        tm.x = ok ? sq : __builtin_huge_valf();
        tm.y = (a.eg_max + fminf(a.rall_max, f * a.rmax_max)) * 1.000001f;
        if (ABLATE & 16) tm = make_float2(1000.0f + m, 1.0f);
        trm[lane] = tm;
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int i = 0; i < RT * 4; i += 2) {
        const float4 v = *reinterpret_cast<const float4*>(trm + kb * NSL + i);
        sqd[i] = v.x;
        er[i] = v.y;
        sqd[i + 1] = v.z;
        er[i + 1] = v.w;
    }
    return ok ? 1u : 0u;
}

// ABLATE & 1: no tests - an XOR keeps every accumulator (and its MFMAs) alive at one lane-op each.
template <int RT, int NT, class V4>
__device__ __forceinline__ void filter_xor_hits(const V4 (&acc)[RT][NT], uint64_t (&hit)[RT * 4]) {
#pragma unroll
    for (int i = 0; i < RT * 4; i++) hit[i] = 0;
    uint32_t x = 0;
#pragma unroll
    for (int i = 0; i < RT * 4; i++)
#pragma unroll
        for (int t = 0; t < NT; t++) x ^= __builtin_bit_cast(uint32_t, acc[i >> 2][t][i & 3]);
    hit[0] = __ballot(x == 0x7fffffffu);
}

// ---- hits -> survivor bits -------------------------------------------------------------------------------------------
// hit[i] = ballot of "row slot i may have a survivor among this lane's columns". Which pairs passed is only worked out
// for the row slots with a hit (steady state: ~2 of the 1024 (lane, slot) units of a pass): pair (row slot i, column
// g * 16 + m) survives iff margin(i, g, alpha) + E_i >= 0, margin being the kernel's |Dc| - alpha * sqrt(d_i).
// Column (g, m)'s row bits then sit in four lanes (kb = 0..3; bit i = 4 rt + jj of mb[g] is row 16 rt + 4 kb + jj of the
// wave's rows). The chunk's bitmap is [column][64-row word], nibble-transposed (quarter kb, nibble rt = row / 16):
// a wave with four row tiles stores its 16 bits as quarter kb of the column's word, one with two row tiles its 8 bits as
// byte (rbase / 32) % 2 of that quarter - no cross-lane traffic, and launch_bitmap_keys (survivors.hip) puts
// the nibbles back in row order. The bitmap is zeroed beforehand; only non-zero pieces are stored.
template <int ABLATE, int PG, int RT, class Args, class Margin>
__device__ __forceinline__ void filter_emit(const Args& a, const uint64_t (&hit)[RT * 4], const float (&alc)[PG], const float (&er)[RT * 4],
                                            const int* colp, uint64_t rbase, uint32_t lane, Margin margin) {
    static_assert(RT == 2 || RT == 4, "row tiles per wave");
    const uint32_t kb = lane >> 4, m = lane & 15u;
    uint64_t hit_any = 0;
#pragma unroll
    for (int i = 0; i < RT * 4; i++) hit_any |= hit[i];
    if ((ABLATE & 32) && hit_any) {
        if (lane == 0) atomicAdd(&a.tested[0], 0ull);
        hit_any = 0;
    }
    if (!hit_any) return;  // wave-uniform
    uint32_t mb[PG];
#pragma unroll
    for (int g = 0; g < PG; g++) mb[g] = 0;
#pragma unroll
    for (int i = 0; i < RT * 4; i++) {
        if (hit[i]) {  // wave-uniform
#pragma unroll
            for (int g = 0; g < PG; g++) {
                float al = alc[g];
                asm volatile("" : "+v"(al));  // recompute here: keeping all the compare masks alive costs more
                mb[g] |= (margin(i, g, al) + er[i] >= 0.0f) ? (1u << i) : 0u;
            }
        }
    }
    if (RT == 4) {
        unsigned short* bm16 = reinterpret_cast<unsigned short*>(a.bitmap) + (rbase >> 6) * 4u + kb;
#pragma unroll
        for (int g = 0; g < PG; g++)
            if (mb[g]) bm16[(uint64_t)colp[g * 16 + m] * a.words_per_col * 4u] = (unsigned short)mb[g];  // column >= 0 wherever a bit is set
    } else {
        unsigned char* bm8 = reinterpret_cast<unsigned char*>(a.bitmap) + (rbase >> 6) * 8u + kb * 2u + ((rbase >> 5) & 1u);
#pragma unroll
        for (int g = 0; g < PG; g++)
            if (mb[g]) bm8[(uint64_t)colp[g * 16 + m] * a.words_per_col * 8u] = (unsigned char)mb[g];
    }
}

// ---- the block-scaled filters (mx_kernel, mxs_kernel) ----------------------------------------------------------------
typedef int mxv8i __attribute__((ext_vector_type(8)));
typedef float mxv4f __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// A operands of step j of a 512-sample group from the lane's four row dwords: nibble bit 0 / 1 / 2 / 2 (bit 3 shifted
// down) = 0.5 / 1.0 / 2.0 / 2.0, which the step's block scale 2^0 / 2^-1 / 2^-2 / 2^-2 makes 0.5.
__host__ __device__ constexpr int mx_step_scale(int j) { return j == 0 ? 0x7F7F7F7F : j == 1 ? 0x7E7E7E7E : 0x7D7D7D7D; }
template <int ABLATE, int RT>
__device__ __forceinline__ void mx_expand_step(mxv8i (&A)[RT], const uint32_t (&piece)[RT][4], int j) {
#pragma unroll
    for (int rt = 0; rt < RT; rt++) {
        A[rt] = (mxv8i){0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int q = 0; q < 4; q++) {
            if (ABLATE & 2)
                A[rt][q] = (int)piece[rt][q];
            else
                A[rt][q] = j < 3 ? (int)(piece[rt][q] & (0x11111111u << j)) : (int)((piece[rt][q] >> 1) & 0x44444444u);
        }
    }
}
// A operand of a quarter step (128 samples): the lane's own dword shifted by 0..3
__device__ __forceinline__ mxv8i mx_expand_quarter(uint32_t w) {
    return (mxv8i){(int)(w & 0x11111111u), (int)((w >> 1) & 0x11111111u), (int)((w >> 2) & 0x11111111u), (int)((w >> 3) & 0x11111111u), 0, 0, 0, 0};
}

// A step's operands are read through three lane addresses (16-byte pieces; 8-byte pieces of the even and of the odd
// tiles - two bases, so that the two 8-byte reads of a unit are not merged into one ds_read2 whose four result
// registers then have to be moved next to their 16-byte halves), every read an immediate offset from them (a step's
// operands span < 64 KB; left alone the compiler forms each read's address with a vector add of its own).
struct MxStepAddr {
    uint32_t o16, o8, o8b;
};
// Slice operands of a wave's CT column tiles (the B side) and their MFMAs. NS slices per column (1: FP6 only); S1F =
// format of the second slice (4 = FP4 E2M1, 2 = FP6 E2M3). One (step, tile) is SB bytes: the FP6 slice (64 lanes x
// 16 B, then 64 lanes x 8 B), then the second slice in the same layout (FP4: the 16-byte pieces only). The operands are
// read one UNIT (two column tiles, 16 MFMAs with two slices) ahead of their MFMAs: while unit u's MFMAs run (256+
// cycles), the ds_reads of unit u + 1 are in flight, into the registers unit u - 1 freed. The callers pin the order
// with scheduling barriers; inside a unit the compiler interleaves freely.
template <int CT, int NS, int S1F>
struct MxOperands {
    static constexpr uint32_t SB = mx_step_bytes(NS, S1F == 2);
    static constexpr uint32_t PART0 = mx_step_bytes(1, 0);
    static constexpr int UT = 2;  // column tiles per unit (one: the same time, three or four: spills)
    static constexpr int NU = (CT + UT - 1) / UT;
    u32x4 Bx[CT], Bz[CT];  // dwords 0-3 of the first slice's operand, the second slice's
    u32x2 By[CT], Bv[CT];  // dwords 4-5 (FP6 operands only)

    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int t = 0; t < CT; t++) Bx[t] = Bz[t] = (u32x4){0u, 0u, 0u, 0u}, By[t] = Bv[t] = (u32x2){0u, 0u};
    }
    __device__ __forceinline__ void take(const MxOperands& o) {
#pragma unroll
        for (int t = 0; t < CT; t++) Bx[t] = o.Bx[t], By[t] = o.By[t], Bz[t] = o.Bz[t], Bv[t] = o.Bv[t];
    }
    // addresses of the step whose first tile's operands start at byte `base` of the LDS
    static __device__ __forceinline__ MxStepAddr step_addr(uint32_t base, uint32_t lane) {
        MxStepAddr sa;
        sa.o16 = base + lane * 16u;
        sa.o8 = base + lane * 8u + 1024u;
        sa.o8b = sa.o8 + SB;
        asm volatile("" : "+v"(sa.o16), "+v"(sa.o8), "+v"(sa.o8b));
        return sa;
    }
    template <int ABLATE>
    __device__ __forceinline__ void read_unit(int u, const MxStepAddr& sa, const char* lds, uint32_t lane) {
#pragma unroll
        for (int t = UT * u; t < (UT * u + UT < CT ? UT * u + UT : CT); t++) {
            if (ABLATE & 4) {
                Bx[t] = (u32x4){lane, (uint32_t)t, 3u, (uint32_t)u};
                By[t] = (u32x2){5u, 6u};
                Bz[t] = (u32x4){lane, (uint32_t)t, 7u, (uint32_t)u};
                Bv[t] = (u32x2){1u, 2u};
                continue;
            }
            const char* p16 = lds + sa.o16 + t * SB;
            const char* p8 = (t & 1) ? lds + sa.o8b + (t - 1) * SB : lds + sa.o8 + t * SB;
            Bx[t] = *reinterpret_cast<const u32x4*>(p16);
            By[t] = *reinterpret_cast<const u32x2*>(p8);
            if (NS == 2) {
                Bz[t] = *reinterpret_cast<const u32x4*>(p16 + PART0);
                if (S1F == 2) Bv[t] = *reinterpret_cast<const u32x2*>(p8 + PART0);
            }
        }
    }
    // One unit: RT MFMAs per slice for each of its column tiles - both slices' products into the same accumulator
    // (block scale sc0 on the first slice, 2^0 on the second; sa: the A side's scale, mx_step_scale).
    template <int RT>
    __device__ __forceinline__ void mfma_unit(int u, const mxv8i (&A)[RT], mxv4f (&acc)[RT][CT], int sa, int sc0) const {
#pragma unroll
        for (int t = UT * u; t < (UT * u + UT < CT ? UT * u + UT : CT); t++) {
            const mxv8i B0 = {(int)Bx[t].x, (int)Bx[t].y, (int)Bx[t].z, (int)Bx[t].w, (int)By[t].x, (int)By[t].y, 0, 0};
#pragma unroll
            for (int rt = 0; rt < RT; rt++)
                acc[rt][t] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(A[rt], B0, acc[rt][t], 4, 2, 0, sa, 0, sc0);
            if (NS == 2) {
                const mxv8i B1 = {(int)Bz[t].x, (int)Bz[t].y, (int)Bz[t].z, (int)Bz[t].w, S1F == 2 ? (int)Bv[t].x : 0, S1F == 2 ? (int)Bv[t].y : 0, 0, 0};
#pragma unroll
                for (int rt = 0; rt < RT; rt++)
                    acc[rt][t] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(A[rt], B1, acc[rt][t], 4, S1F, 0, sa, 0, 0x7F7F7F7F);
            }
        }
    }
};

// The epilogue of a pass of the block-scaled kernels: row terms, test, survivor bits. colc: the alphas of the wave's
// CT * 16 columns, colp: their phenotype columns. Returns 1 if this lane's row was tested.
// The test: a pair (row slot i, column p) survives iff  |acc| - alpha_p * sqrt(d_i) + E_i >= 0  (one fma with |.| as an
// operand modifier, one add; the roundings are covered by the constants' safety margins). It is only evaluated for row
// slots that can have a survivor at all: with alpha_min the smallest alpha of the lane's columns,
// max_p |acc_p| - alpha_min * sqrt(d_i) + E_i >= 0 is necessary (the fma is monotone in alpha) - a running maximum of
// |acc| per row slot (v_max3_f32 with |.| modifiers: half a lane-op per pair) and ONE fma + compare per row slot
// instead of an fma per pair. Permutation columns share their value set, so their alphas differ by the few per cent
// their thresholds do, and the pre-test flags ~1.2x the row slots the exact one would; whatever the columns, only the
// amount of rare-path work depends on how far the alphas spread.
template <int ABLATE, int CT, int RT, class Args>
__device__ __forceinline__ uint32_t mx_epilogue(const Args& a, const mxv4f (&acc)[RT][CT], float* wscr, const float* colc, const int* colp,
                                                uint64_t rbase, uint32_t lane) {
    constexpr int NSL = RT * 4;
    const uint32_t m = lane & 15u;
    float sqd[NSL], er[NSL];
    const uint32_t tested = filter_row_terms<float, ABLATE>(a, acc, wscr, rbase, lane, sqd, er);
    float alc[CT];
    float al_min = __builtin_huge_valf();
#pragma unroll
    for (int t = 0; t < CT; t++) {
        alc[t] = colc[t * 16 + m];
        al_min = fminf(al_min, alc[t]);  // (a NaN alpha - frozen column - is skipped; +inf = padding / ones column)
    }
    uint64_t hit[NSL];
    if (!(ABLATE & 1)) {
        const bool ones_lane = m == 15u;  // slot 15 of the last tile is the ones column: its accumulator (N1) is no margin
        float mx[NSL];
#pragma unroll
        for (int i = 0; i < NSL; i++) mx[i] = ones_lane ? 0.0f : fabsf(acc[i >> 2][CT - 1][i & 3]);
#pragma unroll
        for (int t = 0; t + 1 < CT; t++)
#pragma unroll
            for (int i = 0; i < NSL; i++) mx[i] = fmaxf(mx[i], fabsf(acc[i >> 2][t][i & 3]));
#pragma unroll
        for (int i = 0; i < NSL; i++) hit[i] = __ballot(fmaf(-al_min, sqd[i], mx[i]) + er[i] >= 0.0f);
    } else {
        filter_xor_hits(acc, hit);
    }
    filter_emit<ABLATE, CT, RT>(a, hit, alc, er, colp, rbase, lane, [&](int i, int t, float al) {
        return fmaf(-al, sqd[i], fabsf(acc[i >> 2][t][i & 3]));  // NaN (frozen column) never passes
    });
    __builtin_amdgcn_wave_barrier();  // the exchange area is rewritten by the next pass
    return tested;
}

}  // namespace kgwas
