// lmm_kernels.hip — device side of lmm_lrt: the ML likelihood-ratio test of y = W a + x b + u + e, u ~ N(0, lambda K / tau),
// e ~ N(0, I / tau), W = 1, for every variant of a PLINK .bed chunk (emma.R's emma.ML.LRT is the same statistic).
//
// With K = U diag(d) U^T, yt = U^T y, wt = U^T 1, xt = U^T x and h_i = 1 / (lambda d_i + 1):
//     l(lambda) = n/2 log(n / 2 pi) - n/2 + 1/2 sum log h_i - n/2 log RSS(lambda),
// RSS the residual of the h-weighted regression of yt on [wt] (H0) or [wt, xt] (H1), and with t = log lambda
//     dl/dt = 1/2 (sum h_i - n) - n/2 RSS' / RSS,  RSS' = sum h'_i r_i^2,  h' = dh/dt = h^2 - h,  r = yt - [wt xt] beta.
//
//   lmm_prep_kernel    one wave per variant: counts of the four codes (integers), af, n_miss, the tested flag, the centred value of
//                      every code, and the code bytes copied to rows of a 4-byte multiple;
//   lmm_rotate_kernel  Xt = X U on v_mfma_f64_16x16x4_f64: a wave owns 32 variants x 64 individuals (8 accumulator tiles), A is
//                      the decoded code (one per lane), B a row of U. The k of a 16-block are taken in the order 4q + s (q the
//                      lane's quarter, s the step), which lets a lane decode its four codes from ONE byte;
//   lmm_base_kernel    the sums without x at the 101 grid points (one wave each);
//   lmm_grid_kernel    G = [xt^2 | xt wt | xt yt] . HB on the same MFMA: per variant the three x sums at all grid points, with
//                      weights h and h';
//   lmm_grid_xy_kernel the xt yt sums alone, for a block of phenotype columns that share one .bed: a wave keeps its xt values and
//                      HB operands for LMM_PTILE columns at once. Every sum is the MFMA chain of lmm_grid_kernel's third row, so
//                      its bits are those of the single-phenotype pass; lmm_grid_kernel<2> leaves the two shared rows;
//   lmm_null_kernel / lmm_refine_kernel / lmm_refine_multi_kernel   one wave per model: l and dl/dt at the grid points, then every
//                      interval where dl/dt goes from + to - is refined by LMM_REFINE_STEPS bracketing steps (secant with the
//                      Illinois correction, every third one a bisection) whose sums run over i with lanes striding and a fixed
//                      butterfly; the evaluated point with the smallest |dl/dt| is the interval's candidate. Both ends and every
//                      such point are candidates; the largest l wins, the earliest on a tie.
//   lmm_null_reml_kernel / lmm_refine_all_kernel   -lmm 4: the same maximisation of the REML likelihood, then beta, se, the Wald
//                      and the score statistic from the sums at l_remle and at lambda0, and their F(1, n - 2) tails (fdist_tail.h).
//   lmm_*_cov_kernel   the same stages for W of q > 1 columns (or q = 1 given as covariates): further down, with their own notes.
// Each step is written once. `maximise` is the search, for both models (PlainModel: W = 1, on ll_from_sums and direct_sums;
// CovModel: covariates, on ll_cov and eval_cov) and both objectives (a compile-time switch). `null_body` and `refine_body` are the
// bodies of all nine null and refine kernels: the REML kernels are the ML ones plus their REML half, so the ML numbers of -lmm 4
// are those of -lmm 2 by construction. `store_lrt`, `store_untested` and `store_wald_score` are the three ways a variant's results
// are written. The __global__ functions only name their model and their LDS. The shared functions take plain pointers: the
// kernels' parameters carry __restrict__, and a second __restrict__ scope inside them changes what the compiler hoists and merges
// (it cost registers and duplicated logarithms when tried).
// Nothing here depends on a variant's neighbours or uses an atomic: a variant's numbers are the same in any batch.
//
// f64 MFMA layout (16x16x4): lane l holds A[row l & 15][k l >> 4] and B[k l >> 4][col l & 15]; result register j of lane l is
// D[row (l >> 4) + 4 j][col l & 15] - not the f32 forms' 4 (l >> 4) + j.
#include "lmm_kernels.h"

#include <utility>

#include "fdist_tail.h"

namespace kgwas {

namespace {

using d4 = __attribute__((ext_vector_type(4))) double;

__device__ inline double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ inline uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__global__ void __launch_bounds__(64) lmm_prep_kernel(const uint8_t* __restrict__ bed, LmmDims dm, double maf, double miss,
                                                      uint8_t* __restrict__ codes, LmmVariant* __restrict__ vars) {
    const uint32_t v = blockIdx.x, lane = threadIdx.x;
    const uint8_t* row = bed + (uint64_t)v * dm.bps;
    uint8_t* out = codes + (uint64_t)v * dm.bpsp;
    uint32_t c[4] = {0, 0, 0, 0};
    for (uint32_t b = lane; b < dm.bpsp; b += 64) {
        const uint32_t byte = b < dm.bps ? row[b] : 0u;
        out[b] = (uint8_t)byte;
        const uint32_t valid = b < dm.bps ? min(4u, dm.n - 4u * b) : 0u;
        for (uint32_t j = 0; j < valid; j++) {
            const uint32_t code = (byte >> (2u * j)) & 3u;
            c[0] += code == 0u;
            c[1] += code == 1u;
            c[2] += code == 2u;
            c[3] += code == 3u;
        }
    }
    for (int k = 0; k < 4; k++) c[k] = wave_sum_u32(c[k]);
    if (lane != 0) return;
    const uint32_t nn = dm.n - c[1];
    const double mean = nn ? (double)(2u * c[0] + c[2]) / (double)nn : 0.0;
    const double af = 0.5 * mean;
    const bool constant = nn == 0 || c[0] == nn || c[2] == nn || c[3] == nn;
    LmmVariant o;
    o.val[0] = 2.0 - mean;
    o.val[1] = 0.0;
    o.val[2] = 1.0 - mean;
    o.val[3] = 0.0 - mean;
    o.af = af;
    o.n_miss = c[1];
    o.tested = !constant && fmin(af, 1.0 - af) >= maf && (double)c[1] / (double)dm.n <= miss;
    vars[v] = o;
}

__global__ void __launch_bounds__(256) lmm_rotate_kernel(const uint8_t* __restrict__ codes, const LmmVariant* __restrict__ vars,
                                                         uint32_t nv, LmmDims dm, const double* __restrict__ U,
                                                         double* __restrict__ Xt) {
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
    const uint32_t v0 = blockIdx.x * LMM_VTILE;
    const uint32_t i0 = (blockIdx.y * 4 + wave) * 64;
    if (i0 >= dm.ldi) return;
    d4 acc[2][4];
    double tv[2][4];
    const uint8_t* crow[2];
    for (int m = 0; m < 2; m++) {
        const uint32_t v = v0 + 16 * m + r;
        const bool ok = v < nv;
        for (int k = 0; k < 4; k++) tv[m][k] = ok ? vars[v].val[k] : 0.0;
        crow[m] = codes + (uint64_t)(ok ? v : 0) * dm.bpsp + q;
        for (int t = 0; t < 4; t++) acc[m][t] = d4{0, 0, 0, 0};
    }
    const double* ucol = U + i0 + r;
    for (uint32_t k0 = 0; k0 < dm.n16; k0 += 16) {
        const uint32_t b0 = crow[0][k0 >> 2], b1 = crow[1][k0 >> 2];
#pragma unroll
        for (uint32_t s = 0; s < 4; s++) {
            const uint32_t c0 = (b0 >> (2 * s)) & 3u, c1 = (b1 >> (2 * s)) & 3u;
            const double a0 = c0 == 0 ? tv[0][0] : c0 == 1 ? tv[0][1] : c0 == 2 ? tv[0][2] : tv[0][3];
            const double a1 = c1 == 0 ? tv[1][0] : c1 == 1 ? tv[1][1] : c1 == 2 ? tv[1][2] : tv[1][3];
            const double* urow = ucol + (uint64_t)(k0 + 4 * q + s) * dm.ldi;
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const double b = urow[16 * t];
                acc[0][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b, acc[0][t], 0, 0, 0);
                acc[1][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b, acc[1][t], 0, 0, 0);
            }
        }
    }
    for (int m = 0; m < 2; m++)
        for (int t = 0; t < 4; t++)
            for (int j = 0; j < 4; j++)
                Xt[(uint64_t)(v0 + 16 * m + q + 4 * j) * dm.ldi + i0 + 16 * t + r] = acc[m][t][j];
}

// NS = 3: the rows xt^2, xt wt, xt yt of G[v][3][LMM_HB_COLS]; NS = 2: the first two alone, G[v][2][LMM_HB_COLS] (yt is not read).
// Every accumulator is a chain of its own, so a row's bits do not depend on NS.
template <int NS>
__global__ void __launch_bounds__(256) lmm_grid_kernel(const double* __restrict__ Xt, uint32_t nv, LmmDims dm,
                                                       const double* __restrict__ wt, const double* __restrict__ yt,
                                                       const double* __restrict__ HB, double* __restrict__ G) {
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
    const uint32_t v0 = (blockIdx.x * 4 + wave) * 16;
    if (v0 >= nv) return;
    const uint32_t tile0 = blockIdx.y * 4, n_tiles = LMM_HB_COLS / 16;
    d4 acc[NS][4];
    for (int c = 0; c < NS; c++)
        for (int t = 0; t < 4; t++) acc[c][t] = d4{0, 0, 0, 0};
    const double* xrow = Xt + (uint64_t)(v0 + r) * dm.ldi + 4 * q;  // (rows up to nv rounded up to 16 exist: LMM_VTILE padding)
    for (uint32_t i0 = 0; i0 < dm.ldi; i0 += 16) {
#pragma unroll
        for (uint32_t s = 0; s < 4; s++) {
            const uint32_t i = i0 + 4 * q + s;
            const double x = xrow[i0 + s];
            const double axx = x * x, axw = x * wt[i], axy = NS == 3 ? x * yt[i] : 0.0;
            const double* hrow = HB + (uint64_t)i * LMM_HB_COLS + r;
#pragma unroll
            for (uint32_t t = 0; t < 4; t++) {
                if (tile0 + t >= n_tiles) continue;
                const double b = hrow[16 * (tile0 + t)];
                acc[0][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(axx, b, acc[0][t], 0, 0, 0);
                acc[1][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(axw, b, acc[1][t], 0, 0, 0);
                if (NS == 3) acc[NS - 1][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(axy, b, acc[NS - 1][t], 0, 0, 0);
            }
        }
    }
    for (int j = 0; j < 4; j++) {
        const uint32_t v = v0 + q + 4 * j;
        if (v >= nv) continue;
        for (int c = 0; c < NS; c++)
            for (uint32_t t = 0; t < 4; t++)
                if (tile0 + t < n_tiles) G[((uint64_t)v * NS + c) * LMM_HB_COLS + 16 * (tile0 + t) + r] = acc[c][t][j];
    }
}

// Gxy[p][v][c] = sum_i HB[i][c] (xt[v][i] Yt[p][i]) for the np phenotype columns of a block, v < nv. The mapping, the order of
// i (i0 in steps of 16, then s, lane quarter q) and the rounding of the A operand are lmm_grid_kernel's for its xt yt row: the
// same bits. A wave owns 16 variants x 4 column tiles x LMM_PTILE columns of Yt: x and the four B operands are loaded once
// for all of them (LMM_PTILE x 4 accumulator tiles of 4 doubles per lane).
__global__ void __launch_bounds__(256) lmm_grid_xy_kernel(const double* __restrict__ Xt, uint32_t nv, LmmDims dm,
                                                          const double* __restrict__ Yt, uint32_t np,
                                                          const double* __restrict__ HB, double* __restrict__ Gxy) {
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
    const uint32_t v0 = (blockIdx.x * 4 + wave) * 16;
    if (v0 >= nv) return;
    const uint32_t tile0 = blockIdx.y * 4, n_tiles = LMM_HB_COLS / 16;
    const uint32_t p0 = blockIdx.z * LMM_PTILE, np_here = min(LMM_PTILE, np - p0);  // (the launcher gives p0 < np)
    d4 acc[LMM_PTILE][4];
    const double* yrow[LMM_PTILE];
    for (uint32_t pp = 0; pp < LMM_PTILE; pp++) {
        yrow[pp] = Yt + (uint64_t)(p0 + (pp < np_here ? pp : 0)) * dm.ldi;  // (columns past np: a valid row, never used)
        for (int t = 0; t < 4; t++) acc[pp][t] = d4{0, 0, 0, 0};
    }
    const double* xrow = Xt + (uint64_t)(v0 + r) * dm.ldi + 4 * q;  // (rows up to nv rounded up to 16 exist: LMM_VTILE padding)
    for (uint32_t i0 = 0; i0 < dm.ldi; i0 += 16) {
#pragma unroll
        for (uint32_t s = 0; s < 4; s++) {
            const uint32_t i = i0 + 4 * q + s;
            const double x = xrow[i0 + s];
            double axy[LMM_PTILE];
#pragma unroll
            for (uint32_t pp = 0; pp < LMM_PTILE; pp++) axy[pp] = x * yrow[pp][i];
            const double* hrow = HB + (uint64_t)i * LMM_HB_COLS + r;
#pragma unroll
            for (uint32_t t = 0; t < 4; t++) {
                if (tile0 + t >= n_tiles) continue;
                const double b = hrow[16 * (tile0 + t)];
#pragma unroll
                for (uint32_t pp = 0; pp < LMM_PTILE; pp++)
                    if (pp < np_here) acc[pp][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(axy[pp], b, acc[pp][t], 0, 0, 0);
            }
        }
    }
    for (int j = 0; j < 4; j++) {
        const uint32_t v = v0 + q + 4 * j;
        if (v >= nv) continue;
#pragma unroll
        for (uint32_t pp = 0; pp < LMM_PTILE; pp++) {
            if (pp >= np_here) continue;
#pragma unroll
            for (uint32_t t = 0; t < 4; t++)
                if (tile0 + t < n_tiles) Gxy[((uint64_t)(p0 + pp) * nv + v) * LMM_HB_COLS + 16 * (tile0 + t) + r] = acc[pp][t][j];
        }
    }
}

__global__ void __launch_bounds__(64) lmm_base_kernel(LmmDims dm, const double* __restrict__ d, const double* __restrict__ wt,
                                                      const double* __restrict__ yt, const double* __restrict__ grid,
                                                      double* __restrict__ base) {
    const uint32_t g = blockIdx.x, lane = threadIdx.x;
    yt += (uint64_t)blockIdx.y * dm.ldi;  // blockIdx.y: the phenotype column (rows of Yt, blocks of base)
    base += (uint64_t)blockIdx.y * LMM_GRID * LMM_BASE;
    const double lam = grid[g];
    double s[LMM_BASE] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t i = lane; i < dm.n; i += 64) {
        const double ld = lam * d[i], h = 1.0 / (ld + 1.0), hd = h * h - h, w = wt[i], y = yt[i];
        s[0] += h;
        s[1] -= log1p(ld);
        s[2] += h * w * w;
        s[3] += h * w * y;
        s[4] += h * y * y;
        s[5] += hd * w * w;
        s[6] += hd * w * y;
        s[7] += hd * y * y;
    }
    for (uint32_t k = 0; k < LMM_BASE; k++) s[k] = wave_sum(s[k]);
    if (lane < LMM_BASE) base[g * LMM_BASE + lane] = s[lane];
}

struct Sums {
    double sh, slog, ww, wy, yy, dww, dwy, dyy;  // as a row of base
    double xx, xw, xy, dxx, dxw, dxy;
};

// l and dl/dt from the weighted sums. REML = false: the ML likelihood above. REML = true: the restricted likelihood of -lmm 4,
//     lR(lambda) = df/2 (log(df / 2 pi) - 1) + 1/2 sum log h_i - 1/2 log |X^T H X| - df/2 log RSS,  df = n - 1 (H0) or n - 2 (H1),
// X = [wt] or [wt xt], |X^T H X| = ww or ww xx.w; its derivative adds -1/2 d log |X^T H X| / dt, from the h' sums.
template <bool HAS_X, bool REML = false>
__device__ inline void ll_from_sums(const Sums& s, double n, double& l, double& dl) {
    const double bw0 = s.wy / s.ww;
    double rss = s.yy - s.wy * bw0, drss;
    double det = s.ww, ddet = s.dww;  // |X^T H X| and its derivative (REML)
    if (HAS_X) {
        const double xxw = s.xx - s.xw * s.xw / s.ww, xyw = s.xy - s.xw * bw0;
        const double bx = xyw / xxw, bw = (s.wy - s.xw * bx) / s.ww;
        rss -= xyw * bx;
        drss = s.dyy - 2.0 * (bw * s.dwy + bx * s.dxy) + bw * bw * s.dww + 2.0 * bw * bx * s.dxw + bx * bx * s.dxx;
        if (REML) {
            det = s.ww * xxw;
            ddet = s.dww * s.xx + s.dxx * s.ww - 2.0 * s.dxw * s.xw;
        }
    } else {
        drss = s.dyy - 2.0 * bw0 * s.dwy + bw0 * bw0 * s.dww;
    }
    if (REML) {
        const double df = n - (HAS_X ? 2.0 : 1.0);
        l = 0.5 * df * (log(df / 6.283185307179586476925) - 1.0) + 0.5 * s.slog - 0.5 * log(det) - 0.5 * df * log(rss);
        dl = 0.5 * (s.sh - n) - 0.5 * ddet / det - 0.5 * df * drss / rss;
    } else {
        l = 0.5 * n * (log(n / 6.283185307179586476925) - 1.0) + 0.5 * s.slog - 0.5 * n * log(rss);
        dl = 0.5 * (s.sh - n) - 0.5 * n * drss / rss;
    }
}

// the sums at one lambda, over i with lanes striding; every lane gets them
template <bool HAS_X, bool WITH_LOG>
__device__ inline Sums direct_sums(double lam, uint32_t n, const double* __restrict__ d, const double* __restrict__ wt,
                                   const double* __restrict__ yt, const double* __restrict__ xt) {
    Sums s = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t i = threadIdx.x; i < n; i += 64) {
        const double ld = lam * d[i], h = 1.0 / (ld + 1.0), hd = h * h - h, w = wt[i], y = yt[i];
        s.sh += h;
        if (WITH_LOG) s.slog -= log1p(ld);
        s.ww += h * w * w;
        s.wy += h * w * y;
        s.yy += h * y * y;
        s.dww += hd * w * w;
        s.dwy += hd * w * y;
        s.dyy += hd * y * y;
        if (HAS_X) {
            const double x = xt[i];
            s.xx += h * x * x;
            s.xw += h * x * w;
            s.xy += h * x * y;
            s.dxx += hd * x * x;
            s.dxw += hd * x * w;
            s.dxy += hd * x * y;
        }
    }
    s.sh = wave_sum(s.sh);
    if (WITH_LOG) s.slog = wave_sum(s.slog);
    s.ww = wave_sum(s.ww), s.wy = wave_sum(s.wy), s.yy = wave_sum(s.yy);
    s.dww = wave_sum(s.dww), s.dwy = wave_sum(s.dwy), s.dyy = wave_sum(s.dyy);
    if (HAS_X) {
        s.xx = wave_sum(s.xx), s.xw = wave_sum(s.xw), s.xy = wave_sum(s.xy);
        s.dxx = wave_sum(s.dxx), s.dxw = wave_sum(s.dxw), s.dxy = wave_sum(s.dxy);
    }
    return s;
}

// The Schur complements after w of the sums at one lambda
struct AfterW {
    double xx, xy, yy;
};
__device__ inline AfterW after_w(const Sums& s) {
    const double bw0 = s.wy / s.ww;
    return {s.xx - s.xw * s.xw / s.ww, s.xy - s.xw * bw0, s.yy - s.wy * bw0};
}

// A *model* is what the search below and the bodies of the null and refine kernels see of the likelihood: l and dl/dt at grid
// point g (from the sums the grid kernels left), l and dl/dt at a lambda off the grid (the wave sums over i itself, with or without
// the log-determinant sum), the Schur complements at a lambda, and the degrees of freedom of its RSS. REML picks the objective of
// ll_from_sums / ll_cov. Every lane gets the same numbers.
//
// PlainModel: W = 1. Gx = the variant's xt^2 and xt wt rows of the grid sums, Gxy = its xt yt row (HAS_X; null pointers without).
template <bool HAS_X>
struct PlainModel {
    uint32_t n;
    const double *d, *wt, *yt, *xt, *Gx, *Gxy, *base;

    template <bool REML>
    __device__ __forceinline__ void at_grid(uint32_t g, double& l, double& dl) const {
        const double* b = base + g * LMM_BASE;
        Sums s = {b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7], 0, 0, 0, 0, 0, 0};
        if (HAS_X) {
            s.xx = Gx[g], s.xw = Gx[LMM_HB_COLS + g], s.xy = Gxy[g];
            s.dxx = Gx[LMM_GRID + g], s.dxw = Gx[LMM_HB_COLS + LMM_GRID + g], s.dxy = Gxy[LMM_GRID + g];
        }
        ll_from_sums<HAS_X, REML>(s, (double)n, l, dl);
    }
    template <bool REML, bool WITH_LOG>
    __device__ __forceinline__ void at_lambda(double lam, double& l, double& dl) const {
        ll_from_sums<HAS_X, REML>(direct_sums<HAS_X, WITH_LOG>(lam, n, d, wt, yt, xt), (double)n, l, dl);
    }
    __device__ __forceinline__ AfterW after_w_at(double lam) const { return after_w(direct_sums<HAS_X, false>(lam, n, d, wt, yt, xt)); }
    __device__ __forceinline__ double df() const { return (double)n - (HAS_X ? 2.0 : 1.0); }
};

// One wave (a block of 64): the maximum of l over the grid's ends and the refined interior points. grid = lambda[101], then
// t[101] = log lambda. s_l, s_dl: LMM_GRID doubles of LDS each. The one copy of the rule: both models, ML and REML, run these
// steps, so a change to it (the step count, the tie-break, another candidate) reaches every kernel at once.
template <bool REML, class Model>
__device__ __forceinline__ void maximise(const Model& m, const double* grid, double* s_l, double* s_dl, double& best_l,
                                         double& best_lam) {
    for (uint32_t g = threadIdx.x; g < LMM_GRID; g += 64) m.template at_grid<REML>(g, s_l[g], s_dl[g]);
    __syncthreads();
    best_l = s_l[0];
    best_lam = grid[0];
    if (s_l[LMM_GRID - 1] > best_l) {
        best_l = s_l[LMM_GRID - 1];
        best_lam = grid[LMM_GRID - 1];
    }
    for (uint32_t g = 0; g + 1 < LMM_GRID; g++) {
        double fa = s_dl[g], fb = s_dl[g + 1];
        if (!(fa > 0.0 && fb <= 0.0)) continue;  // (wave-uniform: LDS values)
        double ta = grid[LMM_GRID + g], tb = grid[LMM_GRID + g + 1];
        int side = 0;
        // the evaluated point with the smallest |dl/dt| so far (an Illinois step overshoots on purpose: the last point
        // need not be the best one)
        double t_best = fa < -fb ? ta : tb, f_best = fa < -fb ? fa : -fb;
        for (uint32_t step = 0; step < LMM_REFINE_STEPS; step++) {
            double tm = (ta * fb - tb * fa) / (fb - fa);
            if (step % 3 == 2 || !(tm > ta && tm < tb)) tm = 0.5 * (ta + tb);
            double l, dl;
            m.template at_lambda<REML, false>(exp(tm), l, dl);
            if (fabs(dl) < f_best) {
                f_best = fabs(dl);
                t_best = tm;
            }
            if (dl > 0.0) {
                ta = tm, fa = dl;
                if (side == 1) fb *= 0.5;
                side = 1;
            } else {
                tb = tm, fb = dl;
                if (side == -1) fa *= 0.5;
                side = -1;
            }
        }
        // the candidate: l there, with the log-determinant term
        const double lam = exp(t_best);
        double l, dl;
        m.template at_lambda<REML, true>(lam, l, dl);
        if (l > best_l) {
            best_l = l;
            best_lam = lam;
        }
    }
}

// The body of the null kernels. out = (l0, lambda0) of the ML likelihood; REML (-lmm 4): (lR0, lambda0_remle, vg, ve) with
// ve = RSS0 / df and vg = lambda ve at the maximiser.
template <bool REML, class Model>
__device__ __forceinline__ void null_body(const Model& m, const double* grid, double* s_l, double* s_dl,
                                          double* out) {
    double l, lam;
    maximise<REML>(m, grid, s_l, s_dl, l, lam);
    AfterW a = {0, 0, 0};
    if (REML) a = m.after_w_at(lam);
    if (threadIdx.x == 0) {
        out[0] = l;
        out[1] = lam;
        if (REML) {
            const double ve = a.yy / m.df();
            out[2] = lam * ve;
            out[3] = ve;
        }
    }
}

// What one lane stores for a variant: the LRT of the maximum (l, lam) against the null model's l0 ...
__device__ inline void store_lrt(uint64_t o, double l, double lam, double l0, double* lrt, double* lam_out,
                                 double* p_out) {
    const double stat = fmax(0.0, 2.0 * (l - l0));
    lrt[o] = stat;
    lam_out[o] = lam;
    p_out[o] = erfc(sqrt(0.5 * stat));
}
// ... and NaN everywhere for a variant that is not tested (ALL: the five -lmm 4 outputs too)
template <bool ALL>
__device__ inline void store_untested(uint64_t o, double* lrt, double* lam_out, double* p_out,
                                      const LmmWaldOut& w) {
    lrt[o] = lam_out[o] = p_out[o] = __builtin_nan("");
    if (ALL) w.beta[o] = w.se[o] = w.lam[o] = w.p_wald[o] = w.p_score[o] = __builtin_nan("");
}

// -lmm 4's close, from the Schur complements a at l_remle = lamr (Wald) and a0 at the null model's ML lambda0 (score): lane 0
// closes the Wald test and lane 1 the score test, so the two F(1, df) tails (fdist_tail.h) run side by side. nd = n.
__device__ inline void store_wald_score(uint64_t o, const AfterW& a, const AfterW& a0, double nd, double df, double lamr,
                                        const LmmWaldOut& w) {
    if (threadIdx.x >= 2) return;
    const double beta = a.xy / a.xx, rss1 = a.yy - a.xy * beta;
    // F_wald = (yy.w - RSS1) df / RSS1 with yy.w - RSS1 = xy.w beta taken as the product it is: (beta / se)^2 to a few ulps
    const double F = threadIdx.x == 0 ? a.xy * beta * df / rss1 : nd * a0.xy * a0.xy / (a0.xx * a0.yy);
    const double p = fdist_tail(F, df);
    if (threadIdx.x == 0) {
        w.beta[o] = beta;
        w.se[o] = sqrt(rss1 / (df * a.xx));
        w.lam[o] = lamr;
        w.p_wald[o] = p;
    } else {
        w.p_score[o] = p;
    }
}

// The body of the refine kernels, one wave per model m of a variant: the ML maximisation and its LRT at index o. ALL (-lmm 4): then
// the REML maximisation over the same rows in the same LDS, the Schur complements at l_remle and at lam0, and the close. The ML
// half is one source for both, so lrt, lambda and p have the same bits with and without ALL. l0 is read by lane 0 alone.
template <bool ALL, class Model>
__device__ __forceinline__ void refine_body(const Model& m, uint32_t tested, uint64_t o, const double* grid, double* s_l,
                                            double* s_dl, const double& l0, double lam0, double* lrt,
                                            double* lam_out, double* p_out, const LmmWaldOut& w) {
    if (!tested) {  // (the whole block leaves)
        if (threadIdx.x == 0) store_untested<ALL>(o, lrt, lam_out, p_out, w);
        return;
    }
    double l, lam;
    maximise<false>(m, grid, s_l, s_dl, l, lam);
    if (threadIdx.x == 0) store_lrt(o, l, lam, l0, lrt, lam_out, p_out);
    if constexpr (ALL) {
        __syncthreads();  // (s_l and s_dl are written again)
        double lr, lamr;
        maximise<true>(m, grid, s_l, s_dl, lr, lamr);
        const AfterW a = m.after_w_at(lamr);
        const AfterW a0 = m.after_w_at(lam0);
        store_wald_score(o, a, a0, (double)m.n, m.df(), lamr, w);
    }
}

// blockIdx.x: the phenotype column (rows of Yt, blocks of base, pairs of out)
__global__ void __launch_bounds__(64) lmm_null_kernel(LmmDims dm, const double* __restrict__ d, const double* __restrict__ wt,
                                                      const double* __restrict__ yt, const double* __restrict__ grid,
                                                      const double* __restrict__ base, double* __restrict__ out) {
    __shared__ double s_l[LMM_GRID], s_dl[LMM_GRID];
    const uint32_t col = blockIdx.x;
    const PlainModel<false> m = {dm.n, d, wt, yt + (uint64_t)col * dm.ldi, nullptr, nullptr, nullptr, base + (uint64_t)col * LMM_GRID * LMM_BASE};
    null_body<false>(m, grid, s_l, s_dl, out + 2 * col);
}

// -lmm 4: the REML null model
__global__ void __launch_bounds__(64) lmm_null_reml_kernel(LmmDims dm, const double* __restrict__ d, const double* __restrict__ wt,
                                                           const double* __restrict__ yt, const double* __restrict__ grid,
                                                           const double* __restrict__ base, double* __restrict__ out) {
    __shared__ double s_l[LMM_GRID], s_dl[LMM_GRID];
    const PlainModel<false> m = {dm.n, d, wt, yt, nullptr, nullptr, nullptr, base};
    null_body<true>(m, grid, s_l, s_dl, out);
}

__global__ void __launch_bounds__(64) lmm_refine_kernel(const double* __restrict__ Xt, const double* __restrict__ G,
                                                        const LmmVariant* __restrict__ vars, LmmDims dm, const double* __restrict__ d,
                                                        const double* __restrict__ wt, const double* __restrict__ yt,
                                                        const double* __restrict__ grid, const double* __restrict__ base, double l0,
                                                        double* __restrict__ lrt, double* __restrict__ lam_out,
                                                        double* __restrict__ p_out) {
    __shared__ double s_l[LMM_GRID], s_dl[LMM_GRID];
    const uint32_t v = blockIdx.x;
    const double* Gv = G + (uint64_t)v * 3 * LMM_HB_COLS;
    const PlainModel<true> m = {dm.n, d, wt, yt, Xt + (uint64_t)v * dm.ldi, Gv, Gv + 2 * LMM_HB_COLS, base};
    refine_body<false>(m, vars[v].tested, v, grid, s_l, s_dl, l0, 0.0, lrt, lam_out, p_out, LmmWaldOut{});
}

// The same per (variant blockIdx.x, phenotype column blockIdx.y of a block): Gx[v][2][LMM_HB_COLS] is shared by the columns,
// Gxy[p][v][LMM_HB_COLS], Yt[p][ldi], base[p][LMM_GRID][LMM_BASE] and null[p] = (l0, lambda0) are the column's. Results at [p][v].
__global__ void __launch_bounds__(64) lmm_refine_multi_kernel(const double* __restrict__ Xt, const double* __restrict__ Gx,
                                                              const double* __restrict__ Gxy, const LmmVariant* __restrict__ vars,
                                                              uint32_t nv, LmmDims dm, const double* __restrict__ d,
                                                              const double* __restrict__ wt, const double* __restrict__ Yt,
                                                              const double* __restrict__ grid, const double* __restrict__ base,
                                                              const double* __restrict__ null, double* __restrict__ lrt,
                                                              double* __restrict__ lam_out, double* __restrict__ p_out) {
    __shared__ double s_l[LMM_GRID], s_dl[LMM_GRID];
    const uint32_t v = blockIdx.x, col = blockIdx.y;
    const uint64_t o = (uint64_t)col * nv + v;
    const PlainModel<true> m = {dm.n, d, wt, Yt + (uint64_t)col * dm.ldi, Xt + (uint64_t)v * dm.ldi, Gx + (uint64_t)v * 2 * LMM_HB_COLS,
                                Gxy + o * LMM_HB_COLS, base + (uint64_t)col * LMM_GRID * LMM_BASE};
    refine_body<false>(m, vars[v].tested, o, grid, s_l, s_dl, null[2 * col], 0.0, lrt, lam_out, p_out, LmmWaldOut{});
}

// -lmm 4, one wave per variant: lmm_refine_kernel's body with its REML half (beta, se, l_remle, the Wald and the score p to w)
__global__ void __launch_bounds__(64) lmm_refine_all_kernel(const double* __restrict__ Xt, const double* __restrict__ G,
                                                            const LmmVariant* __restrict__ vars, LmmDims dm, const double* __restrict__ d,
                                                            const double* __restrict__ wt, const double* __restrict__ yt,
                                                            const double* __restrict__ grid, const double* __restrict__ base, double l0,
                                                            double lam0, double* __restrict__ lrt, double* __restrict__ lam_out,
                                                            double* __restrict__ p_out, LmmWaldOut w) {
    __shared__ double s_l[LMM_GRID], s_dl[LMM_GRID];
    const uint32_t v = blockIdx.x;
    const double* Gv = G + (uint64_t)v * 3 * LMM_HB_COLS;
    const PlainModel<true> m = {dm.n, d, wt, yt, Xt + (uint64_t)v * dm.ldi, Gv, Gv + 2 * LMM_HB_COLS, base};
    refine_body<true>(m, vars[v].tested, v, grid, s_l, s_dl, l0, lam0, lrt, lam_out, p_out, w);
}

// ---- covariates: W is n x Q, 1 <= Q <= LMM_MAXC, with orthonormal columns whose span holds the constant vector (lmm.cpp sees to
// both). Wt[Q][ldi] = (U^T W)^T replaces wt. The search and the kernel bodies are the ones above, on CovModel; a handle without
// covariates launches the kernels above and never comes here (their instructions are what they were before CovModel existed). ----
//
// Per lambda, with z = (wt_0 .. wt_{Q-1}, yt, xt): every sum_i h_i z_a z_b and sum_i h'_i z_a z_b, a <= b. From those without x
// the wave makes a *record* of LMM_BASEC doubles (the layout stands beside LMM_BASEC): A = Wt^T H Wt is factored (Cholesky, every
// lane the same arithmetic in registers), lane c < Q solves for column c of A^-1 and lane Q for A^-1 b. A variant then costs
// O(Q^2) per lambda (ll_cov): g = A^-1 xw, xx.w = xx - xw^T g, xy.w = xy - xw^T A^-1 b, bx = xy.w / xx.w, RSS = RSS0 - xy.w bx,
// RSS' = the h'-weighted quadratic form of (a, bx, -1) with a = A^-1 b - g bx; REML adds log|A| + log xx.w and its derivative
// tr(A^-1 dA) + (dxx - 2 g^T dxw + g^T dA g) / xx.w. The record of a grid point comes from lmm_base_cov_kernel; at the lambdas
// of the refinement the wave sums over i itself, in passes of LMM_COV_PASS pairs (twice that many running sums per lane, the
// first pass two more), into LDS, and builds the record there.

constexpr int LMM_COV_MZ = LMM_MAXC + 2;  // row stride of the pair sums in LDS
constexpr int LMM_COV_PASS = 8;

struct CovLds {
    double Sh[LMM_COV_MZ * LMM_COV_MZ], Sd[LMM_COV_MZ * LMM_COV_MZ];  // [a][b], a <= b: sums with weights h and h'
    double sh, slog;
    double rec[LMM_BASEC];
};

// pair k of the upper triangle of an M x M matrix, row by row
constexpr int pair_a(int M, int k) {
    int a = 0;
    while (k >= M - a) k -= M - a, a++;
    return a;
}
constexpr int pair_b(int M, int k) {
    int a = 0;
    while (k >= M - a) k -= M - a, a++;
    return a + k;
}

template <int M, int K>
__device__ inline void cov_acc_pair(const double (&z)[M], double h, double hd, double& ah, double& ad) {
    constexpr int a = pair_a(M, K), b = pair_b(M, K);
    const double zz = z[a] * z[b];
    ah += h * zz;
    ad += hd * zz;
}
template <int M, int K>
__device__ inline void cov_store_pair(CovLds& L, double ah, double ad) {
    constexpr int a = pair_a(M, K), b = pair_b(M, K);
    L.Sh[a * LMM_COV_MZ + b] = ah;
    L.Sd[a * LMM_COV_MZ + b] = ad;
}

// pairs K0 .. K0 + NP of the M rows zp (each of n doubles) at one lambda, lanes striding over i, then a fixed butterfly
template <int M, int K0, bool WITH_LOG, int... I>
__device__ inline void cov_sum_pass(std::integer_sequence<int, I...>, double lam, uint32_t n, const double* __restrict__ d,
                                    const double* const (&zp)[M], CovLds& L) {
    constexpr int NP = sizeof...(I);
    double ah[NP], ad[NP], sh = 0, slog = 0;
    for (int k = 0; k < NP; k++) ah[k] = ad[k] = 0;
    for (uint32_t i = threadIdx.x; i < n; i += 64) {
        const double ld = lam * d[i], h = 1.0 / (ld + 1.0), hd = h * h - h;
        double z[M];
#pragma unroll
        for (int a = 0; a < M; a++) z[a] = zp[a][i];  // (the rows no pair of this pass names are not loaded)
        if (K0 == 0) {
            sh += h;
            if (WITH_LOG) slog -= log1p(ld);
        }
        (cov_acc_pair<M, K0 + I>(z, h, hd, ah[I], ad[I]), ...);
    }
#pragma unroll
    for (int k = 0; k < NP; k++) ah[k] = wave_sum(ah[k]), ad[k] = wave_sum(ad[k]);
    if (K0 == 0) {
        sh = wave_sum(sh);
        if (WITH_LOG) slog = wave_sum(slog);
    }
    if (threadIdx.x == 0) {
        (cov_store_pair<M, K0 + I>(L, ah[I], ad[I]), ...);
        if (K0 == 0) L.sh = sh, L.slog = slog;
    }
}
template <int M, int K0, bool WITH_LOG>
__device__ inline void cov_sum_passes(double lam, uint32_t n, const double* __restrict__ d, const double* const (&zp)[M], CovLds& L) {
    constexpr int TOTAL = M * (M + 1) / 2;
    if constexpr (K0 < TOTAL) {
        constexpr int NP = TOTAL - K0 < LMM_COV_PASS ? TOTAL - K0 : LMM_COV_PASS;
        cov_sum_pass<M, K0, WITH_LOG>(std::make_integer_sequence<int, NP>{}, lam, n, d, zp, L);
        cov_sum_passes<M, K0 + LMM_COV_PASS, WITH_LOG>(lam, n, d, zp, L);
    }
}

// The record from the sums in L.Sh, L.Sd, L.sh, L.slog (written by lane 0; the caller has NOT yet synchronised): L.rec. The wave
// is synchronised on return.
template <int Q>
__device__ inline void cov_record(CovLds& L) {
    constexpr int MZ = LMM_COV_MZ;
    const int lane = threadIdx.x;
    __syncthreads();
    double C[Q][Q], rc[Q];  // the lower Cholesky factor of A, below the diagonal; rc = 1 / its diagonal
    double logdet = 0;
#pragma unroll
    for (int j = 0; j < Q; j++) {
#pragma unroll
        for (int k = 0; k < j; k++) {
            double s = L.Sh[k * MZ + j];
#pragma unroll
            for (int t = 0; t < k; t++) s -= C[j][t] * C[k][t];
            C[j][k] = s * rc[k];
        }
        double s = L.Sh[j * MZ + j];
#pragma unroll
        for (int t = 0; t < j; t++) s -= C[j][t] * C[j][t];
        logdet += log(s);  // (log |A| = sum log C[j][j]^2)
        rc[j] = 1.0 / sqrt(s);
    }
    // lane c < Q: column c of A^-1; the others: A^-1 b (lane Q stores it)
    double u[Q];
#pragma unroll
    for (int k = 0; k < Q; k++) {
        double s = lane < Q ? (k == lane ? 1.0 : 0.0) : L.Sh[k * MZ + Q];
#pragma unroll
        for (int t = 0; t < k; t++) s -= C[k][t] * u[t];
        u[k] = s * rc[k];
    }
#pragma unroll
    for (int k = Q - 1; k >= 0; k--) {
        double s = u[k];
#pragma unroll
        for (int t = k + 1; t < Q; t++) s -= C[t][k] * u[t];
        u[k] = s * rc[k];
    }
#pragma unroll
    for (int k = 0; k < Q; k++) {
        if (lane < Q) L.rec[LMM_REC_AINV + k * LMM_MAXC + lane] = u[k];
        if (lane == Q) L.rec[LMM_REC_A0 + k] = u[k];
    }
    if (lane < Q * Q) {  // dA, both triangles
        const int j = lane / Q, k = lane % Q;
        L.rec[LMM_REC_DA + j * LMM_MAXC + k] = L.Sd[(j < k ? j : k) * MZ + (j < k ? k : j)];
    }
    if (lane < Q) {
        L.rec[LMM_REC_DB + lane] = L.Sd[lane * MZ + Q];
        L.rec[LMM_REC_B + lane] = L.Sh[lane * MZ + Q];
    }
    __syncthreads();
    if (lane == 0) {
        double tr = 0, ba = 0, aDa = 0, adb = 0;
        for (int j = 0; j < Q; j++) {
            const double aj = L.rec[LMM_REC_A0 + j];
            double Da = 0;
            for (int k = 0; k < Q; k++) {
                tr += L.rec[LMM_REC_AINV + j * LMM_MAXC + k] * L.rec[LMM_REC_DA + j * LMM_MAXC + k];
                Da += L.rec[LMM_REC_DA + j * LMM_MAXC + k] * L.rec[LMM_REC_A0 + k];
            }
            ba += L.rec[LMM_REC_B + j] * aj;
            aDa += aj * Da;
            adb += aj * L.rec[LMM_REC_DB + j];
        }
        const double yy = L.Sh[Q * MZ + Q], dyy = L.Sd[Q * MZ + Q];
        L.rec[LMM_REC_SH] = L.sh;
        L.rec[LMM_REC_SLOG] = L.slog;
        L.rec[LMM_REC_RSS0] = yy - ba;
        L.rec[LMM_REC_LOGDET] = logdet;
        L.rec[LMM_REC_TR] = tr;
        L.rec[LMM_REC_DYY] = dyy;
        L.rec[LMM_REC_DRSS0] = aDa - 2.0 * adb + dyy;
    }
    __syncthreads();
}

struct XSums {  // a variant's sums at one lambda
    double xx, xy, dxx, dxy;
};

// l and dl/dt from a record (global memory or LDS) and, with HAS_X, the variant's sums. Also the Schur complements after W.
template <int Q, bool HAS_X, bool REML>
__device__ inline void ll_cov(const double* rec, const XSums& x, const double (&xw)[Q], const double (&dxw)[Q], double n, double& l,
                              double& dl, AfterW& s) {
    double rss = rec[LMM_REC_RSS0], drss = rec[LMM_REC_DRSS0], logdet = rec[LMM_REC_LOGDET], dlogdet = rec[LMM_REC_TR];
    s = {0.0, 0.0, rss};
    if (HAS_X) {
        double g[Q], a[Q];
        double xg = 0, xa0 = 0;
#pragma unroll
        for (int j = 0; j < Q; j++) {
            double t = 0;
#pragma unroll
            for (int k = 0; k < Q; k++) t += rec[LMM_REC_AINV + j * LMM_MAXC + k] * xw[k];
            g[j] = t;
            xg += xw[j] * t;
            xa0 += xw[j] * rec[LMM_REC_A0 + j];
        }
        const double xxw = x.xx - xg, xyw = x.xy - xa0, bx = xyw / xxw;
        s.xx = xxw, s.xy = xyw;
        rss -= xyw * bx;
        double aDa = 0, adxw = 0, adb = 0, gDg = 0, gdxw = 0;
#pragma unroll
        for (int j = 0; j < Q; j++) a[j] = rec[LMM_REC_A0 + j] - g[j] * bx;
#pragma unroll
        for (int j = 0; j < Q; j++) {
            double Da = 0, Dg = 0;
#pragma unroll
            for (int k = 0; k < Q; k++) {
                const double D = rec[LMM_REC_DA + j * LMM_MAXC + k];
                Da += D * a[k];
                if (REML) Dg += D * g[k];
            }
            aDa += a[j] * Da;
            adxw += a[j] * dxw[j];
            adb += a[j] * rec[LMM_REC_DB + j];
            if (REML) gDg += g[j] * Dg, gdxw += g[j] * dxw[j];
        }
        drss = aDa + 2.0 * bx * adxw + bx * bx * x.dxx - 2.0 * adb - 2.0 * bx * x.dxy + rec[LMM_REC_DYY];
        if (REML) {
            logdet += log(xxw);
            dlogdet += (x.dxx - 2.0 * gdxw + gDg) / xxw;
        }
    }
    const double sh = rec[LMM_REC_SH], slog = rec[LMM_REC_SLOG];
    if (REML) {
        const double df = n - (double)Q - (HAS_X ? 1.0 : 0.0);
        l = 0.5 * df * (log(df / 6.283185307179586476925) - 1.0) + 0.5 * slog - 0.5 * logdet - 0.5 * df * log(rss);
        dl = 0.5 * (sh - n) - 0.5 * dlogdet - 0.5 * df * drss / rss;
    } else {
        l = 0.5 * n * (log(n / 6.283185307179586476925) - 1.0) + 0.5 * slog - 0.5 * n * log(rss);
        dl = 0.5 * (sh - n) - 0.5 * n * drss / rss;
    }
}

// l, dl/dt and the Schur complements at one lambda off the grid: the sums over i, the record, then ll_cov; every lane gets them
template <int Q, bool HAS_X, bool REML, bool WITH_LOG>
__device__ __forceinline__ void eval_cov(double lam, uint32_t n, uint32_t ldi, const double* __restrict__ d, const double* __restrict__ Wt,
                                const double* __restrict__ yt, const double* __restrict__ xt, CovLds& L, double& l, double& dl,
                                AfterW& s) {
    constexpr int M = Q + (HAS_X ? 2 : 1), MZ = LMM_COV_MZ;
    const double* zp[M];
#pragma unroll
    for (int j = 0; j < Q; j++) zp[j] = Wt + (uint64_t)j * ldi;
    zp[Q] = yt;
    if (HAS_X) zp[M - 1] = xt;
    __syncthreads();  // (the last call's readers of L are done)
    cov_sum_passes<M, 0, WITH_LOG>(lam, n, d, zp, L);
    cov_record<Q>(L);
    XSums x = {0, 0, 0, 0};
    double xw[Q], dxw[Q];
#pragma unroll
    for (int j = 0; j < Q; j++) xw[j] = dxw[j] = 0;
    if (HAS_X) {
        x = {L.Sh[(Q + 1) * MZ + Q + 1], L.Sh[Q * MZ + Q + 1], L.Sd[(Q + 1) * MZ + Q + 1], L.Sd[Q * MZ + Q + 1]};
#pragma unroll
        for (int j = 0; j < Q; j++) xw[j] = L.Sh[j * MZ + Q + 1], dxw[j] = L.Sd[j * MZ + Q + 1];
    }
    ll_cov<Q, HAS_X, REML>(L.rec, x, xw, dxw, (double)n, l, dl, s);
}

// The model with covariates, as maximise, null_body and refine_body see it. Gv = the variant's Q + 2 rows of the grid sums (xt^2,
// xt wt_j, xt yt; HAS_X), base = the records of the grid points, L = the wave's LDS for the sums off the grid.
template <int Q, bool HAS_X>
struct CovModel {
    uint32_t n, ldi;
    const double *d, *Wt, *yt, *xt, *Gv, *base;
    CovLds& L;

    template <bool REML>
    __device__ __forceinline__ void at_grid(uint32_t g, double& l, double& dl) const {
        AfterW unused;
        XSums x = {0, 0, 0, 0};
        double xw[Q], dxw[Q];
#pragma unroll
        for (int j = 0; j < Q; j++) xw[j] = dxw[j] = 0;
        if (HAS_X) {
            x = {Gv[g], Gv[(Q + 1) * LMM_HB_COLS + g], Gv[LMM_GRID + g], Gv[(Q + 1) * LMM_HB_COLS + LMM_GRID + g]};
#pragma unroll
            for (int j = 0; j < Q; j++) xw[j] = Gv[(1 + j) * LMM_HB_COLS + g], dxw[j] = Gv[(1 + j) * LMM_HB_COLS + LMM_GRID + g];
        }
        ll_cov<Q, HAS_X, REML>(base + (uint64_t)g * LMM_BASEC, x, xw, dxw, (double)n, l, dl, unused);
    }
    template <bool REML, bool WITH_LOG>
    __device__ __forceinline__ void at_lambda(double lam, double& l, double& dl) const {
        AfterW unused;
        eval_cov<Q, HAS_X, REML, WITH_LOG>(lam, n, ldi, d, Wt, yt, xt, L, l, dl, unused);
    }
    __device__ __forceinline__ AfterW after_w_at(double lam) const {
        double l, dl;
        AfterW a;
        eval_cov<Q, HAS_X, true, false>(lam, n, ldi, d, Wt, yt, xt, L, l, dl, a);
        return a;
    }
    __device__ __forceinline__ double df() const { return (double)n - (double)Q - (HAS_X ? 1.0 : 0.0); }
};

// One wave per grid point: the record of lambda[g] to base[g][LMM_BASEC]
template <int Q>
__global__ void __launch_bounds__(64) lmm_base_cov_kernel(LmmDims dm, const double* __restrict__ d, const double* __restrict__ Wt,
                                                          const double* __restrict__ yt, const double* __restrict__ grid,
                                                          double* __restrict__ base) {
    __shared__ CovLds L;
    const uint32_t g = blockIdx.x;
    const double* zp[Q + 1];
#pragma unroll
    for (int j = 0; j < Q; j++) zp[j] = Wt + (uint64_t)j * dm.ldi;
    zp[Q] = yt;
    for (uint32_t k = threadIdx.x; k < LMM_BASEC; k += 64) L.rec[k] = 0.0;  // (the entries past Q stay zero)
    cov_sum_passes<Q + 1, 0, true>(grid[g], dm.n, d, zp, L);
    cov_record<Q>(L);
    for (uint32_t k = threadIdx.x; k < LMM_BASEC; k += 64) base[(uint64_t)g * LMM_BASEC + k] = L.rec[k];
}

// The grid sums with covariates: G[v][Q + 2][LMM_HB_COLS], rows xt^2, xt wt_j (j < q), xt yt. lmm_grid_kernel's mapping and order
// of i; blockIdx.z picks a group of up to three rows, so a wave holds lmm_grid_kernel's accumulators whatever q is.
__global__ void __launch_bounds__(256) lmm_grid_cov_kernel(const double* __restrict__ Xt, uint32_t nv, LmmDims dm, uint32_t q,
                                                           const double* __restrict__ Wt, const double* __restrict__ yt,
                                                           const double* __restrict__ HB, double* __restrict__ G) {
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, qq = lane >> 4;
    const uint32_t v0 = (blockIdx.x * 4 + wave) * 16;
    if (v0 >= nv) return;
    const uint32_t tile0 = blockIdx.y * 4, n_tiles = LMM_HB_COLS / 16;
    const uint32_t row0 = blockIdx.z * 3, n_rows = q + 2, nr = min(3u, n_rows - row0);  // (the launcher gives row0 < n_rows)
    const double* xrow = Xt + (uint64_t)(v0 + r) * dm.ldi + 4 * qq;  // (rows up to nv rounded up to 16 exist: LMM_VTILE padding)
    // the other factor of row c of the group: xt itself, a row of Wt, or yt (rows past nr: yt, never used)
    const double* other[3];
    for (uint32_t c = 0; c < 3; c++) {
        const uint32_t row = row0 + c;
        other[c] = row == 0 ? xrow - 4 * qq : row <= q ? Wt + (uint64_t)(row - 1) * dm.ldi : yt;
    }
    d4 acc[3][4];
    for (int c = 0; c < 3; c++)
        for (int t = 0; t < 4; t++) acc[c][t] = d4{0, 0, 0, 0};
    for (uint32_t i0 = 0; i0 < dm.ldi; i0 += 16) {
#pragma unroll
        for (uint32_t s = 0; s < 4; s++) {
            const uint32_t i = i0 + 4 * qq + s;
            const double x = xrow[i0 + s];
            const double a0 = x * other[0][i], a1 = nr > 1 ? x * other[1][i] : 0.0, a2 = nr > 2 ? x * other[2][i] : 0.0;
            const double* hrow = HB + (uint64_t)i * LMM_HB_COLS + r;
#pragma unroll
            for (uint32_t t = 0; t < 4; t++) {
                if (tile0 + t >= n_tiles) continue;
                const double b = hrow[16 * (tile0 + t)];
                acc[0][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b, acc[0][t], 0, 0, 0);
                if (nr > 1) acc[1][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b, acc[1][t], 0, 0, 0);
                if (nr > 2) acc[2][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, b, acc[2][t], 0, 0, 0);
            }
        }
    }
    for (int j = 0; j < 4; j++) {
        const uint32_t v = v0 + qq + 4 * j;
        if (v >= nv) continue;
        for (uint32_t c = 0; c < 3; c++) {
            if (c >= nr) continue;
            for (uint32_t t = 0; t < 4; t++)
                if (tile0 + t < n_tiles) G[((uint64_t)v * n_rows + row0 + c) * LMM_HB_COLS + 16 * (tile0 + t) + r] = acc[c][t][j];
        }
    }
}

// The null and refine kernels with covariates: the bodies of the kernels without, on a CovModel. (The evaluation off the grid is
// inlined at each of its uses, six in lmm_refine_all_cov_kernel, which costs occupancy at Q >= 5: DESIGN.md 4.12. Sharing the
// source has left that as it was.)
template <int Q>
__global__ void __launch_bounds__(64) lmm_null_cov_kernel(LmmDims dm, const double* __restrict__ d, const double* __restrict__ Wt,
                                                          const double* __restrict__ yt, const double* __restrict__ grid,
                                                          const double* __restrict__ base, double* __restrict__ out) {
    __shared__ double s_l[LMM_GRID], s_dl[LMM_GRID];
    __shared__ CovLds L;
    const CovModel<Q, false> m = {dm.n, dm.ldi, d, Wt, yt, nullptr, nullptr, base, L};
    null_body<false>(m, grid, s_l, s_dl, out);
}

template <int Q>
__global__ void __launch_bounds__(64) lmm_null_reml_cov_kernel(LmmDims dm, const double* __restrict__ d, const double* __restrict__ Wt,
                                                               const double* __restrict__ yt, const double* __restrict__ grid,
                                                               const double* __restrict__ base, double* __restrict__ out) {
    __shared__ double s_l[LMM_GRID], s_dl[LMM_GRID];
    __shared__ CovLds L;
    const CovModel<Q, false> m = {dm.n, dm.ldi, d, Wt, yt, nullptr, nullptr, base, L};
    null_body<true>(m, grid, s_l, s_dl, out);
}

template <int Q>
__global__ void __launch_bounds__(64) lmm_refine_cov_kernel(const double* __restrict__ Xt, const double* __restrict__ G,
                                                            const LmmVariant* __restrict__ vars, LmmDims dm, const double* __restrict__ d,
                                                            const double* __restrict__ Wt, const double* __restrict__ yt,
                                                            const double* __restrict__ grid, const double* __restrict__ base, double l0,
                                                            double* __restrict__ lrt, double* __restrict__ lam_out,
                                                            double* __restrict__ p_out) {
    __shared__ double s_l[LMM_GRID], s_dl[LMM_GRID];
    __shared__ CovLds L;
    const uint32_t v = blockIdx.x;
    const CovModel<Q, true> m = {dm.n, dm.ldi, d, Wt, yt, Xt + (uint64_t)v * dm.ldi, G + (uint64_t)v * (Q + 2) * LMM_HB_COLS, base, L};
    refine_body<false>(m, vars[v].tested, v, grid, s_l, s_dl, l0, 0.0, lrt, lam_out, p_out, LmmWaldOut{});
}

// -lmm 4 with covariates; the F tails have n - q - 1 degrees of freedom
template <int Q>
__global__ void __launch_bounds__(64) lmm_refine_all_cov_kernel(const double* __restrict__ Xt, const double* __restrict__ G,
                                                                const LmmVariant* __restrict__ vars, LmmDims dm,
                                                                const double* __restrict__ d, const double* __restrict__ Wt,
                                                                const double* __restrict__ yt, const double* __restrict__ grid,
                                                                const double* __restrict__ base, double l0, double lam0,
                                                                double* __restrict__ lrt, double* __restrict__ lam_out,
                                                                double* __restrict__ p_out, LmmWaldOut w) {
    __shared__ double s_l[LMM_GRID], s_dl[LMM_GRID];
    __shared__ CovLds L;
    const uint32_t v = blockIdx.x;
    const CovModel<Q, true> m = {dm.n, dm.ldi, d, Wt, yt, Xt + (uint64_t)v * dm.ldi, G + (uint64_t)v * (Q + 2) * LMM_HB_COLS, base, L};
    refine_body<true>(m, vars[v].tested, v, grid, s_l, s_dl, l0, lam0, lrt, lam_out, p_out, w);
}

}  // namespace

// ---- the launchers. q = 0: W = 1, `W` is wt[ldi] and base holds LMM_BASE sums per grid point; 1 <= q <= LMM_MAXC: `W` is
// Wt[q][ldi] and base holds records of LMM_BASEC doubles, on the <q> instantiation; any other q is refused. ----

#define LMM_DISPATCH(q, PLAIN, COV)                  \
    switch (q) {                                    \
        case 0: { PLAIN; break; }                   \
        case 1: { constexpr int Q = 1; COV; break; } \
        case 2: { constexpr int Q = 2; COV; break; } \
        case 3: { constexpr int Q = 3; COV; break; } \
        case 4: { constexpr int Q = 4; COV; break; } \
        case 5: { constexpr int Q = 5; COV; break; } \
        case 6: { constexpr int Q = 6; COV; break; } \
        case 7: { constexpr int Q = 7; COV; break; } \
        case 8: { constexpr int Q = 8; COV; break; } \
        default: return hipErrorInvalidValue;       \
    }
static_assert(LMM_MAXC == 8, "LMM_DISPATCH lists the widths");

hipError_t launch_lmm_prep(const uint8_t* bed, uint32_t nv, LmmDims dm, double maf, double miss, uint8_t* codes, LmmVariant* vars,
                           hipStream_t st) {
    if (!nv) return hipSuccess;
    hipLaunchKernelGGL(lmm_prep_kernel, dim3(nv), dim3(64), 0, st, bed, dm, maf, miss, codes, vars);
    return hipGetLastError();
}

hipError_t launch_lmm_rotate(const uint8_t* codes, const LmmVariant* vars, uint32_t nv, LmmDims dm, const double* U, double* Xt,
                             hipStream_t st) {
    if (!nv) return hipSuccess;
    const dim3 grid((nv + LMM_VTILE - 1) / LMM_VTILE, (dm.ldi / 64 + 3) / 4);
    hipLaunchKernelGGL(lmm_rotate_kernel, grid, dim3(256), 0, st, codes, vars, nv, dm, U, Xt);
    return hipGetLastError();
}

hipError_t launch_lmm_base(LmmDims dm, uint32_t q, const double* d, const double* W, const double* Yt, uint32_t np, const double* grid,
                           double* base, hipStream_t st) {
    if (!np) return hipSuccess;
    if (q && np != 1) return hipErrorInvalidValue;
    LMM_DISPATCH(q, hipLaunchKernelGGL(lmm_base_kernel, dim3(LMM_GRID, np), dim3(64), 0, st, dm, d, W, Yt, grid, base),
                 hipLaunchKernelGGL(lmm_base_cov_kernel<Q>, dim3(LMM_GRID), dim3(64), 0, st, dm, d, W, Yt, grid, base));
    return hipGetLastError();
}

hipError_t launch_lmm_grid(const double* Xt, uint32_t nv, LmmDims dm, uint32_t q, const double* W, const double* yt, const double* HB,
                           double* G, hipStream_t st) {
    if (!nv) return hipSuccess;
    if (q > LMM_MAXC) return hipErrorInvalidValue;
    const dim3 grid((nv + 63) / 64, (LMM_HB_COLS / 16 + 3) / 4, q ? (q + 2 + 2) / 3 : 1);
    if (q)
        hipLaunchKernelGGL(lmm_grid_cov_kernel, grid, dim3(256), 0, st, Xt, nv, dm, q, W, yt, HB, G);
    else
        hipLaunchKernelGGL(lmm_grid_kernel<3>, grid, dim3(256), 0, st, Xt, nv, dm, W, yt, HB, G);
    return hipGetLastError();
}

hipError_t launch_lmm_grid_shared(const double* Xt, uint32_t nv, LmmDims dm, const double* wt, const double* HB, double* Gx,
                                  hipStream_t st) {
    if (!nv) return hipSuccess;
    const dim3 grid((nv + 63) / 64, (LMM_HB_COLS / 16 + 3) / 4);
    hipLaunchKernelGGL(lmm_grid_kernel<2>, grid, dim3(256), 0, st, Xt, nv, dm, wt, (const double*)nullptr, HB, Gx);
    return hipGetLastError();
}

hipError_t launch_lmm_grid_xy(const double* Xt, uint32_t nv, LmmDims dm, const double* Yt, uint32_t np, const double* HB, double* Gxy,
                              hipStream_t st) {
    if (!nv || !np) return hipSuccess;
    if (np > LMM_PBLOCK) return hipErrorInvalidValue;
    const dim3 grid((nv + 63) / 64, (LMM_HB_COLS / 16 + 3) / 4, (np + LMM_PTILE - 1) / LMM_PTILE);
    hipLaunchKernelGGL(lmm_grid_xy_kernel, grid, dim3(256), 0, st, Xt, nv, dm, Yt, np, HB, Gxy);
    return hipGetLastError();
}

hipError_t launch_lmm_null(LmmDims dm, uint32_t q, const double* d, const double* W, const double* Yt, uint32_t np, const double* grid,
                           const double* base, double* out, hipStream_t st) {
    if (!np) return hipSuccess;
    if (q && np != 1) return hipErrorInvalidValue;
    LMM_DISPATCH(q, hipLaunchKernelGGL(lmm_null_kernel, dim3(np), dim3(64), 0, st, dm, d, W, Yt, grid, base, out),
                 hipLaunchKernelGGL(lmm_null_cov_kernel<Q>, dim3(1), dim3(64), 0, st, dm, d, W, Yt, grid, base, out));
    return hipGetLastError();
}

hipError_t launch_lmm_null_reml(LmmDims dm, uint32_t q, const double* d, const double* W, const double* yt, const double* grid,
                                const double* base, double* out, hipStream_t st) {
    LMM_DISPATCH(q, hipLaunchKernelGGL(lmm_null_reml_kernel, dim3(1), dim3(64), 0, st, dm, d, W, yt, grid, base, out),
                 hipLaunchKernelGGL(lmm_null_reml_cov_kernel<Q>, dim3(1), dim3(64), 0, st, dm, d, W, yt, grid, base, out));
    return hipGetLastError();
}

hipError_t launch_lmm_refine(const double* Xt, const double* G, const LmmVariant* vars, uint32_t nv, LmmDims dm, uint32_t q,
                             const double* d, const double* W, const double* yt, const double* grid, const double* base, double l0,
                             double* lrt, double* lam, double* p, hipStream_t st) {
    if (!nv) return hipSuccess;
    LMM_DISPATCH(q, hipLaunchKernelGGL(lmm_refine_kernel, dim3(nv), dim3(64), 0, st, Xt, G, vars, dm, d, W, yt, grid, base, l0, lrt, lam, p),
                 hipLaunchKernelGGL(lmm_refine_cov_kernel<Q>, dim3(nv), dim3(64), 0, st, Xt, G, vars, dm, d, W, yt, grid, base, l0, lrt, lam, p));
    return hipGetLastError();
}

hipError_t launch_lmm_refine_all(const double* Xt, const double* G, const LmmVariant* vars, uint32_t nv, LmmDims dm, uint32_t q,
                                 const double* d, const double* W, const double* yt, const double* grid, const double* base, double l0,
                                 double lam0, double* lrt, double* lam, double* p, LmmWaldOut w, hipStream_t st) {
    if (!nv) return hipSuccess;
    LMM_DISPATCH(q,
                 hipLaunchKernelGGL(lmm_refine_all_kernel, dim3(nv), dim3(64), 0, st, Xt, G, vars, dm, d, W, yt, grid, base, l0, lam0, lrt, lam, p, w),
                 hipLaunchKernelGGL(lmm_refine_all_cov_kernel<Q>, dim3(nv), dim3(64), 0, st, Xt, G, vars, dm, d, W, yt, grid, base, l0, lam0, lrt,
                                    lam, p, w));
    return hipGetLastError();
}

hipError_t launch_lmm_refine_multi(const double* Xt, const double* Gx, const double* Gxy, const LmmVariant* vars, uint32_t nv, LmmDims dm,
                                   const double* d, const double* wt, const double* Yt, uint32_t np, const double* grid,
                                   const double* base, const double* null, double* lrt, double* lam, double* p, hipStream_t st) {
    if (!nv || !np) return hipSuccess;
    if (np > LMM_PBLOCK) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lmm_refine_multi_kernel, dim3(nv, np), dim3(64), 0, st, Xt, Gx, Gxy, vars, nv, dm, d, wt, Yt, grid, base, null, lrt,
                       lam, p);
    return hipGetLastError();
}

}  // namespace kgwas
