// scan_plan.cpp — what a scan session is made of, worked out on the host: the plan (exact scorer, filter family, operand sets,
// their LDS groups and launches, chunk sizes) and the host-side operands (phenotype layouts of the exact scorers, the operand
// bytes and error bounds of the filters: block-scaled FP4 x FP6/FP4, int8, narrow). Arithmetic on Y only, no device calls:
// kgwas_scan_create (scan_create.cpp) uploads what these functions return.
#include "scan_internal.h"

namespace kgwas {

FilterOpts read_filter_opts() {
    FilterOpts o;
    if (const char* e = opt_str("KGWAS_COARSE_MX"))
        if (*e) o.coarse_mx = atoll(e) != 0 ? 1 : 0;  // (as opt_int: a set but empty value is no value)
    if (const char* e = opt_str("KGWAS_COARSE_SLICES")) o.coarse_slices = (atoi(e) == 1 || atoi(e) == 2) ? atoi(e) : 0;
    o.mx_s1_fp6 = opt_int("KGWAS_MX_S1", -1) == 6;
    o.mxs = (int)opt_int("KGWAS_MXS", 1);
    o.mxs_form = (int)opt_int("KGWAS_MXS_FORM", 0);
    o.narrow = !(opt_int("KGWAS_NARROW", 1) == 0);
    o.debug_residuals = opt_set("KGWAS_DEBUG_RESIDUALS");
    o.debug_survivors = opt_set("KGWAS_DEBUG_SURVIVORS");
    o.mixed = !(exp_int("KGWAS_COARSE_MIXED", 1) == 0);
    o.split = !exp_set("KGWAS_COARSE_NOSPLIT");
    o.narrow_pack = !(exp_int("KGWAS_NARROW_PACK", 1) == 0);
    o.cap_mult = exp_int("KGWAS_CAP_MULT", -1);
    o.cap_budget = exp_int("KGWAS_CAP_BUDGET", (long long)(4ull << 20));
    if (const char* e = exp_str("KGWAS_MODE_K")) o.mode_k = atof(e);
    return o;
}

// ---- exact scorers ---------------------------------------------------------------------------------------------------------

// permute_scores (src/kmer_general.cpp:155-167): R[128b+4s+l] = V[128b+32l+31-s], V a column zero-padded to L samples;
// returns update_scores_and_sum (src/kmers_multiple_databases.cpp:288-295): the sequential float32 sum of R
static float permute_and_sum(const std::vector<float>& V, float* R) {
    const uint64_t L = V.size();
    for (uint64_t b = 0; b < L / 128; b++)
        for (uint64_t sx = 0; sx < 32; sx++)
            for (uint64_t l = 0; l < 4; l++) R[128 * b + 4 * sx + l] = V[128 * b + 32 * l + 31 - sx];
    volatile float sum = 0.0f;
    for (uint64_t i = 0; i < L; i++) sum = sum + R[i];
    return sum;
}

ExactLayouts exact_layouts(const ScanShape& sh, const std::vector<uint64_t>& col, const std::vector<float>& Y) {
    const uint64_t S = sh.S, L = sh.L, W_m = sh.W_m, P = sh.P;
    ExactLayouts ex;
    ex.dmask.assign(2 * W_m, 0);
    ex.colmap.assign(L, 0xFFFFFFFFu);
    for (uint64_t d = 0; d < 2 * W_m; d++) {
        if (!sh.direct)
            ex.dmask[d] = 0xFFFFFFFFu;
        else if (32 * d + 32 <= S)
            ex.dmask[d] = 0xFFFFFFFFu;
        else if (32 * d < S)
            ex.dmask[d] = (1u << (S - 32 * d)) - 1u;
    }
    for (uint64_t i = 0; i < S; i++) ex.colmap[i] = (uint32_t)col[i];
    const uint64_t P4 = (P + 3) / 4 * 4, nct = (P + 15) / 16;
    ex.Yperm.assign(P4 * L, 0.0f);
    ex.Ymfma.assign(nct * L * 16, 0.0f);
    ex.sums.assign(P, 0.0f);
    std::vector<float> V(L);
    for (uint64_t j = 0; j < P; j++) {
        std::fill(V.begin(), V.end(), 0.0f);
        for (uint64_t i = 0; i < S; i++) V[i] = Y[j * S + i];
        ex.sums[j] = permute_and_sum(V, &ex.Yperm[j * L]);
        // MFMA layout (see score_mfma.hip): [ct][(((b*4+l)*2 + t/4)*64 + kk*16+n)*4 + t%4], s = 4t+kk
        const uint64_t ct = j / 16, n = j % 16;
        for (uint64_t b = 0; b < L / 128; b++)
            for (uint64_t l = 0; l < 4; l++)
                for (uint64_t sx = 0; sx < 32; sx++)
                {
                    // chain step sx = 4t + kk; lane = kk*16 + n; four consecutive t sit together
                    const uint64_t t = sx / 4, kk = sx % 4;
                    ex.Ymfma[ct * L * 16 + (((b * 4 + l) * 2 + t / 4) * 64 + kk * 16 + n) * 4 + t % 4] =
                        V[128 * b + 32 * l + 31 - sx];
                }
    }
    const uint64_t avail = sh.direct ? 2 * sh.W_f : 2 * W_m;
    while (ex.nb_full < W_m / 2 && 4ull * ex.nb_full + 3 < avail && ex.dmask[4 * ex.nb_full] == 0xFFFFFFFFu &&
           ex.dmask[4 * ex.nb_full + 1] == 0xFFFFFFFFu && ex.dmask[4 * ex.nb_full + 2] == 0xFFFFFFFFu &&
           ex.dmask[4 * ex.nb_full + 3] == 0xFFFFFFFFu)
        ex.nb_full++;
    return ex;
}

// ---- error bounds of the filters -------------------------------------------------------------------------------------------
// int8 slices per column: y_i ~ c + u*(254*q0_i + q1_i) (two slices, ~15 bits) or c + u*q0_i (one),
// centred at c = sum/N, sum being the reference's float32 sum of the column: then
//   r_c = N*yc - N1*sum = N*u*Dc + N1*(N*c - sum),   |N1*(N*c - sum)| <= rho  (rounding of c only),
// i.e. an exact integer Dc times a constant. For every row
//   |yigi_ref - yc| <= Eg + |sum_{i in row} resid_i| <= Eg + min(Rall, N1 * rmax):
//   Eg   = gamma_{L/4+3} * sum|y_i|  float32 summation error of the reference chains (Higham, recursive sums)
//   Rall = max(sum of the positive resid_i, sum of the |negative resid_i|)  (a row's residuals cannot
//          add up to more than all residuals of one sign), rmax = max_i |resid_i|,
//          resid_i = y_i - c - u*(254 q0_i + q1_i)
// so score_ref > thr needs (N*u*|Dc| + rho + N*E)^2 >= thr*d*(1 - 2^-40), i.e.
//   |Dc| >= sqrt(thr)*kalpha*sqrt(d) - eg - min(rall, N1*rmax)       (units of u; score_coarse.hip)
// with kalpha rounded down by 2^-19 relative and the error terms rounded up and padded: the device
// evaluates the right-hand side in float32, and these margins dominate its rounding. The block-scaled filter's bound is the
// same with its own unit u (see block_scaled_operands). The library builds with -ffp-contract=off: these expressions, in this
// order, are the exactness argument.
struct ErrBound {
    float eg, rall, rmax;     // phenotype units, rounded up
    float egD, rallD, rmaxD;  // the same in units of Dc (divided by u), rounded up: what the kernel uses
};

static double chain_gamma(uint64_t L) {  // gamma_{L/4+3}
    const double u32 = std::ldexp(1.0, -24);
    const double nterms = (double)L / 4.0 + 3.0;
    return nterms * u32 / (1.0 - nterms * u32);
}

static float up(double x) { return std::nextafter((float)x, std::numeric_limits<float>::infinity()); }

// The bound of one column of S samples (float32 sum `sum`, sum |y_i| = A) quantised with unit u, residuals rpos / rneg / rmax.
static void column_bound(uint64_t S, uint64_t L, double sum, double A, double u, double rpos, double rneg, double rmax,
                         CoarseCol& cc, ErrBound& eb) {
    const double Nd = (double)S;
    const double c = sum / Nd;
    const double rho = Nd * std::fabs(Nd * c - sum) * 2.0 + 1e-9 * (1.0 + std::fabs(sum));
    const double Eg = chain_gamma(L) * A * (1.0 + 1e-6) + 1e-12 * (1.0 + A);
    cc.kalpha = (1.0 - std::ldexp(1.0, -19)) / (Nd * u);
    cc.iu = up(1.0 / u * (1.0 + 1e-6));
    eb.eg = up((Eg + rho / Nd) * (1.0 + 1e-6) + 1e-30);
    eb.rall = up(std::max(rpos, rneg) * (1.0 + 1e-6));
    eb.rmax = up(rmax * (1.0 + 1e-6));
    const double iu = 1.0 / u * (1.0 + 1e-6);
    eb.egD = up((double)eb.eg * iu);
    eb.rallD = up((double)eb.rall * iu);
    eb.rmaxD = up((double)eb.rmax * iu);
}

// The narrow filter's bound, in double precision (its test is evaluated in double): column of S samples centred at c
// (float32 sum `sum`), max |y_i - c| = mx, sum |y_i| = A, residuals of the three slices rpos / rneg / rmax.
static void narrow_bound(uint64_t S, uint64_t L, double sum, double c, double mx, double A, double rpos, double rneg, double rmax,
                         NarrowCol& nc) {
    const double Nd = (double)S;
    // (the slice products u_k * v and the running residual are evaluated in double: pad by their rounding)
    const double fuzz = 64.0 * std::ldexp(1.0, -52) * (mx + std::fabs(c));
    nc.t1 = Nd * c - sum;
    nc.eg = (chain_gamma(L) * A * (1.0 + 1e-6) + 1e-12 * (1.0 + A)) * (1.0 + 1e-9);
    nc.rall = (std::max(rpos, rneg) + Nd * fuzz) * (1.0 + 1e-9);
    nc.rmax = (rmax + fuzz) * (1.0 + 1e-9);
    // both sides evaluate N * x - N1 * sum and the slice sums in double: absolute slack of a few ulps of
    // the largest intermediate (N * N * max|y|)
    nc.pad = 256.0 * std::ldexp(1.0, -52) * Nd * Nd * (mx + std::fabs(c) + 1.0) + 1e-300;
    // float32 pre-screen (score_narrow.hip): |r| <= N |ycf| (1 + 2^-10) + slackf: N1 |t1|, N E and the pad
    // of the exact test, and the float32 roundings of the three products and sums.
    const double slack = Nd * (nc.eg + std::min(nc.rall, Nd * nc.rmax)) + Nd * std::fabs(nc.t1) + nc.pad +
                         Nd * std::ldexp(1.0, -20) * mx * Nd;
    for (int k = 0; k < 3; k++) nc.wf[k] = (float)nc.w[k];
    nc.slackf = std::nextafter((float)(slack * 1.001), std::numeric_limits<float>::infinity());
}

// int8 slices of column y (S samples, float32 sum `sum`): q0 (and q1 with two slices), the column's constants and bound;
// resid (or null): y_i - c - what the slices encode
static void quantise_int8(const float* y, uint64_t S, uint64_t L, double sum, int ns, int* q0, int* q1, double* resid,
                          CoarseCol& cc, ErrBound& eb) {
    const double c = sum / (double)S;
    double mx = 0, A = 0;
    for (uint64_t i = 0; i < S; i++) {
        mx = std::max(mx, std::fabs((double)y[i] - c));
        A += std::fabs((double)y[i]);
    }
    // unit u: one slice spans +-127 u, two slices +-(127*254 + 127) u
    const double u = mx > 0 ? (ns == 2 ? mx / (127.0 * 254.0) : mx / 127.0) : 1.0;
    const double a0 = ns == 2 ? 254.0 * u : u;
    double rpos = 0, rneg = 0, rmax = 0;
    for (uint64_t i = 0; i < S; i++) {
        const double yc = (double)y[i] - c;
        int v0 = (int)std::lrint(yc / a0);
        v0 = std::max(-127, std::min(127, v0));
        double r = yc - a0 * v0;
        int v1 = 0;
        if (ns == 2) {
            v1 = (int)std::lrint(r / u);
            v1 = std::max(-127, std::min(127, v1));
            r -= u * v1;
        }
        q0[i] = v0;
        q1[i] = v1;
        if (resid) resid[i] = r;
        if (r > 0) rpos += r; else rneg -= r;
        rmax = std::max(rmax, std::fabs(r));
    }
    column_bound(S, L, sum, A, u, rpos, rneg, rmax, cc, eb);
}

// ---- the plan --------------------------------------------------------------------------------------------------------------

static uint64_t tiles_for(uint64_t cols) { return (cols + 1 + 15) / 16; }  // 16-column tiles of `cols` columns + a ones column

// LDS groups of at most tmax column tiles that hold P columns (~0: none, tmax = 0)
static uint64_t groups_for(uint64_t P, uint32_t tmax) {
    uint64_t g = 1;
    while (tmax && tiles_for((P + g - 1) / g) > tmax) g++;
    return tmax ? g : ~0ull;
}

// Largest number of column tiles whose block-scaled operands stay resident in one LDS group (0: not even one)
static uint32_t resident_tiles(uint32_t n_steps, uint32_t ns, uint32_t s1_fp6) {
    for (uint32_t ct = 7; ct >= 1; ct--)
        if (mx_lds_bytes(n_steps, ct, ns, s1_fp6) <= 160u * 1024u) return ct;
    return 0u;
}

// Does the two-slice block-scaled set stream its operands (score_mxs.hip) instead of keeping them resident with at most ct
// column tiles per LDS group? KGWAS_MXS: see plan_scan.
static bool streams(const FilterOpts& o, bool mxs_can, uint64_t P, uint32_t ct) {
    return mxs_can && (o.mxs >= 3 || !ct || (groups_for(P, ct) >= 2 && (o.mxs >= 2 || ct <= 2)));
}

// LDS groups: as few as hold all columns (+ a ones column each) - the balanced split, which pads every group (201 columns,
// 4 tiles per group: 4 x (51 + ones) of 4 x 64 slots = 16 tiles for 13 tiles' worth of columns). Alternative: groups filled to
// the last slot and ONE smaller launch for the rest - taken when it multiplies fewer tiles, with no more row passes, by more
// than `premium` tiles. tmax: column tiles per group; ns: operand tiles per column tile (int8: one per slice).
static std::vector<FilterPart> split_parts(uint64_t P, uint32_t ns, uint32_t tmax, double premium, bool split) {
    const uint64_t groups = groups_for(P, tmax), cper = (P + groups - 1) / groups;
    const uint32_t T = ns * (uint32_t)tiles_for(cper);
    std::vector<FilterPart> parts{FilterPart{0, P, cper, T, groups}};
    const uint64_t cpf = (uint64_t)tmax * 16 - 1;  // columns of a full group
    const uint64_t full = P / cpf, rem = P - full * cpf;
    const uint64_t Tr = rem ? ns * tiles_for(rem) : 0;
    if (groups > 1 && split && full >= 1 && full + (rem ? 1 : 0) <= groups &&
        (double)(full * ns * tmax + Tr) + premium < (double)(groups * T)) {
        parts = {FilterPart{0, full * cpf, cpf, ns * tmax, full}};
        if (rem) parts.push_back(FilterPart{full * cpf, rem, rem, (uint32_t)Tr, 1});
    }
    return parts;
}

// An int8 set (score_coarse.hip) of ns slices. Operand columns ("slots") per LDS group: the group's share of the phenotype
// columns, padding, and the ones column in the last slot (its dot product is the row's masked popcount N1).
static FilterSet plan_int8(uint64_t P, int ns, uint32_t coarse_T, const FilterOpts& o) {
    FilterSet fs;
    fs.slices = (uint32_t)ns;
    const uint32_t Tmax = ns == 2 ? coarse_T & ~1u : coarse_T;  // largest tile count whose operands fit the LDS
    fs.parts = split_parts(P, (uint32_t)ns, Tmax / (uint32_t)ns, 0.0, o.split);
    for (const FilterPart& fp : fs.parts) fs.tile_slices += fp.T * (uint32_t)fp.groups;
    return fs;
}

// A block-scaled set (score_mx.hip, score_mxs.hip) of ns slices
static FilterSet plan_block_scaled(uint64_t S, uint64_t P, int ns, uint32_t n_kgroups, bool mxs_can, const FilterOpts& o) {
    FilterSet fs;
    fs.mx = true;
    fs.slices = (uint32_t)ns;
    // whole 512-sample groups (the kernel reads all 64 bytes of those without a bounds check) + up to four quarter groups
    fs.n_full = (uint32_t)(S / 512);
    fs.n_quarter = (uint32_t)((S % 512 + 127) / 128);
    fs.n_steps = 4 * fs.n_full + fs.n_quarter;
    // Second slice: FP4. An FP6 one (1.1 survivors per candidate instead of 1.4) costs LDS, a slower MFMA (8.25
    // against 9.5 POP/s) and two more operand registers per tile: measured at 1135 x 101, the same 2 x 4 tiles,
    // filter 14.4 against 13.6 ms per 100 M rows and all kernels 18.3 against 17.8. KGWAS_MX_S1=6 selects it
    // (tests keep that kernel form covered).
    fs.s1_fp6 = ns == 2 && o.mx_s1_fp6 && resident_tiles(fs.n_steps, 2, 1) ? 1u : 0u;
    const uint32_t CTmax = resident_tiles(fs.n_steps, (uint32_t)ns, fs.s1_fp6);
    // Operand-streaming form (score_mxs.hip): every row is loaded and expanded ONCE per operand group of up to 14 column
    // tiles, whatever the number of accessions; taken where the resident plan would pass every row through several LDS
    // groups. Up to 7 tiles (111 columns + the ones column): one column group, eight waves of 64 rows each. Beyond: TWO
    // column groups of up to 7 tiles per block (222 columns), the waves w and w + 4 working on the same 64 rows - each
    // group with its own ones column - and as many such operand groups (grid blocks sharing rows) as the columns need.
    // KGWAS_MXS_FORM=1 / 2: one column group of up to 13 tiles, eight waves of 32 rows / four waves of 64 rows.
    if (mxs_can && ns == 2 && !fs.s1_fp6 && streams(o, mxs_can, P, CTmax)) {
        uint64_t g = 1, ng = 1, ct = 0;
        uint32_t form = 0;
        if (P + 1 <= 7 * 16) {
            ct = std::max<uint64_t>(3, tiles_for(P));
        } else if (o.mxs_form == 1 || o.mxs_form == 2) {
            while (tiles_for((P + g - 1) / g) > 13) g++;
            ct = tiles_for((P + g - 1) / g);
            if (ct > 7) form = (uint32_t)o.mxs_form;
        } else {
            ng = 2;
            g = 2;
            while (tiles_for((P + g - 1) / g) > 7) g += 2;
            ct = std::max<uint64_t>(4, tiles_for((P + g - 1) / g));
        }
        if (mxs_supported((uint32_t)ct, (uint32_t)ng, 2, 0) && mxs_lds_bytes((uint32_t)ct, (uint32_t)ng) <= 160u * 1024u)
            fs.parts = {FilterPart{0, P, (P + g - 1) / g, (uint32_t)ct, g, 1u + form, (uint32_t)ng}};
    }
    if (!CTmax && fs.parts.empty()) throw Error(KGWAS_ERR_ARG, "coarse filter: too many accessions for the LDS");
    // (a second launch for the rest is worth two and a half tiles of its own: its few column tiles multiply at
    // a fraction of the full groups' efficiency. 1135 x 101: 2 x 4 tiles in one launch 13.6 ms per 100 M rows,
    // 6 + 1 tiles in two 16.3; 2048 x 201: 5 x 3 tiles in one launch 39.2, 4 x 3 + 1 in two 40.2)
    const bool streamed = !fs.parts.empty();
    if (!streamed) fs.parts = split_parts(P, 1, CTmax, 2.5, o.split);
    for (const FilterPart& fp : fs.parts) fs.tile_slices += fp.T * (uint32_t)ns * (uint32_t)fp.groups;
    // the set's matrix work per row in int8 tile-slice equivalents (a K = 128 step is one of the 8 n_kgroups K = 64
    // steps' worth of two; measured 30 % less efficient per MFMA with three column tiles per LDS group: 0.48 against 0.37 ms per M rows at 2048 x 201)
    fs.tile_slices_eq = (double)fs.tile_slices * (double)fs.n_steps / (8.0 * (double)n_kgroups) * ((CTmax <= 3 && !streamed) ? 1.30 : 1.0);
    return fs;
}

ScanPlan plan_scan(const kgwas_scan_params& p, const ScanShape& sh, const FilterOpts& o, const std::vector<float>& Y,
                   std::vector<double> resid[3]) {
    const uint64_t S = sh.S, P = sh.P;
    ScanPlan pl;
    uint32_t kern = p.kernel;
    const bool mfma_fits = mfma_lds_bytes((uint32_t)sh.W_m) <= 160u * 1024u;
    // Coarse int8 filter + exact re-scoring for the sparse phase (score_coarse.hip): needs finite values,
    // an exact kernel for the dense phase / re-runs, and T >= 2 int8 tiles of the whole sample axis in LDS.
    pl.n_kgroups = (uint32_t)((sh.W_m + 7) / 8);
    uint32_t coarse_T = 0;  // most int8 operand tiles the LDS can hold
    for (uint32_t T : {8u, 7u, 6u, 5u, 4u, 3u, 2u})
        if (coarse_lds_bytes(pl.n_kgroups, T) <= 152u * 1024u) {
            coarse_T = T;
            break;
        }
    // The operand-streaming form of the block-scaled filter (score_mxs.hip) holds one step's operands in LDS, not a whole
    // column tile's: no limit on the accessions. KGWAS_MXS: 0 never; 1 (default) where the resident form does not exist
    // (no column tile's operands fit the LDS) or would pass every row through several LDS groups of ONE or TWO column
    // tiles (its matrix instructions run at a fraction of a full group's efficiency there); 2 wherever the resident form
    // needs more than one LDS group - measured level with it, not ahead: 2048 x 201 40.4-41.0 against 39.2-40.3 ms per
    // 100 M rows, 1135 x 101 13.3 against 13.4 -; 3 wherever the form exists. The int8 filter
    // (KGWAS_COARSE_MX=0) stops at 5120 accessions.
    const bool mxs_can = o.mxs != 0 && o.coarse_mx != 0 && o.coarse_slices < 0 && !o.mx_s1_fp6;
    const bool filter_fits = coarse_T != 0 || mxs_can;
    if (kern == KGWAS_KERNEL_COARSE) {
        if (!sh.chain_safe || !filter_fits)
            throw Error(KGWAS_ERR_ARG, "coarse filter needs finite phenotype values whose float32 sums cannot overflow (sum |y| < FLT_MAX per column) and, for its int8 form, <= 5120 accessions");
        pl.coarse = true;
        kern = KGWAS_KERNEL_AUTO;
    } else if (kern == KGWAS_KERNEL_AUTO && sh.chain_safe && filter_fits) {
        // any number of columns: even a single column (one mostly empty 16-column tile) runs twice as fast behind
        // the filter as through the exact VALU scorer (12.5 vs 27 ms per 100 M-row pass)
        pl.coarse = true;
    }
    if (kern == KGWAS_KERNEL_AUTO) kern = (P >= 4 && sh.finite && mfma_fits) ? KGWAS_KERNEL_MFMA : KGWAS_KERNEL_VALU;
    if (kern == KGWAS_KERNEL_MFMA && !mfma_fits)
        throw Error(KGWAS_ERR_ARG, "MFMA scorer: phenotype tile does not fit LDS for this many accessions");
    if (kern == KGWAS_KERNEL_MFMA && !sh.finite)
        throw Error(KGWAS_ERR_ARG, "MFMA scorer needs finite phenotype values (0*inf); use the VALU scorer");
    if (kern != KGWAS_KERNEL_MFMA && kern != KGWAS_KERNEL_VALU) throw Error(KGWAS_ERR_ARG, "unknown kernel id");
    pl.kernel = kern;
    // One to four columns under AUTO: the narrow filter (FP4 x FP8 block-scaled MFMA, three slices per column)
    // instead of the int8 one, whose 16-column tiles would be mostly padding (KGWAS_NARROW=0: keep the int8 filter).
    pl.narrow = pl.coarse && p.kernel == KGWAS_KERNEL_AUTO && P <= NARROW_MAX_COLS &&
                narrow_lds_bytes(pl.n_kgroups) <= 64u * 1024u && o.narrow;

    // (narrow filter on rows read in place: chunks of up to 128 M rows - with one column a chunk's fixed costs, five
    // launches and a copy with the gaps between them, ~40 us, weigh more than the candidates a staler threshold lets
    // through. 1.2 G rows x 1024 samples, one column: cap 32 M rows 49 chunks 30.8 ms, 64 M 33 / 30.0, 128 M 25 / 29.8,
    // 256 M 21 / 29.7 - identical heaps, tools/p1_large_chunks.py)
    pl.chunk_max = p.chunk_rows ? p.chunk_rows : ((pl.narrow && sh.direct) ? (128ull << 20) : (8ull << 20));
    pl.chunk_max = std::max<uint64_t>(128, (pl.chunk_max + 127) / 128 * 128);
    if (pl.coarse) {  // survivor keys are (column << row_bits | row) in 32 bits, the 0xFFFFFFFF fill included
        uint32_t pbits = 1;
        while ((1ull << pbits) < P + 1) pbits++;
        if (pbits > 22) throw Error(KGWAS_ERR_ARG, "coarse filter: too many phenotype columns for 32-bit survivor keys");
        pl.chunk_max = std::max<uint64_t>(128, std::min<uint64_t>(pl.chunk_max, 1ull << (32 - pbits)));
    }
    if (pl.coarse && !pl.narrow) {  // the coarse kernel addresses a chunk's rows with 32-bit byte offsets
        const uint64_t stride_dw = 2 * (1 + std::max<uint64_t>(sh.W_f, sh.W_m));
        const uint64_t lim = ((1ull << 32) - (1ull << 20)) / (4 * stride_dw) / 128 * 128;
        pl.chunk_max = std::max<uint64_t>(128, std::min<uint64_t>(pl.chunk_max, lim));
    }
    pl.dense_rows = std::min<uint64_t>(16384, pl.chunk_max);
    // Dense chunks of a feed: enough rows to fill the largest heap with a margin for the MAC filter (more
    // dense chunks follow while a heap is still short); everything after goes through the sparse path.
    pl.dense_chunk = std::min<uint64_t>(pl.dense_rows, std::max<uint64_t>(1024, (sh.max_topn + sh.max_topn / 8 + 512 + 127) / 128 * 128));
    // candidate records per slot (few columns: longer lists, so that the ramp takes ~6 chunks instead of ~13 - a chunk's
    // fixed costs, not its rows, are what a one-column scan pays for)
    const uint64_t budget = (uint64_t)o.cap_budget;
    const uint64_t cap_mult = (uint64_t)(o.cap_mult >= 0 ? o.cap_mult : (pl.narrow ? 16 : 2));
    const uint64_t cap = std::min<uint64_t>(cap_mult * sh.max_topn + 4096, std::max<uint64_t>(budget / P, 1024));
    pl.cap = (uint32_t)std::min<uint64_t>(cap, 0x7FFFFFFFull);
    if (!pl.coarse) return pl;

    // test hook (kgwas_scan_debug_residuals): keep every filter form's quantisation residuals, so that a test can build the
    // rows on which the bound |yigi_ref - yc| <= Eg + min(Rall, N1 * rmax) is TIGHT (tests/test_gpu_parity.py, adversarial bound)
    pl.keep_resid = o.debug_residuals;
    // test hook (kgwas_scan_debug_survivors): log every filtered chunk's thresholds and survivors (scan_gpu.cpp, submit_sparse)
    pl.keep_surv = o.debug_survivors;
    if (pl.keep_resid)
        for (int f = 0; f < 3; f++) resid[f].assign(P * S, 0.0);
    // One slice halves the matrix work but widens the bound; it is offered when, for every column, the bound
    // at N1 = S/2 stays below 15 % of the deviation of yigi a z = 4 association needs (2*sigma*sqrt(S)), so the
    // survivors stay within a small multiple of the true candidates. KGWAS_COARSE_SLICES=1|2 forces one set.
    // (the columns' float32 sums as exact_layouts makes them: the plan comes first, so that its errors precede any allocation)
    std::vector<float> V(sh.L), R(sh.L);
    std::vector<int> q0(S), q1(S);
    bool one_ok = true;
    for (uint64_t j = 0; j < P && one_ok; j++) {
        const float* y = &Y[j * S];
        std::fill(V.begin(), V.end(), 0.0f);
        std::copy(y, y + S, V.begin());
        CoarseCol cc;
        ErrBound eb;
        quantise_int8(y, S, sh.L, (double)permute_and_sum(V, R.data()), 1, q0.data(), q1.data(),
                      pl.keep_resid ? &resid[0][j * S] : nullptr, cc, eb);
        double mean = 0, var = 0;
        for (uint64_t i = 0; i < S; i++) mean += (double)y[i];
        mean /= (double)S;
        for (uint64_t i = 0; i < S; i++) var += ((double)y[i] - mean) * ((double)y[i] - mean);
        const double sigma = std::sqrt(var / (double)S);
        const double e_half = (double)eb.eg + std::min((double)eb.rall, 0.5 * (double)S * (double)eb.rmax);
        if (!(e_half <= 0.15 * 2.0 * sigma * std::sqrt((double)S))) one_ok = false;
    }
    if (pl.narrow) {  // the int8 operand sets are not needed
        pl.narrow_pack1 = P == 1 && o.narrow_pack;
        return pl;
    }
    bool want[2] = {one_ok, true};
    if (o.coarse_slices == 1) want[0] = true, want[1] = false;
    if (o.coarse_slices == 2) want[0] = false, want[1] = true;
    // ---- block-scaled filter (score_mx.hip), the default: FP6 (+ FP4 / FP6) slices on the integer grids (see
    // block_scaled_operands). Which filter (KGWAS_COARSE_MX=1|0 forces one): the block-scaled one unless its operands (1.25
    // bytes per sample and column with two slices) make a row pass through more than ONE more LDS group than the int8
    // filter's single slice (1 byte) does - every row is loaded, expanded and tested once per group. Measured, all kernels per
    // 100 M rows: 1024 x 101 (one group each) 14.2 ms against 15.2; 1135 x 101 (two each) 17.6 against 21.1; 2048 x 201
    // (five equal groups of three column tiles in one launch against four groups of four int8 tiles + the two-slice
    // ramp) 50.1 against 52.2 (51.5 with the int8 one-slice set + a block-scaled ramp, the arrangement beyond).
    if (o.coarse_mx >= 0) {
        pl.use_mx = o.coarse_mx == 1;
    } else {
        const uint32_t ctm = resident_tiles(4u * (uint32_t)(S / 512) + (uint32_t)((S % 512 + 127) / 128), 2, 0);
        // (streamed operands are one group whatever the shape; beyond 5120 accessions there is no int8 plan to compare
        // with: coarse_T = 0)
        pl.use_mx = streams(o, mxs_can, P, ctm) || !coarse_T || groups_for(P, ctm) <= groups_for(P, coarse_T) + 1;
    }
    // Where the int8 filter keeps the shape, its TWO-slice set (the ramp: the first chunks of a scan, many
    // candidates per row) is still the block-scaled one: at 2048 x 201 that is 13 column tiles x 2 slices x 16
    // K = 128 steps against 28 int8 tile-slices x 32 K = 64 steps - about half the matrix work per row for the same
    // ~1 survivor per candidate - and the chunks stay on it longer before the one-slice int8 set takes over
    // (pick_coarse_mode prices both sets in int8 tile-slice equivalents).
    const bool mixed = !pl.use_mx && o.coarse_mx < 0 && o.coarse_slices < 0 && want[0] && want[1] && o.mixed;
    if (pl.use_mx && o.coarse_slices < 0) want[0] = false;  // one FP6 slice alone: only on request
    for (int mi = 0; mi < 2; mi++)
        if (want[mi])
            pl.set[mi] = (pl.use_mx || (mixed && mi == 1)) ? plan_block_scaled(S, P, mi + 1, pl.n_kgroups, mxs_can, o)
                                                           : plan_int8(P, mi + 1, coarse_T, o);
    return pl;
}

// ---- operands of the filters -----------------------------------------------------------------------------------------------

NarrowOperands narrow_operands(const ScanShape& sh, const ScanPlan& pl, const std::vector<float>& Y, const std::vector<float>& sums,
                               double* resid) {
    const uint64_t S = sh.S, P = sh.P, n_kgroups = pl.n_kgroups;
    // FP8 E4M3 operands of the narrow filter (score_narrow.hip): three slices of integers in [-15, 15] per
    // column, y_i - c ~ sum_k u_k q_ki with u_0 = max|y_i - c| / 15 and u_{k+1} = u_k / 30 (a rounding
    // residual of at most u_k / 2 fills the next slice's range exactly), and a ones row per column.
    auto e4m3 = [](int v) -> uint8_t {
        if (v == 0) return 0;
        const int sg = v < 0 ? 0x80 : 0, av = std::abs(v);
        int e = 0;
        while ((2 << e) <= av) e++;
        return (uint8_t)(sg | ((e + 7) << 3) | ((av * 8) / (1 << e) - 8));
    };
    const uint64_t n_steps = 4ull * n_kgroups;
    NarrowOperands op;
    op.Bn.assign(n_steps * 64 * 32, 0);
    op.ncols.resize(P);
    std::vector<int> q(S);
    auto put_slot = [&](uint64_t slot, const std::vector<int>& v) {
        for (uint64_t g = 0; g < n_kgroups; g++)
            for (uint64_t jj = 0; jj < 4; jj++)
                for (uint64_t k = 0; k < 128; k++) {
                    // FP4 side: k = 32 kb + 8 q + e' <-> bit 4 e' + jj of dword q of the lane's 16 bytes
                    const uint64_t kbA = k / 32, e = k % 32, smp = 512 * g + 128 * kbA + 32 * (e / 8) + 4 * (e % 8) + jj;
                    if (smp >= S) continue;
                    // FP8 side: lane kb = (k % 64) / 16, byte (k / 64) * 16 + k % 16
                    const uint64_t lane = slot + 16 * ((k % 64) / 16), byte = (k / 64) * 16 + k % 16;
                    op.Bn[((g * 4 + jj) * 64 + lane) * 32 + byte] = e4m3(v[smp]);
                }
    };
    for (uint64_t j = 0; j < P; j++) {
        const double Nd = (double)S, sum = (double)sums[j];
        const double c = sum / Nd;
        double mx = 0, A = 0;
        std::vector<double> t(S);
        for (uint64_t i = 0; i < S; i++) {
            t[i] = (double)Y[j * S + i] - c;
            mx = std::max(mx, std::fabs(t[i]));
            A += std::fabs((double)Y[j * S + i]);
        }
        double u = mx > 0 ? mx / 15.0 : 1.0;
        NarrowCol& nc = op.ncols[j];
        for (int k = 0; k < NARROW_SLICES; k++) {
            for (uint64_t i = 0; i < S; i++) {
                int v = (int)std::lrint(t[i] / u);
                v = std::max(-15, std::min(15, v));
                q[i] = v;
                t[i] -= u * v;
            }
            put_slot(4 * j + k, q);  // operand row 4 p + k; 4 p + 3 = ones
            if (pl.narrow_pack1)    // (one column: the same rows in the other three column slots, kernels.h NarrowArgs::pack1)
                for (uint64_t t = 1; t < 4; t++) put_slot(4 * t + k, q);
            nc.w[k] = 2.0 * u;
            u /= 30.0;
        }
        double rpos = 0, rneg = 0, rmax = 0;
        for (uint64_t i = 0; i < S; i++) {
            if (resid) resid[j * S + i] = t[i];
            if (t[i] > 0) rpos += t[i]; else rneg -= t[i];
            rmax = std::max(rmax, std::fabs(t[i]));
        }
        narrow_bound(S, sh.L, sum, c, mx, A, rpos, rneg, rmax, nc);
    }
    for (uint64_t j = 0; j < (pl.narrow_pack1 ? 4 : P); j++) put_slot(4 * j + 3, std::vector<int>(S, 1));
    return op;
}

static PartOperands empty_part(const FilterPart& fp, size_t Bq_bytes, uint64_t slots) {
    PartOperands op;
    op.Bq.assign(Bq_bytes, 0);
    op.cols.resize(fp.groups * slots);
    for (auto& cc : op.cols) {
        memset(&cc, 0, sizeof(cc));
        cc.pheno = -1;
    }
    return op;
}

static void fold_bound(PartOperands& op, const ErrBound& eb) {
    op.eg_max = std::max(op.eg_max, eb.egD);
    op.rall_max = std::max(op.rall_max, eb.rallD);
    op.rmax_max = std::max(op.rmax_max, eb.rmaxD);
}

PartOperands int8_operands(const ScanShape& sh, uint32_t n_kgroups, const FilterSet& fs, const FilterPart& fp, const std::vector<float>& Y,
                           const std::vector<float>& sums, double* resid) {
    const uint64_t S = sh.S;
    const int ns = (int)fs.slices;
    const uint32_t Tp = fp.T, PG = Tp / (uint32_t)ns, slots = PG * 16;
    PartOperands op = empty_part(fp, fp.groups * n_kgroups * 8ull * Tp * 1024ull, slots);
    auto put = [&](uint64_t lg, uint64_t slot, const std::vector<int>& v0, const std::vector<int>& v1) {
        const uint64_t pgl = slot / 16, n = slot % 16;
        for (uint64_t g = 0; g < n_kgroups; g++)
            for (uint64_t jj = 0; jj < 8; jj++)
                for (uint64_t kg = 0; kg < 4; kg++)
                    for (uint64_t e = 0; e < 16; e++) {
                        // k-element e of step jj <-> sample (score_coarse.hip: expand_step)
                        const uint64_t smp = 512 * g + 128 * kg + 32 * (e / 4) + 8 * (e % 4) + jj;
                        if (smp >= S) continue;
                        const uint64_t lane = kg * 16 + n;
                        const uint64_t base = (((lg * n_kgroups + g) * 8 + jj) * Tp);
                        if (ns == 1) {
                            op.Bq[((base + pgl) * 64 + lane) * 16 + e] = (uint8_t)v0[smp];
                        } else {
                            op.Bq[((base + 2 * pgl) * 64 + lane) * 16 + e] = (uint8_t)v0[smp];
                            op.Bq[((base + 2 * pgl + 1) * 64 + lane) * 16 + e] = (uint8_t)v1[smp];
                        }
                    }
    };
    std::vector<int> q0(S), q1(S);
    for (uint64_t j = fp.j0; j < fp.j0 + fp.n; j++) {
        const uint64_t lg = (j - fp.j0) / fp.cper, slot = (j - fp.j0) % fp.cper;
        CoarseCol& cc = op.cols[lg * slots + slot];
        ErrBound eb;
        quantise_int8(&Y[j * S], S, sh.L, (double)sums[j], ns, q0.data(), q1.data(), resid ? resid + j * S : nullptr, cc, eb);
        fold_bound(op, eb);
        cc.pheno = (int32_t)j;
        put(lg, slot, q0, q1);
    }
    {  // ones column: Dc = N1 (one slice: q0 = 1; two slices: Dc = 254*D0 + D1 with q0 = 0, q1 = 1)
        std::vector<int> ones(S, 1), zeros(S, 0);
        for (uint64_t lg = 0; lg < fp.groups; lg++) put(lg, slots - 1, ns == 1 ? ones : zeros, ones);
    }
    return op;
}

// FP6 (+ FP4 / FP6) slices on the integer grids
//   A6 = {0..15, 16..30 step 2, 32..60 step 4} (E2M3 x 8),  A4 = {0, 1, 2, 3, 4, 6, 8, 12} (E2M1 x 2):
//   y_i - c ~ w * t_i,  t_i = a6_i (one slice), 8 a6_i + a4_i (FP4 second slice) or 32 a6_i + a6'_i (FP6 second
//   slice); the accumulator is kappa * sum_i g_i t_i, kappa = 1/16, 1/4, 1/16, so one accumulator unit is
//   u = w / kappa phenotype units and the int8 filter's bound (column_bound: kalpha, the error terms in units of Dc)
//   carries over with that u. The ones column has t = 1 / kappa: its accumulator is N1.
PartOperands block_scaled_operands(const ScanShape& sh, const FilterSet& fs, const FilterPart& fp, const std::vector<float>& Y,
                                   const std::vector<float>& sums, double* resid) {
    const uint64_t S = sh.S;
    const int ns = (int)fs.slices;
    const uint32_t s1_fp6 = fs.s1_fp6, n_full = fs.n_full, n_steps = fs.n_steps;
    std::vector<int> G6, G4;  // the signed grids, ascending
    for (int q = 60; q >= 32; q -= 4) G6.push_back(-q);
    for (int q = 30; q >= 16; q -= 2) G6.push_back(-q);
    for (int q = 15; q >= -15; q--) G6.push_back(-q);
    for (int q = 16; q <= 30; q += 2) G6.push_back(q);
    for (int q = 32; q <= 60; q += 4) G6.push_back(q);
    for (int h : {-12, -8, -6, -4, -3, -2, -1, 0, 1, 2, 3, 4, 6, 8, 12}) G4.push_back(h);
    auto nearest = [](const std::vector<int>& g, double v) {  // index of the grid value closest to v
        size_t hi = std::lower_bound(g.begin(), g.end(), v, [](int a, double b) { return (double)a < b; }) - g.begin();
        if (hi == 0) return (size_t)0;
        if (hi == g.size()) return g.size() - 1;
        return (v - (double)g[hi - 1] <= (double)g[hi] - v) ? hi - 1 : hi;
    };
    auto e2m3 = [](int q) -> uint32_t {  // E2M3 code of q / 8
        const uint32_t sg = q < 0 ? 0x20u : 0u;
        const int a = std::abs(q);
        if (a < 8) return sg | (uint32_t)a;
        int e = 1, base = 8;
        while (a >= 2 * base) base *= 2, e++;
        return sg | ((uint32_t)e << 3) | (uint32_t)((a - base) / (base / 8));
    };
    auto e2m1 = [](int h) -> uint32_t {  // E2M1 code of h / 2
        static const int tab[8] = {0, 1, 2, 3, 4, 6, 8, 12};
        uint32_t i = 0;
        while (tab[i] != std::abs(h)) i++;
        return (h < 0 ? 8u : 0u) | i;
    };
    const int sh1 = ns == 1 ? 0 : (s1_fp6 ? 5 : 3);                // t = 2^sh1 * a6 + a1
    const double kappa = (ns == 2 && !s1_fp6) ? 0.25 : 0.0625;     // accumulator = kappa * sum g t
    const int t_ones = (int)(1.0 / kappa);                         // in the LAST slice (a6 = 0 with two slices)
    const double t_max = ns == 1 ? 60.0 : (s1_fp6 ? 32.0 * 60.0 + 60.0 : 8.0 * 60.0 + 12.0);
    const std::vector<int>& G1 = s1_fp6 ? G6 : G4;
    auto quantise_mx = [&](uint64_t j, CoarseCol& cc, ErrBound& eb, std::vector<int>& a0, std::vector<int>& a1) {
        const double Nd = (double)S, sum = (double)sums[j];
        const double c = sum / Nd;
        double mx = 0, A = 0;
        for (uint64_t i = 0; i < S; i++) {
            const double y = (double)Y[j * S + i];
            mx = std::max(mx, std::fabs(y - c));
            A += std::fabs(y);
        }
        const double w = mx > 0 ? mx / t_max : 1.0;
        const double u = w / kappa;  // one accumulator unit in phenotype units
        double rpos = 0, rneg = 0, rmax = 0;
        for (uint64_t i = 0; i < S; i++) {
            const double y = (double)Y[j * S + i] - c;
            const double x = y / w;
            int b0 = 0, b1 = 0;
            if (ns == 1) {
                b0 = G6[nearest(G6, x)];
            } else {
                // the first slice's neighbours of x / 2^sh1, each with its best second slice
                const double sc = (double)(1 << sh1);
                const size_t k0 = nearest(G6, x / sc);
                double best = 1e300;
                for (size_t k = k0 ? k0 - 1 : 0; k <= std::min(k0 + 1, G6.size() - 1); k++) {
                    const int c1 = G1[nearest(G1, x - sc * G6[k])];
                    const double r = std::fabs(x - sc * G6[k] - c1);
                    if (r < best) best = r, b0 = G6[k], b1 = c1;
                }
            }
            a0[i] = b0;
            a1[i] = b1;
            const double r = y - w * ((double)(1 << sh1) * b0 + b1);
            if (resid) resid[j * S + i] = r;
            if (r > 0) rpos += r; else rneg -= r;
            rmax = std::max(rmax, std::fabs(r));
        }
        column_bound(S, sh.L, sum, A, u, rpos, rneg, rmax, cc, eb);
    };
    const uint32_t CT = fp.T, slots = CT * 16;
    const uint64_t NGs = fp.ng;  // column groups per block (streaming form; else 1)
    const uint32_t SB = mx_step_bytes((uint32_t)ns, s1_fp6);
    const size_t group_bytes = (size_t)n_steps * CT * SB;
    // (the streaming form's last transfer of a slab reads up to 1 KB past it)
    PartOperands op = empty_part(fp, fp.groups * group_bytes + 1024, slots);
    // the slice values of operand column `slot` of LDS group lg: v0 on the A6 grid, v1 on the second slice's
    auto put = [&](uint64_t lg, uint64_t slot, const std::vector<int>& v0, const std::vector<int>& v1) {
        const uint64_t t = slot / 16, n = slot % 16;
        for (uint64_t st = 0; st < n_steps; st++) {
            // (streaming form: the NG column groups of a block lie side by side within a step's slab)
            uint8_t* blk = &op.Bq[(lg / NGs) * (NGs * group_bytes) + ((st * NGs + lg % NGs) * CT + t) * SB];
            for (uint64_t kb = 0; kb < 4; kb++) {
                const uint64_t lane = kb * 16 + n;
                for (uint64_t e = 0; e < 32; e++) {
                    // score_mx.hip: k = 32 kb + e <-> sample
                    const uint64_t smp = st < 4ull * n_full ? 512 * (st / 4) + 128 * kb + 32 * (e / 8) + 4 * (e % 8) + st % 4
                                                            : 512ull * n_full + 128 * (st - 4ull * n_full) + 32 * kb + 4 * (e % 8) + e / 8;
                    if (smp >= S) continue;
                    auto put6 = [&](uint8_t* part, int q) {  // 6-bit field e of the lane's 6 dwords: dwords 0-3 | 4-5
                        const uint32_t code = e2m3(q);
                        for (int b = 0; b < 6; b++)
                            if (code & (1u << b)) {
                                const uint64_t bit = 6 * e + b, dw = bit / 32;
                                uint8_t* d = dw < 4 ? part + lane * 16 + dw * 4 : part + 1024 + lane * 8 + (dw - 4) * 4;
                                d[(bit % 32) / 8] |= (uint8_t)(1u << (bit % 8));
                            }
                    };
                    put6(blk, v0[smp]);
                    if (ns == 2) {
                        if (s1_fp6)
                            put6(blk + 1536, v1[smp]);
                        else
                            blk[1536 + lane * 16 + e / 2] |= (uint8_t)(e2m1(v1[smp]) << (4 * (e % 2)));
                    }
                }
            }
        }
    };
    // The columns on a few threads (quantising and packing 101 columns of 1135 samples took 35 ms of a session's
    // creation - a tenth of a whole `associate_kmers` run on a 6 GB table): a column's operand bytes are its own
    // (lane kb * 16 + slot % 16 of tile slot / 16), as are its constants; the bounds are folded afterwards.
    {
        std::vector<ErrBound> ebs(fp.n);
        const unsigned nt = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(usable_cpus(), 16), fp.n / 4));
        std::atomic<uint64_t> next(0);
        kgwas_run_on_threads(nt, "kgwas-quant", [&] {
            std::vector<int> b0(S), b1(S);
            try {
                for (uint64_t i; (i = next.fetch_add(1, std::memory_order_relaxed)) < fp.n;) {
                    const uint64_t j = fp.j0 + i, lg = i / fp.cper, slot = i % fp.cper;
                    CoarseCol& cc = op.cols[lg * slots + slot];
                    quantise_mx(j, cc, ebs[i], b0, b1);
                    cc.pheno = (int32_t)j;
                    put(lg, slot, b0, b1);
                }
            } catch (...) {
                next.store(fp.n);  // (the other threads stop at their next column)
                throw;
            }
        });
        for (const ErrBound& eb : ebs) fold_bound(op, eb);
    }
    {  // ones column: accumulator = N1
        std::vector<int> ones(S, t_ones), zeros(S, 0);
        for (uint64_t lg = 0; lg < fp.groups; lg++) put(lg, slots - 1, ns == 1 ? ones : zeros, ones);
    }
    return op;
}

}  // namespace kgwas
