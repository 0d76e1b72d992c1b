// lmm.cpp — kgwas_lmm_*: the mixed-model likelihood-ratio test that the pipeline takes from `gemma -lmm 2` (kmers_gwas.py:150-165),
// on the GPU (lmm_kernels.hip). This file holds the device session, the two passes over the variants of a PLINK
// .bed and the back-end steps they share with the k-mers table route (lmm_table.cpp); lmm_files.cpp is the file layer over both.
//
// create   : K's eigendecomposition on host threads (sym_eigen.cpp), the positive-semi-definite guard, then the device session:
//            U, d, wt = U^T 1, the grid of 101 lambdas and the table of h and dh/dlog lambda at them. All of it is shared by
//            every phenotype and .bed given to the handle;
// null     : yt = U^T (y - mean y) on the host in index order, the sums without x at the grid points, the null model's maximum;
// test_bed : per chunk of variants the raw bytes go to the device, then prep, rotate, grid and refine run in order on one stream;
// test_bed_multi: several phenotype columns against ONE .bed. Per chunk prep, rotate and the two grid sums without y run once; the
//            xt yt sums and the refinement run per block of LMM_PBLOCK columns. Every number has the bits of test_bed's.
// -lmm 4  : null_reml fits the REML null model (vg, ve) on the sums null left; test_bed_all is test_bed with the other refinement
//            kernel, which adds beta, se, l_remle and the Wald and score p-values and leaves lrt, lambda and p their bits.
// covariates: set_covariates replaces W = 1 by W (n x q): W is checked and orthonormalised on the host (orthonormal_covariates),
//            rotated like y and uploaded; null, null_reml, test_bed, test_bed_all and the table pass then launch the *_cov kernels,
//            the multi-phenotype passes refuse. Without covariates every launch is the one it was.
// No CPU fallback: the statistics need the GPU.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "lmm_internal.h"

using namespace kgwas;
using namespace kgwas::lmm;

// ---- the stage timer and the handle's buffers ----

void LmmStageTimer::stamp(hipStream_t st) {
    if (used == events.size()) {
        events.emplace_back();
        events.back().create();
    }
    KGWAS_HIP(hipEventRecord(events[used++], st));
}

void LmmStageTimer::collect(kgwas_lmm_stats& stats) {
    for (const Interval& i : closed) {
        float ms = 0;
        KGWAS_HIP(hipEventElapsedTime(&ms, events[i.from], events[i.from + 1]));
        stats.*i.bucket += ms;
    }
    closed.clear();
    used = 0;
}

void kgwas_lmm::ensure_multi_chunk() {
    if (have_multi_chunk) return;
    const uint64_t c = chunk;
    d_Gx.alloc(c * 2 * LMM_HB_COLS);
    d_Gxy.alloc(c * LMM_PBLOCK * LMM_HB_COLS);
    d_lrtm.alloc(c * LMM_PBLOCK);
    d_lamm.alloc(c * LMM_PBLOCK);
    d_pm.alloc(c * LMM_PBLOCK);
    h_outm.resize(3 * c * LMM_PBLOCK);
    have_multi_chunk = true;
}

void kgwas_lmm::ensure_multi_cols(uint32_t n_pheno) {
    if (n_pheno <= multi_cols) return;
    multi_cols = 0;
    d_Ytm.alloc((uint64_t)n_pheno * dm.ldi);
    d_basem.alloc((uint64_t)n_pheno * LMM_GRID * LMM_BASE);
    d_nullm.alloc(2 * (uint64_t)n_pheno);
    multi_cols = n_pheno;
}

void kgwas_lmm::ensure_select() {
    if (have_select) return;
    const uint64_t cap = (uint64_t)LMM_PBLOCK * chunk, n_blocks = (cap + LMM_TABLE_BLOCK - 1) / LMM_TABLE_BLOCK;
    d_sel_cnt.alloc(n_blocks);
    d_sel_off.alloc(n_blocks);
    d_sel_total.alloc(1);
    d_sel_cols.alloc(LMM_PBLOCK);
    d_sel_rec.alloc(cap);
    h_sel_rec.alloc(cap);
    have_select = true;
}

void kgwas_lmm::ensure_wald() {
    if (have_wald) return;
    d_wald.alloc(5 * (uint64_t)chunk);
    d_null_reml.alloc(4);
    have_wald = true;
}

namespace {

template <class T>
void upload(DevBuf<T>& b, const std::vector<T>& v) {
    b.alloc(v.size());
    KGWAS_HIP(hipMemcpy(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
}

void device_init(kgwas_lmm* h) {
    use_device(h->device);
    h->on_device = true;
    const uint64_t n = h->n, ldi = h->dm.ldi, n16 = h->dm.n16;
    std::vector<double> Up(n16 * ldi, 0.0), dp(ldi, 0.0), wt(ldi, 0.0), HB(ldi * LMM_HB_COLS, 0.0), grid(2 * LMM_GRID);
    for (uint64_t k = 0; k < n; k++) {
        memcpy(&Up[k * ldi], &h->U[k * n], n * sizeof(double));
        for (uint64_t i = 0; i < n; i++) wt[i] += h->U[k * n + i];  // U^T 1, in row order
    }
    for (uint64_t i = 0; i < n; i++) dp[i] = h->d[i];
    const double tmin = std::log(h->lmin), tmax = std::log(h->lmax);
    for (uint32_t g = 0; g < LMM_GRID; g++) {
        const double t = g == 0 ? tmin : g == LMM_GRID - 1 ? tmax : tmin + (double)g * ((tmax - tmin) / (double)(LMM_GRID - 1));
        grid[LMM_GRID + g] = t;
        grid[g] = g == 0 ? h->lmin : g == LMM_GRID - 1 ? h->lmax : std::exp(t);
    }
    for (uint64_t i = 0; i < n; i++)
        for (uint32_t g = 0; g < LMM_GRID; g++) {
            const double hh = 1.0 / (grid[g] * dp[i] + 1.0);
            HB[i * LMM_HB_COLS + g] = hh;
            HB[i * LMM_HB_COLS + LMM_GRID + g] = hh * hh - hh;
        }
    upload(h->d_U, Up);
    upload(h->d_d, dp);
    upload(h->d_wt, wt);
    upload(h->d_HB, HB);
    upload(h->d_grid, grid);
    h->d_yt.alloc(ldi);
    h->d_base.alloc(LMM_GRID * LMM_BASE);
    h->d_null.alloc(2);
    const uint64_t c = h->chunk;
    h->d_Xt.alloc(c * ldi);
    h->d_G.alloc(c * 3 * LMM_HB_COLS);
    h->d_lrt.alloc(c);
    h->d_lam.alloc(c);
    h->d_p.alloc(c);
    h->d_bed.alloc(c * h->dm.bps);
    h->d_codes.alloc(c * h->dm.bpsp);
    h->d_vars.alloc(c);
    h->stream.create(hipStreamNonBlocking);
}

// yt[ldi] (zeroed by the caller) = U^T (y - mean y), in index order; `where` ends the message of a refused y
void rotate_phenotype(const kgwas_lmm* h, const double* y, double* yt, const std::string& where) {
    const uint64_t n = h->n;
    double mean = 0;
    for (uint64_t k = 0; k < n; k++) {
        if (!std::isfinite(y[k])) throw Error(KGWAS_ERR_ARG, "kgwas_lmm: a phenotype value is not finite" + where);
        mean += y[k];
    }
    mean /= (double)n;
    bool varies = false;
    for (uint64_t k = 0; k < n; k++) {
        const double yc = y[k] - mean;
        varies |= yc != 0;
        const double* u = &h->U[k * n];
        for (uint64_t i = 0; i < n; i++) yt[i] += u[i] * yc;
    }
    if (!varies) throw Error(KGWAS_ERR_ARG, "kgwas_lmm: the phenotype is constant" + where);
}

// The end of a chunk of a .bed pass: the chunk's LmmVariants (on the host) go to the optional arrays from `pos` on, and the chunk
// is counted in the stats, a tested variant `weight` times (once per phenotype column).
void account_chunk(kgwas_lmm* h, const std::vector<LmmVariant>& vars, uint64_t pos, uint64_t weight, double* af, uint32_t* n_miss,
                   uint8_t* tested) {
    h->st.chunks++;
    for (size_t v = 0; v < vars.size(); v++) {
        if (af) af[pos + v] = vars[v].af;
        if (n_miss) n_miss[pos + v] = vars[v].n_miss;
        if (tested) tested[pos + v] = (uint8_t)vars[v].tested;
        h->st.variants_tested += (uint64_t)vars[v].tested * weight;
    }
    h->st.variants_read += vars.size();
}

}  // namespace

kgwas_lmm* kgwas::lmm::create(uint64_t n, const double* K, int device, double lmin, double lmax, uint64_t chunk_variants) {
    if (!K) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_create: null argument");
    if (n < 3 || n >= (1ull << 16)) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_create: the number of individuals must be within 3..65535");
    if (!(lmin > 0) || !(lmax > lmin) || !std::isfinite(lmax)) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_create: need 0 < lmin < lmax");
    std::unique_ptr<kgwas_lmm> h(new kgwas_lmm);
    h->device = device;
    h->n = n;
    h->lmin = lmin;
    h->lmax = lmax;
    h->dm.n = (uint32_t)n;
    h->dm.ldi = (uint32_t)((n + 63) / 64 * 64);
    h->dm.n16 = (uint32_t)((n + 15) / 16 * 16);
    h->dm.bps = (uint32_t)((n + 3) / 4);
    h->dm.bpsp = h->dm.n16 / 4;
    if (!chunk_variants) chunk_variants = 10240;  // a whole 10 001-variant file of pass 2 in one chunk (Xt: 94 MB at n = 1135)
    h->chunk = (uint32_t)((std::min<uint64_t>(chunk_variants, 1u << 16) + LMM_VTILE - 1) / LMM_VTILE * LMM_VTILE);
    h->U.resize(n * n);
    h->d.resize(n);
    const double t0 = now_ms();
    const int rc = kgwas_sym_eigen(n, K, h->d.data(), h->U.data(), 0);
    if (rc != KGWAS_OK) throw Error(rc, kgwas_last_error());
    h->st.eigen_ms = now_ms() - t0;
    h->st.eigendecompositions = 1;
    h->st.n_individuals = n;
    // transform_and_permute_phenotypes.R:54 (is.positive.semi.definite, tolerance 1e-8)
    for (double& v : h->d) {
        if (v < -1e-8) throw Error(KGWAS_ERR_FORMAT, "Kinship matrix is not positive semi-definite");
        if (std::fabs(v) < 1e-8) v = 0;
    }
    device_init(h.get());
    return h.release();
}

void kgwas::lmm::fit_null(kgwas_lmm* h, const double* y) {
    const uint64_t n = h->n;
    if (h->have_null && memcmp(h->y_cur.data(), y, n * sizeof(double)) == 0) return;
    std::vector<double> yt(h->dm.ldi, 0.0);
    rotate_phenotype(h, y, yt.data(), "");
    KGWAS_HIP(hipSetDevice(h->device));
    h->have_null = h->have_null_reml = false;
    KGWAS_HIP(hipMemcpyAsync(h->d_yt.p, yt.data(), yt.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    KGWAS_HIP(launch_lmm_base(h->dm, h->q, h->d_d.p, h->fixed_t(), h->d_yt.p, 1, h->d_grid.p, h->base_rows(), h->stream));
    KGWAS_HIP(launch_lmm_null(h->dm, h->q, h->d_d.p, h->fixed_t(), h->d_yt.p, 1, h->d_grid.p, h->base_rows(), h->d_null.p, h->stream));
    double out[2];
    KGWAS_HIP(hipMemcpyAsync(out, h->d_null.p, sizeof(out), hipMemcpyDeviceToHost, h->stream));
    KGWAS_HIP(hipStreamSynchronize(h->stream));  // (yt is read by the copy until here)
    h->l0 = out[0];
    h->lambda0 = out[1];
    h->y_cur.assign(y, y + n);
    h->have_null = true;
}

// The REML null model of y on what fit_null left on the device (yt and the base sums): l0_reml, lambda0_reml, vg, ve.
void kgwas::lmm::fit_null_reml(kgwas_lmm* h, const double* y) {
    fit_null(h, y);
    if (h->have_null_reml) return;
    KGWAS_HIP(hipSetDevice(h->device));
    h->ensure_wald();
    KGWAS_HIP(launch_lmm_null_reml(h->dm, h->q, h->d_d.p, h->fixed_t(), h->d_yt.p, h->d_grid.p, h->base_rows(), h->d_null_reml.p, h->stream));
    double out[4];
    KGWAS_HIP(hipMemcpyAsync(out, h->d_null_reml.p, sizeof(out), hipMemcpyDeviceToHost, h->stream));
    KGWAS_HIP(hipStreamSynchronize(h->stream));
    h->l0_reml = out[0] - h->log_det_R;  // (0 without covariates)
    h->lambda0_reml = out[1];
    h->vg = out[2];
    h->ve = out[3];
    h->have_null_reml = true;
}

// ---- covariates ----

void kgwas::lmm::orthonormal_covariates(uint64_t n, uint32_t q, const double* W, std::vector<double>& Qw, double& log_det_R,
                                        const std::string& who) {
    if (q < 1 || q > LMM_MAXC)
        throw Error(KGWAS_ERR_ARG, who + ": " + std::to_string(q) + " covariate columns; at most " + std::to_string(LMM_MAXC) + " are built");
    for (uint64_t k = 0; k < n * q; k++)
        if (!std::isfinite(W[k])) throw Error(KGWAS_ERR_ARG, who + ": a covariate value is not finite");
    if (n < (uint64_t)q + 2)
        throw Error(KGWAS_ERR_ARG, who + ": " + std::to_string(n) + " individuals are too few for " + std::to_string(q) +
                                       " covariate columns (at least " + std::to_string(q + 2) + " are needed)");
    std::vector<std::vector<double>> col(q, std::vector<double>(n));
    const auto dot = [n](const std::vector<double>& a, const std::vector<double>& b) {
        double s = 0;
        for (uint64_t k = 0; k < n; k++) s += a[k] * b[k];
        return s;
    };
    const auto project_out = [&](std::vector<double>& v, uint32_t upto) {  // twice: the second pass removes what rounding left
        for (int pass = 0; pass < 2; pass++)
            for (uint32_t c = 0; c < upto; c++) {
                const double t = dot(col[c], v);
                for (uint64_t k = 0; k < n; k++) v[k] -= t * col[c][k];
            }
    };
    log_det_R = 0;
    for (uint32_t j = 0; j < q; j++) {
        std::vector<double>& v = col[j];
        for (uint64_t k = 0; k < n; k++) v[k] = W[k * q + j];
        const double norm = std::sqrt(dot(v, v));
        project_out(v, j);
        const double rest = std::sqrt(dot(v, v));
        if (!(rest > 1e-8 * norm))
            throw Error(KGWAS_ERR_ARG, who + ": the covariates are rank-deficient: column " + std::to_string(j + 1) +
                                           " is a combination of the columns before it");
        for (uint64_t k = 0; k < n; k++) v[k] /= rest;
        log_det_R += std::log(rest);
    }
    std::vector<double> one(n, 1.0);
    project_out(one, q);
    if (!(std::sqrt(dot(one, one)) <= 1e-8 * std::sqrt((double)n)))
        throw Error(KGWAS_ERR_ARG, who + ": the covariates do not span the constant vector: give the file a column of 1s (the intercept)");
    Qw.resize(n * q);
    for (uint32_t j = 0; j < q; j++)
        for (uint64_t k = 0; k < n; k++) Qw[k * q + j] = col[j][k];
}

// W[n][q] in place of W = 1 for every later call with one phenotype; q = 0 restores W = 1. The null models are forgotten.
void kgwas::lmm::set_covariates(kgwas_lmm* h, uint32_t q, const double* W) {
    const uint64_t n = h->n, ldi = h->dm.ldi;
    if (!q) {
        h->q = 0;
        h->log_det_R = 0;
        h->have_null = h->have_null_reml = false;
        return;
    }
    if (!W) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_set_covariates: null argument");
    std::vector<double> Qw;
    double log_det_R = 0;
    orthonormal_covariates(n, q, W, Qw, log_det_R, "kgwas_lmm_set_covariates");
    std::vector<double> Wt((uint64_t)q * ldi, 0.0);
    for (uint64_t k = 0; k < n; k++) {  // U^T Q, in row order
        const double* u = &h->U[k * n];
        for (uint32_t j = 0; j < q; j++) {
            const double w = Qw[k * q + j];
            double* out = &Wt[(uint64_t)j * ldi];
            for (uint64_t i = 0; i < n; i++) out[i] += u[i] * w;
        }
    }
    KGWAS_HIP(hipSetDevice(h->device));
    KGWAS_HIP(hipStreamSynchronize(h->stream));
    h->have_null = h->have_null_reml = false;
    h->q = 0;  // (until everything below is in place)
    if (h->g_rows < (uint64_t)q + 2) {
        h->d_G.alloc((uint64_t)h->chunk * (q + 2) * LMM_HB_COLS);
        h->g_rows = (uint64_t)q + 2;
    }
    if (!h->d_basec.p) h->d_basec.alloc((uint64_t)LMM_GRID * LMM_BASEC);
    upload(h->d_Wt, Wt);
    h->q = q;
    h->log_det_R = log_det_R;
}

// ---- the back-end steps. They launch on the handle's stream and time their stages; the caller issues the copies, synchronises
// the stream and collects the times (h->timer.collect). ----

// The single-phenotype back end over cc variants: rotate -> grid -> refine against the null model fit_null left; codes and vars
// are on the device. Leaves d_lrt, d_lam, d_p. The caller has opened the rotation's interval (test_bed's prep falls into it).
void kgwas::lmm::single_backend(kgwas_lmm* h, const uint8_t* codes, const LmmVariant* vars, uint32_t cc, bool wald) {
    hipStream_t st = h->stream;
    KGWAS_HIP(launch_lmm_rotate(codes, vars, cc, h->dm, h->d_U.p, h->d_Xt.p, st));
    h->timer.end(&kgwas_lmm_stats::rotate_ms, st);
    KGWAS_HIP(launch_lmm_grid(h->d_Xt.p, cc, h->dm, h->q, h->fixed_t(), h->d_yt.p, h->d_HB.p, h->d_G.p, st));
    h->timer.end(&kgwas_lmm_stats::grid_ms, st);
    if (wald)  // -lmm 4 (the caller has called ensure_wald): d_wald too
        KGWAS_HIP(launch_lmm_refine_all(h->d_Xt.p, h->d_G.p, vars, cc, h->dm, h->q, h->d_d.p, h->fixed_t(), h->d_yt.p, h->d_grid.p,
                                        h->base_rows(), h->l0, h->lambda0, h->d_lrt.p, h->d_lam.p, h->d_p.p, h->wald_out(), st));
    else
        KGWAS_HIP(launch_lmm_refine(h->d_Xt.p, h->d_G.p, vars, cc, h->dm, h->q, h->d_d.p, h->fixed_t(), h->d_yt.p, h->d_grid.p, h->base_rows(),
                                    h->l0, h->d_lrt.p, h->d_lam.p, h->d_p.p, st));
    h->timer.end(&kgwas_lmm_stats::refine_ms, st);
}

// What the phenotype columns of a multi pass share over cc variants: the rotation and the grid sums without y (d_Xt, d_Gx). The
// caller has opened the rotation's interval, as for single_backend.
void kgwas::lmm::multi_front(kgwas_lmm* h, const uint8_t* codes, const LmmVariant* vars, uint32_t cc) {
    hipStream_t st = h->stream;
    KGWAS_HIP(launch_lmm_rotate(codes, vars, cc, h->dm, h->d_U.p, h->d_Xt.p, st));
    h->timer.end(&kgwas_lmm_stats::rotate_ms, st);
    KGWAS_HIP(launch_lmm_grid_shared(h->d_Xt.p, cc, h->dm, h->d_wt.p, h->d_HB.p, h->d_Gx.p, st));
    h->timer.end(&kgwas_lmm_stats::grid_ms, st);
}

// The block of pb <= LMM_PBLOCK columns from p0 on, after multi_front: the xt yt sums and the refinement against the columns
// multi_prepare left. Leaves d_lrtm, d_lamm, d_pm as [pb][cc]. The refinement's interval stays open: the caller closes it into
// refine_ms, the table route after the select kernels it launches behind.
void kgwas::lmm::multi_block(kgwas_lmm* h, const LmmVariant* vars, uint32_t cc, uint32_t p0, uint32_t pb) {
    hipStream_t st = h->stream;
    const double* Ytb = h->d_Ytm.p + (uint64_t)p0 * h->dm.ldi;
    h->timer.begin(st);
    KGWAS_HIP(launch_lmm_grid_xy(h->d_Xt.p, cc, h->dm, Ytb, pb, h->d_HB.p, h->d_Gxy.p, st));
    h->timer.end(&kgwas_lmm_stats::grid_ms, st);
    KGWAS_HIP(launch_lmm_refine_multi(h->d_Xt.p, h->d_Gx.p, h->d_Gxy.p, vars, cc, h->dm, h->d_d.p, h->d_wt.p, Ytb, pb, h->d_grid.p,
                                      h->d_basem.p + (uint64_t)p0 * LMM_GRID * LMM_BASE, h->d_nullm.p + 2 * (uint64_t)p0, h->d_lrtm.p,
                                      h->d_lamm.p, h->d_pm.p, st));
}

// ---- the .bed passes ----

void kgwas::lmm::test_bed(kgwas_lmm* h, const double* y, const uint8_t* body, uint64_t nv, double maf, double miss, double* lrt,
                          double* lam, double* p, double* af, uint32_t* n_miss, uint8_t* tested, const WaldArrays* wald) {
    fit_null(h, y);
    KGWAS_HIP(hipSetDevice(h->device));
    if (wald) h->ensure_wald();
    hipStream_t st = h->stream;
    std::vector<LmmVariant> vars;
    for (uint64_t pos = 0; pos < nv; pos += h->chunk) {
        const uint32_t c = (uint32_t)std::min<uint64_t>(h->chunk, nv - pos);
        KGWAS_HIP(hipMemcpyAsync(h->d_bed.p, body + pos * h->dm.bps, (size_t)c * h->dm.bps, hipMemcpyHostToDevice, st));
        h->timer.begin(st);
        KGWAS_HIP(launch_lmm_prep(h->d_bed.p, c, h->dm, maf, miss, h->d_codes.p, h->d_vars.p, st));
        single_backend(h, h->d_codes.p, h->d_vars.p, c, wald != nullptr);
        if (wald) {
            double* const host[5] = {wald->beta, wald->se, wald->lam_remle, wald->p_wald, wald->p_score};
            for (int a = 0; a < 5; a++)
                if (host[a])
                    KGWAS_HIP(hipMemcpyAsync(host[a] + pos, h->d_wald.p + (uint64_t)a * h->chunk, c * sizeof(double), hipMemcpyDeviceToHost, st));
        }
        if (lrt) KGWAS_HIP(hipMemcpyAsync(lrt + pos, h->d_lrt.p, c * sizeof(double), hipMemcpyDeviceToHost, st));
        if (lam) KGWAS_HIP(hipMemcpyAsync(lam + pos, h->d_lam.p, c * sizeof(double), hipMemcpyDeviceToHost, st));
        if (p) KGWAS_HIP(hipMemcpyAsync(p + pos, h->d_p.p, c * sizeof(double), hipMemcpyDeviceToHost, st));
        vars.resize(c);
        KGWAS_HIP(hipMemcpyAsync(vars.data(), h->d_vars.p, c * sizeof(LmmVariant), hipMemcpyDeviceToHost, st));
        KGWAS_HIP(hipStreamSynchronize(st));
        h->timer.collect(h->st);
        account_chunk(h, vars, pos, 1, af, n_miss, tested);
    }
}

// The multi-phenotype pass. Nothing of the single-phenotype null (y_cur, have_null, d_yt, d_base, l0) is touched.
// multi_prepare: Y[n_pheno][n] -> Yt, the base sums and the null models of all columns on the device; logl0, lambda0 [n_pheno].
void kgwas::lmm::multi_prepare(kgwas_lmm* h, uint32_t n_pheno, const double* Y, double* logl0, double* lambda0, const char* who) {
    if (h->q) throw Error(KGWAS_ERR_ARG, std::string(who) + ": covariates are not built for the multi-phenotype passes");
    if (!n_pheno) throw Error(KGWAS_ERR_ARG, std::string(who) + ": n_pheno is 0");
    const uint64_t n = h->n, ldi = h->dm.ldi;
    std::vector<double> Yt((uint64_t)n_pheno * ldi, 0.0);
    for (uint32_t k = 0; k < n_pheno; k++) rotate_phenotype(h, Y + k * n, &Yt[k * ldi], " (column " + std::to_string(k) + ")");
    KGWAS_HIP(hipSetDevice(h->device));
    h->ensure_multi_chunk();
    h->ensure_multi_cols(n_pheno);
    hipStream_t st = h->stream;
    KGWAS_HIP(hipMemcpyAsync(h->d_Ytm.p, Yt.data(), Yt.size() * sizeof(double), hipMemcpyHostToDevice, st));
    KGWAS_HIP(launch_lmm_base(h->dm, 0, h->d_d.p, h->d_wt.p, h->d_Ytm.p, n_pheno, h->d_grid.p, h->d_basem.p, st));
    KGWAS_HIP(launch_lmm_null(h->dm, 0, h->d_d.p, h->d_wt.p, h->d_Ytm.p, n_pheno, h->d_grid.p, h->d_basem.p, h->d_nullm.p, st));
    std::vector<double> nulls(2 * (uint64_t)n_pheno);
    KGWAS_HIP(hipMemcpyAsync(nulls.data(), h->d_nullm.p, nulls.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    KGWAS_HIP(hipStreamSynchronize(st));  // (Yt is read by the copy until here)
    for (uint32_t k = 0; k < n_pheno; k++) {
        if (logl0) logl0[k] = nulls[2 * k];
        if (lambda0) lambda0[k] = nulls[2 * k + 1];
    }
}

// multi_run: nv variants against the n_pheno columns multi_prepare left on the device; lrt, lam, p are [n_pheno][nv]. Per chunk
// prep, rotate and the shared grid sums run once; the xt yt sums and the refinement per block of LMM_PBLOCK columns.
void kgwas::lmm::multi_run(kgwas_lmm* h, uint32_t n_pheno, const uint8_t* body, uint64_t nv, double maf, double miss, double* lrt,
                           double* lam, double* p, double* af, uint32_t* n_miss, uint8_t* tested) {
    KGWAS_HIP(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    std::vector<LmmVariant> vars;
    for (uint64_t pos = 0; pos < nv; pos += h->chunk) {
        const uint32_t c = (uint32_t)std::min<uint64_t>(h->chunk, nv - pos);
        KGWAS_HIP(hipMemcpyAsync(h->d_bed.p, body + pos * h->dm.bps, (size_t)c * h->dm.bps, hipMemcpyHostToDevice, st));
        h->timer.begin(st);
        KGWAS_HIP(launch_lmm_prep(h->d_bed.p, c, h->dm, maf, miss, h->d_codes.p, h->d_vars.p, st));
        multi_front(h, h->d_codes.p, h->d_vars.p, c);
        vars.resize(c);
        KGWAS_HIP(hipMemcpyAsync(vars.data(), h->d_vars.p, c * sizeof(LmmVariant), hipMemcpyDeviceToHost, st));
        KGWAS_HIP(hipStreamSynchronize(st));
        h->timer.collect(h->st);
        for (uint32_t p0 = 0; p0 < n_pheno; p0 += LMM_PBLOCK) {
            const uint32_t pb = std::min(LMM_PBLOCK, n_pheno - p0);
            const uint64_t cnt = (uint64_t)pb * c;
            multi_block(h, h->d_vars.p, c, p0, pb);
            h->timer.end(&kgwas_lmm_stats::refine_ms, st);
            double* const host[3] = {lrt, lam, p};
            const double* const dev[3] = {h->d_lrtm.p, h->d_lamm.p, h->d_pm.p};
            for (int a = 0; a < 3; a++)
                if (host[a]) KGWAS_HIP(hipMemcpyAsync(&h->h_outm[a * cnt], dev[a], cnt * sizeof(double), hipMemcpyDeviceToHost, st));
            KGWAS_HIP(hipStreamSynchronize(st));
            h->timer.collect(h->st);
            for (int a = 0; a < 3; a++)
                if (host[a])
                    for (uint32_t k = 0; k < pb; k++)
                        memcpy(host[a] + (uint64_t)(p0 + k) * nv + pos, &h->h_outm[a * cnt + (uint64_t)k * c], c * sizeof(double));
        }
        account_chunk(h, vars, pos, n_pheno, af, n_miss, tested);
    }
}

extern "C" {

int kgwas_lmm_create(uint64_t n, const double* K, int32_t device, double lmin, double lmax, uint64_t chunk_variants, kgwas_lmm** out) {
    return guarded([&] {
        if (!out) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_create: null argument");
        *out = create(n, K, device, lmin, lmax, chunk_variants);
    });
}

int kgwas_lmm_null(kgwas_lmm* h, const double* y, double* logl0, double* lambda0) {
    return guarded([&] {
        if (!h || !y) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_null: null argument");
        fit_null(h, y);
        if (logl0) *logl0 = h->l0;
        if (lambda0) *lambda0 = h->lambda0;
    });
}

int kgwas_lmm_test_bed(kgwas_lmm* h, const double* y, const uint8_t* bed_body, uint64_t n_variants, double maf, double miss, double* lrt,
                       double* lambda, double* p, double* af, uint32_t* n_miss, uint8_t* tested) {
    return guarded([&] {
        if (!h || !y || (!bed_body && n_variants)) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_test_bed: null argument");
        test_bed(h, y, bed_body, n_variants, maf, miss, lrt, lambda, p, af, n_miss, tested);
    });
}

int kgwas_lmm_null_reml(kgwas_lmm* h, const double* y, double* logl0_reml, double* lambda0_reml, double* vg, double* ve) {
    return guarded([&] {
        if (!h || !y) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_null_reml: null argument");
        fit_null_reml(h, y);
        if (logl0_reml) *logl0_reml = h->l0_reml;
        if (lambda0_reml) *lambda0_reml = h->lambda0_reml;
        if (vg) *vg = h->vg;
        if (ve) *ve = h->ve;
    });
}

int kgwas_lmm_test_bed_all(kgwas_lmm* h, const double* y, const uint8_t* bed_body, uint64_t n_variants, double maf, double miss, double* lrt,
                           double* lambda_mle, double* p_lrt, double* beta, double* se, double* lambda_remle, double* p_wald,
                           double* p_score, double* af, uint32_t* n_miss, uint8_t* tested) {
    return guarded([&] {
        if (!h || !y || (!bed_body && n_variants)) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_test_bed_all: null argument");
        const WaldArrays w = {beta, se, lambda_remle, p_wald, p_score};
        test_bed(h, y, bed_body, n_variants, maf, miss, lrt, lambda_mle, p_lrt, af, n_miss, tested, &w);
    });
}

int kgwas_lmm_test_bed_multi(kgwas_lmm* h, uint32_t n_pheno, const double* Y, const uint8_t* bed_body, uint64_t n_variants, double maf,
                             double miss, double* lrt, double* lambda, double* p, double* logl0, double* lambda0, double* af,
                             uint32_t* n_miss, uint8_t* tested) {
    return guarded([&] {
        if (!h || (!Y && n_pheno) || (!bed_body && n_variants)) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_test_bed_multi: null argument");
        multi_prepare(h, n_pheno, Y, logl0, lambda0);
        multi_run(h, n_pheno, bed_body, n_variants, maf, miss, lrt, lambda, p, af, n_miss, tested);
    });
}

int kgwas_lmm_set_covariates(kgwas_lmm* h, uint32_t q, const double* W) {
    return guarded([&] {
        if (!h) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_set_covariates: null argument");
        set_covariates(h, q, W);
    });
}

int kgwas_lmm_get_stats(const kgwas_lmm* h, kgwas_lmm_stats* out) {
    return guarded([&] {
        if (!h || !out) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_get_stats: null argument");
        *out = h->st;
    });
}

void kgwas_lmm_destroy(kgwas_lmm* h) { delete h; }

}  // extern "C"
