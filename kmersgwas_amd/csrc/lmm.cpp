// lmm.cpp — kgwas_lmm_*: the mixed-model likelihood-ratio test that the pipeline takes from `gemma -lmm 2` (kmers_gwas.py:150-165),
// for the variants of PLINK .bed files, on the GPU (lmm_kernels.hip).
//
// create   : K's eigendecomposition on host threads (sym_eigen.cpp), the positive-semi-definite guard, then the device session:
//            U, d, wt = U^T 1, the grid of 101 lambdas and the table of h and dh/dlog lambda at them. All of it is shared by
//            every phenotype and .bed given to the handle;
// null     : yt = U^T (y - mean y) on the host in index order, the sums without x at the grid points, the null model's maximum;
// test_bed : per chunk of variants the raw bytes go to the device, then prep, rotate, grid and refine run in order on one stream;
// test_bed_multi: several phenotype columns against ONE .bed. Per chunk prep, rotate and the two grid sums without y run once; the
//            xt yt sums and the refinement run per block of LMM_PBLOCK columns. Every number has the bits of test_bed's;
// test_table: every row of a k-mers table, without a .bed in between. Per piece of rows the device squeezes them to phenotype
//            order, flags the rows that kmers_table_to_bed would write AND prep would test, and compacts those into code rows
//            and LmmVariants with prep's bits (lmm_table_kernels.hip); rotate, grid and refine then run over them unchanged. The
//            host keeps the best N by (lrt, table row). run_table is its file layer (lmm_lrt --kmers_table);
// test_table_multi: several phenotype columns against ONE table in one pass (the phenotype and its permutations). The front end and
//            the rotation run once per row, the xt yt sums and the refinement per block of LMM_PBLOCK columns, and a select kernel
//            hands the host only the (column, row) pairs that can still enter a column's best N. Every kept row and number has the
//            bits of test_table's for that column. run_table_multi is its file layer (lmm_lrt --kmers_table --pheno_columns);
// run_files: the file layer of the lmm_lrt tool - kinship text, .fam phenotype column, .bim, .bed in, .assoc.txt and .log.txt out.
//            Individuals without a phenotype are dropped from K, y and the .bed rows before anything else; beds that keep the
//            same individuals share one handle, so one eigendecomposition. run_file_multi: one bfile, several .fam columns with
//            one missing set, one pass over the .bed (the shape of kmers_gwas.py:193-223).
// No CPU fallback: the statistics need the GPU. The parsers and the formatter run without one.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <exception>
#include <fstream>
#include <memory>
#include <mutex>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "common.h"
#include "ingest.h"
#include "kernels.h"
#include "lmm_kernels.h"

using namespace kgwas;

struct kgwas_lmm {
    int device = 0;
    uint64_t n = 0;
    LmmDims dm{};
    double lmin = 0, lmax = 0;
    uint32_t chunk = 0;
    std::vector<double> U, d;
    std::vector<double> y_cur;
    bool have_null = false;
    double l0 = 0, lambda0 = 0;
    kgwas_lmm_stats st{};
    bool on_device = false;
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    DevBuf<double> d_U, d_d, d_wt, d_yt, d_HB, d_grid, d_base, d_null, d_Xt, d_G, d_lrt, d_lam, d_p;
    DevBuf<uint8_t> d_bed, d_codes;
    DevBuf<LmmVariant> d_vars;
    // the multi-phenotype pass (allocated at its first call): per column Yt, base sums and null model; per chunk the shared grid
    // sums; per chunk and block of LMM_PBLOCK columns the xt yt sums and the results
    bool multi_ready = false;  // the per-chunk buffers below are allocated
    uint32_t multi_cols = 0;
    DevBuf<double> d_Ytm, d_basem, d_nullm, d_Gx, d_Gxy, d_lrtm, d_lamm, d_pm;
    std::vector<double> h_outm;
    // the selection of the multi-phenotype table pass (allocated at its first call): per block of 256 pairs the counts and offsets,
    // the survivors' number, the block's thresholds, and the records on the device and in pinned host memory
    bool select_ready = false;
    DevBuf<uint32_t> d_sel_cnt, d_sel_off, d_sel_total;
    DevBuf<LmmSelectCol> d_sel_cols;
    DevBuf<LmmTableRecord> d_sel_rec;
    PinBuf<LmmTableRecord> h_sel_rec;
    ~kgwas_lmm() {
        if (!on_device) return;
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace {

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

template <class T>
void upload(DevBuf<T>& b, const std::vector<T>& v) {
    b.alloc(v.size());
    KGWAS_HIP(hipMemcpy(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
}

void device_init(kgwas_lmm* h) {
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) throw Error(KGWAS_ERR_DEVICE, "no HIP device available: libkgwas has no CPU fallback");
    if (h->device < 0 || h->device >= nd) throw Error(KGWAS_ERR_ARG, "device ordinal out of range");
    KGWAS_HIP(hipSetDevice(h->device));
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
    KGWAS_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    for (hipEvent_t& e : h->ev) KGWAS_HIP(hipEventCreate(&e));
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

void fit_null(kgwas_lmm* h, const double* y) {
    const uint64_t n = h->n;
    if (h->have_null && memcmp(h->y_cur.data(), y, n * sizeof(double)) == 0) return;
    std::vector<double> yt(h->dm.ldi, 0.0);
    rotate_phenotype(h, y, yt.data(), "");
    KGWAS_HIP(hipSetDevice(h->device));
    h->have_null = false;
    KGWAS_HIP(hipMemcpyAsync(h->d_yt.p, yt.data(), yt.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    KGWAS_HIP(launch_lmm_base(h->dm, h->d_d.p, h->d_wt.p, h->d_yt.p, h->d_grid.p, h->d_base.p, h->stream));
    KGWAS_HIP(launch_lmm_null(h->dm, h->d_d.p, h->d_wt.p, h->d_yt.p, h->d_grid.p, h->d_base.p, h->d_null.p, h->stream));
    double out[2];
    KGWAS_HIP(hipMemcpyAsync(out, h->d_null.p, sizeof(out), hipMemcpyDeviceToHost, h->stream));
    KGWAS_HIP(hipStreamSynchronize(h->stream));  // (yt is read by the copy until here)
    h->l0 = out[0];
    h->lambda0 = out[1];
    h->y_cur.assign(y, y + n);
    h->have_null = true;
}

void test_bed(kgwas_lmm* h, const double* y, const uint8_t* body, uint64_t nv, double maf, double miss, double* lrt, double* lam,
              double* p, double* af, uint32_t* n_miss, uint8_t* tested) {
    fit_null(h, y);
    KGWAS_HIP(hipSetDevice(h->device));
    std::vector<LmmVariant> vars;
    for (uint64_t pos = 0; pos < nv; pos += h->chunk) {
        const uint32_t c = (uint32_t)std::min<uint64_t>(h->chunk, nv - pos);
        hipStream_t st = h->stream;
        KGWAS_HIP(hipMemcpyAsync(h->d_bed.p, body + pos * h->dm.bps, (size_t)c * h->dm.bps, hipMemcpyHostToDevice, st));
        KGWAS_HIP(hipEventRecord(h->ev[0], st));
        KGWAS_HIP(launch_lmm_prep(h->d_bed.p, c, h->dm, maf, miss, h->d_codes.p, h->d_vars.p, st));
        KGWAS_HIP(launch_lmm_rotate(h->d_codes.p, h->d_vars.p, c, h->dm, h->d_U.p, h->d_Xt.p, st));
        KGWAS_HIP(hipEventRecord(h->ev[1], st));
        KGWAS_HIP(launch_lmm_grid(h->d_Xt.p, c, h->dm, h->d_wt.p, h->d_yt.p, h->d_HB.p, h->d_G.p, st));
        KGWAS_HIP(hipEventRecord(h->ev[2], st));
        KGWAS_HIP(launch_lmm_refine(h->d_Xt.p, h->d_G.p, h->d_vars.p, c, h->dm, h->d_d.p, h->d_wt.p, h->d_yt.p, h->d_grid.p, h->d_base.p,
                                    h->l0, h->d_lrt.p, h->d_lam.p, h->d_p.p, st));
        KGWAS_HIP(hipEventRecord(h->ev[3], st));
        if (lrt) KGWAS_HIP(hipMemcpyAsync(lrt + pos, h->d_lrt.p, c * sizeof(double), hipMemcpyDeviceToHost, st));
        if (lam) KGWAS_HIP(hipMemcpyAsync(lam + pos, h->d_lam.p, c * sizeof(double), hipMemcpyDeviceToHost, st));
        if (p) KGWAS_HIP(hipMemcpyAsync(p + pos, h->d_p.p, c * sizeof(double), hipMemcpyDeviceToHost, st));
        vars.resize(c);
        KGWAS_HIP(hipMemcpyAsync(vars.data(), h->d_vars.p, c * sizeof(LmmVariant), hipMemcpyDeviceToHost, st));
        KGWAS_HIP(hipStreamSynchronize(st));
        float ms[3] = {0, 0, 0};
        for (int k = 0; k < 3; k++) KGWAS_HIP(hipEventElapsedTime(&ms[k], h->ev[k], h->ev[k + 1]));
        h->st.rotate_ms += ms[0];
        h->st.grid_ms += ms[1];
        h->st.refine_ms += ms[2];
        h->st.chunks++;
        for (uint32_t v = 0; v < c; v++) {
            if (af) af[pos + v] = vars[v].af;
            if (n_miss) n_miss[pos + v] = vars[v].n_miss;
            if (tested) tested[pos + v] = (uint8_t)vars[v].tested;
            h->st.variants_tested += vars[v].tested;
        }
        h->st.variants_read += c;
    }
}

// The multi-phenotype pass. Nothing of the single-phenotype null (y_cur, have_null, d_yt, d_base, l0) is touched.
// multi_prepare: Y[n_pheno][n] -> Yt, the base sums and the null models of all columns on the device; logl0, lambda0 [n_pheno].
void multi_prepare(kgwas_lmm* h, uint32_t n_pheno, const double* Y, double* logl0, double* lambda0,
                   const char* who = "kgwas_lmm_test_bed_multi") {
    if (!n_pheno) throw Error(KGWAS_ERR_ARG, std::string(who) + ": n_pheno is 0");
    const uint64_t n = h->n, ldi = h->dm.ldi, chunk = h->chunk;
    std::vector<double> Yt((uint64_t)n_pheno * ldi, 0.0);
    for (uint32_t k = 0; k < n_pheno; k++) rotate_phenotype(h, Y + k * n, &Yt[k * ldi], " (column " + std::to_string(k) + ")");
    KGWAS_HIP(hipSetDevice(h->device));
    if (!h->multi_ready) {
        h->d_Gx.alloc(chunk * 2 * LMM_HB_COLS);
        h->d_Gxy.alloc(chunk * LMM_PBLOCK * LMM_HB_COLS);
        h->d_lrtm.alloc(chunk * LMM_PBLOCK);
        h->d_lamm.alloc(chunk * LMM_PBLOCK);
        h->d_pm.alloc(chunk * LMM_PBLOCK);
        h->h_outm.resize(3 * chunk * LMM_PBLOCK);
        h->multi_ready = true;
    }
    if (n_pheno > h->multi_cols) {
        h->multi_cols = 0;
        h->d_Ytm.alloc((uint64_t)n_pheno * ldi);
        h->d_basem.alloc((uint64_t)n_pheno * LMM_GRID * LMM_BASE);
        h->d_nullm.alloc(2 * (uint64_t)n_pheno);
        h->multi_cols = n_pheno;
    }
    hipStream_t st = h->stream;
    KGWAS_HIP(hipMemcpyAsync(h->d_Ytm.p, Yt.data(), Yt.size() * sizeof(double), hipMemcpyHostToDevice, st));
    KGWAS_HIP(launch_lmm_base_multi(h->dm, h->d_d.p, h->d_wt.p, h->d_Ytm.p, n_pheno, h->d_grid.p, h->d_basem.p, st));
    KGWAS_HIP(launch_lmm_null_multi(h->dm, h->d_d.p, h->d_wt.p, h->d_Ytm.p, n_pheno, h->d_grid.p, h->d_basem.p, h->d_nullm.p, st));
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
void multi_run(kgwas_lmm* h, uint32_t n_pheno, const uint8_t* body, uint64_t nv, double maf, double miss, double* lrt, double* lam,
               double* p, double* af, uint32_t* n_miss, uint8_t* tested) {
    KGWAS_HIP(hipSetDevice(h->device));
    const uint64_t ldi = h->dm.ldi, chunk = h->chunk;
    hipStream_t st = h->stream;
    std::vector<LmmVariant> vars;
    for (uint64_t pos = 0; pos < nv; pos += chunk) {
        const uint32_t c = (uint32_t)std::min<uint64_t>(chunk, nv - pos);
        KGWAS_HIP(hipMemcpyAsync(h->d_bed.p, body + pos * h->dm.bps, (size_t)c * h->dm.bps, hipMemcpyHostToDevice, st));
        KGWAS_HIP(hipEventRecord(h->ev[0], st));
        KGWAS_HIP(launch_lmm_prep(h->d_bed.p, c, h->dm, maf, miss, h->d_codes.p, h->d_vars.p, st));
        KGWAS_HIP(launch_lmm_rotate(h->d_codes.p, h->d_vars.p, c, h->dm, h->d_U.p, h->d_Xt.p, st));
        KGWAS_HIP(hipEventRecord(h->ev[1], st));
        KGWAS_HIP(launch_lmm_grid_shared(h->d_Xt.p, c, h->dm, h->d_wt.p, h->d_HB.p, h->d_Gx.p, st));
        KGWAS_HIP(hipEventRecord(h->ev[2], st));
        vars.resize(c);
        KGWAS_HIP(hipMemcpyAsync(vars.data(), h->d_vars.p, c * sizeof(LmmVariant), hipMemcpyDeviceToHost, st));
        KGWAS_HIP(hipStreamSynchronize(st));
        float ms[2] = {0, 0};
        for (int k = 0; k < 2; k++) KGWAS_HIP(hipEventElapsedTime(&ms[k], h->ev[k], h->ev[k + 1]));
        h->st.rotate_ms += ms[0];
        h->st.grid_ms += ms[1];
        for (uint32_t p0 = 0; p0 < n_pheno; p0 += LMM_PBLOCK) {
            const uint32_t pb = std::min(LMM_PBLOCK, n_pheno - p0);
            const uint64_t cnt = (uint64_t)pb * c;
            const double* Ytb = h->d_Ytm.p + (uint64_t)p0 * ldi;
            KGWAS_HIP(hipEventRecord(h->ev[1], st));
            KGWAS_HIP(launch_lmm_grid_xy(h->d_Xt.p, c, h->dm, Ytb, pb, h->d_HB.p, h->d_Gxy.p, st));
            KGWAS_HIP(hipEventRecord(h->ev[2], st));
            KGWAS_HIP(launch_lmm_refine_multi(h->d_Xt.p, h->d_Gx.p, h->d_Gxy.p, h->d_vars.p, c, h->dm, h->d_d.p, h->d_wt.p, Ytb, pb,
                                              h->d_grid.p, h->d_basem.p + (uint64_t)p0 * LMM_GRID * LMM_BASE, h->d_nullm.p + 2 * (uint64_t)p0,
                                              h->d_lrtm.p, h->d_lamm.p, h->d_pm.p, st));
            KGWAS_HIP(hipEventRecord(h->ev[3], st));
            double* const host[3] = {lrt, lam, p};
            const double* const dev[3] = {h->d_lrtm.p, h->d_lamm.p, h->d_pm.p};
            for (int a = 0; a < 3; a++)
                if (host[a]) KGWAS_HIP(hipMemcpyAsync(&h->h_outm[a * cnt], dev[a], cnt * sizeof(double), hipMemcpyDeviceToHost, st));
            KGWAS_HIP(hipStreamSynchronize(st));
            for (int k = 0; k < 2; k++) KGWAS_HIP(hipEventElapsedTime(&ms[k], h->ev[k + 1], h->ev[k + 2]));
            h->st.grid_ms += ms[0];
            h->st.refine_ms += ms[1];
            for (int a = 0; a < 3; a++)
                if (host[a])
                    for (uint32_t k = 0; k < pb; k++)
                        memcpy(host[a] + (uint64_t)(p0 + k) * nv + pos, &h->h_outm[a * cnt + (uint64_t)k * c], c * sizeof(double));
        }
        h->st.chunks++;
        for (uint32_t v = 0; v < c; v++) {
            if (af) af[pos + v] = vars[v].af;
            if (n_miss) n_miss[pos + v] = vars[v].n_miss;
            if (tested) tested[pos + v] = (uint8_t)vars[v].tested;
            h->st.variants_tested += (uint64_t)vars[v].tested * n_pheno;
        }
        h->st.variants_read += c;
    }
}

// ---- the k-mers table route ----

struct TableHit {  // one tested row's result
    double lrt, lam, p, af;
    uint64_t row, kmer;
};
// a ranks before b: the larger lrt, then the smaller table row (a NaN lrt ranks last). Rows are unique, so the order is total.
bool ranks_before(const TableHit& a, const TableHit& b) {
    const double ka = std::isnan(a.lrt) ? -INFINITY : a.lrt, kb = std::isnan(b.lrt) ? -INFINITY : b.lrt;
    return ka != kb ? ka > kb : a.row < b.row;
}

// offers a result to a heap of at most best_n with the worst kept result on top
void heap_offer(std::vector<TableHit>& heap, uint64_t best_n, const TableHit& hit) {
    auto worse_on_top = [](const TableHit& a, const TableHit& b) { return ranks_before(a, b); };
    if (heap.size() < best_n) {
        heap.push_back(hit);
        std::push_heap(heap.begin(), heap.end(), worse_on_top);
    } else if (ranks_before(hit, heap.front())) {
        std::pop_heap(heap.begin(), heap.end(), worse_on_top);
        heap.back() = hit;
        std::push_heap(heap.begin(), heap.end(), worse_on_top);
    }
}

void sort_by_row(std::vector<TableHit>& heap) {
    std::sort(heap.begin(), heap.end(), [](const TableHit& a, const TableHit& b) { return a.row < b.row; });
}

// What test_table and test_table_multi share: the checks, the pieces and the front end. A reader thread fills two pinned row
// buffers in turn while the device works on the piece before; per piece the rows are squeezed, flagged and compacted
// (lmm_table_kernels.hip). prepare() runs after the checks and before any device work (the null models); per_piece(total, codes,
// vars, row, kmer) gets a piece's compacted tested rows on the device, total > 0 of them, and is done with them when it returns.
// `who` starts the messages; a tested row counts `weight` times in the stats' variants_tested.
template <class Prepare, class PerPiece>
void table_pass(kgwas_lmm* h, kgwas_table* t, const uint64_t* col, uint64_t n_acc, uint64_t min_count, double maf, uint64_t best_n,
                const std::string& who, uint64_t weight, Prepare prepare, PerPiece per_piece, uint64_t& rows_read, uint64_t& rows_tested) {
    if (n_acc != h->n) throw Error(KGWAS_ERR_ARG, who + ": n_acc differs from the handle's number of individuals");
    if (!best_n) throw Error(KGWAS_ERR_ARG, who + ": best_n is 0");
    uint64_t S_f = 0, n_rows = 0, W_f = 0;
    uint32_t klen = 0;
    if (kgwas_table_info(t, &S_f, &n_rows, &W_f, &klen) != KGWAS_OK) throw Error(KGWAS_ERR_ARG, kgwas_last_error());
    const uint64_t S = n_acc;
    for (uint64_t i = 0; i < S; i++)
        if (col[i] >= S_f) throw Error(KGWAS_ERR_ARG, who + ": column index out of range");
    check_squeeze_fits(who.c_str(), S_f, S);  // (before any allocation)
    prepare();
    KGWAS_HIP(hipSetDevice(h->device));
    const uint32_t W_m = (uint32_t)(2 * ((S + 127) / 128));
    const uint64_t stride = 1 + W_f;
    uint64_t piece = std::max<uint64_t>(1024, std::min<uint64_t>(1u << 18, (64ull << 20) / (8 * stride)));
    const long long forced = opt_int("KGWAS_LMM_PIECE_ROWS", 0);
    if (forced > 0) piece = (uint64_t)std::min<long long>(forced, 1 << 20);
    piece = std::min(piece, std::max<uint64_t>(n_rows, 1));
    const uint64_t n_blocks = (piece + LMM_TABLE_BLOCK - 1) / LMM_TABLE_BLOCK;

    std::vector<uint32_t> colmap(64ull * W_m, 0xFFFFFFFFu);
    for (uint64_t i = 0; i < S; i++) colmap[i] = (uint32_t)col[i];
    DevBuf<uint32_t> d_colmap, d_sq, d_n1flag, d_bcnt, d_boff, d_total;
    DevBuf<uint64_t> d_rows, d_row, d_kmer;
    DevBuf<uint8_t> d_codes;
    DevBuf<LmmVariant> d_vars;
    PinBuf<uint64_t> h_rows[2];
    upload(d_colmap, colmap);
    d_rows.alloc(piece * stride);
    d_sq.alloc(piece * 2 * W_m);
    d_n1flag.alloc(piece);
    d_bcnt.alloc(n_blocks);
    d_boff.alloc(n_blocks);
    d_total.alloc(1);
    d_codes.alloc(piece * h->dm.bpsp);
    d_vars.alloc(piece);
    d_row.alloc(piece);
    d_kmer.alloc(piece);
    for (PinBuf<uint64_t>& b : h_rows) b.alloc(piece * stride);
    hipEvent_t fe[2] = {nullptr, nullptr};  // around a piece's front end
    struct EventGuard {
        hipEvent_t* e;
        ~EventGuard() {
            for (int k = 0; k < 2; k++)
                if (e[k]) (void)hipEventDestroy(e[k]);
        }
    } eg{fe};
    for (hipEvent_t& e : fe) KGWAS_HIP(hipEventCreate(&e));

    // the reader: piece k goes into buffer k & 1 once piece k - 2 has left it
    const uint64_t n_pieces = (n_rows + piece - 1) / piece;
    std::mutex mu;
    std::condition_variable cv;
    uint64_t filled = 0, consumed = 0;
    bool stop = false;
    std::exception_ptr rerr;
    std::thread reader([&] {
        kgwas_name_this_thread("kgwas-lmm-read");
        try {
            for (uint64_t k = 0; k < n_pieces; k++) {
                {
                    std::unique_lock<std::mutex> lk(mu);
                    cv.wait(lk, [&] { return stop || consumed + 2 > k; });
                    if (stop) return;
                }
                const uint64_t pos = k * piece;
                if (kgwas_table_read_rows(t, pos, std::min(piece, n_rows - pos), h_rows[k & 1].p) != KGWAS_OK)
                    throw Error(KGWAS_ERR_IO, kgwas_last_error());
                {
                    std::unique_lock<std::mutex> lk(mu);
                    filled = k + 1;
                }
                cv.notify_all();
            }
        } catch (...) {
            std::unique_lock<std::mutex> lk(mu);
            rerr = std::current_exception();
            stop = true;
            cv.notify_all();
        }
    });
    struct ReaderJoin {
        std::thread& t;
        std::mutex& mu;
        std::condition_variable& cv;
        bool& stop;
        ~ReaderJoin() {
            {
                std::unique_lock<std::mutex> lk(mu);
                stop = true;
            }
            cv.notify_all();
            if (t.joinable()) t.join();
        }
    } rj{reader, mu, cv, stop};

    hipStream_t st = h->stream;
    rows_read = rows_tested = 0;
    for (uint64_t k = 0; k < n_pieces; k++) {
        const uint64_t pos = k * piece, c = std::min(piece, n_rows - pos);
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return stop || filled > k; });
            if (filled <= k) break;  // (the reader failed)
        }
        uint32_t total = 0;
        KGWAS_HIP(hipMemcpyAsync(d_rows.p, h_rows[k & 1].p, c * stride * 8, hipMemcpyHostToDevice, st));
        KGWAS_HIP(hipEventRecord(fe[0], st));
        KGWAS_HIP(launch_squeeze(d_rows.p, stride, c, d_colmap.p, W_m, (uint32_t)W_f, d_sq.p, st));
        KGWAS_HIP(launch_lmm_table_front(d_rows.p, stride, d_sq.p, (uint32_t)c, W_m, h->dm, pos, (uint32_t)std::min<uint64_t>(min_count, 0xFFFFFFFFu),
                                         maf, d_n1flag.p, d_bcnt.p, d_boff.p, d_total.p, d_codes.p, d_vars.p, d_row.p, d_kmer.p, st));
        KGWAS_HIP(hipEventRecord(fe[1], st));
        KGWAS_HIP(hipMemcpyAsync(&total, d_total.p, sizeof(total), hipMemcpyDeviceToHost, st));
        KGWAS_HIP(hipStreamSynchronize(st));
        {
            std::unique_lock<std::mutex> lk(mu);  // the rows are on the device: the buffer goes back to the reader
            consumed = k + 1;
        }
        cv.notify_all();
        float fms = 0;
        KGWAS_HIP(hipEventElapsedTime(&fms, fe[0], fe[1]));
        h->st.rotate_ms += fms;
        if (total > c) throw Error(KGWAS_ERR_STATE, who + ": the front end counted more tested rows than rows");
        if (total) per_piece(total, (const uint8_t*)d_codes.p, (const LmmVariant*)d_vars.p, (const uint64_t*)d_row.p, (const uint64_t*)d_kmer.p);
        rows_read += c;
        rows_tested += total;
        h->st.variants_read += c;
        h->st.variants_tested += total * weight;
    }
    if (rerr) std::rethrow_exception(rerr);
}

// Every row of table t against y: the best best_n tested rows by lrt, in table row order. The compacted rows of a piece go
// through rotate, grid and refine in sub-chunks of at most h->chunk. The host keeps a heap of best_n results with the worst on top.
void test_table(kgwas_lmm* h, const double* y, kgwas_table* t, const uint64_t* col, uint64_t n_acc, uint64_t min_count, double maf,
                uint64_t best_n, std::vector<TableHit>& kept, uint64_t& rows_read, uint64_t& rows_tested) {
    const uint64_t chunk = h->chunk;
    std::vector<TableHit> heap;
    std::vector<double> o_lrt, o_lam, o_p;
    std::vector<LmmVariant> o_vars;
    std::vector<uint64_t> o_row, o_kmer;
    auto prepare = [&] {
        fit_null(h, y);
        heap.reserve((size_t)std::min<uint64_t>(best_n, 1u << 20));
        o_lrt.resize(chunk), o_lam.resize(chunk), o_p.resize(chunk), o_vars.resize(chunk), o_row.resize(chunk), o_kmer.resize(chunk);
    };
    auto per_piece = [&](uint32_t total, const uint8_t* d_codes, const LmmVariant* d_vars, const uint64_t* d_row, const uint64_t* d_kmer) {
        hipStream_t st = h->stream;
        for (uint64_t sub = 0; sub < total; sub += chunk) {
            const uint32_t cc = (uint32_t)std::min<uint64_t>(chunk, total - sub);
            const uint8_t* codes = d_codes + sub * h->dm.bpsp;
            const LmmVariant* vars = d_vars + sub;
            KGWAS_HIP(hipEventRecord(h->ev[0], st));
            KGWAS_HIP(launch_lmm_rotate(codes, vars, cc, h->dm, h->d_U.p, h->d_Xt.p, st));
            KGWAS_HIP(hipEventRecord(h->ev[1], st));
            KGWAS_HIP(launch_lmm_grid(h->d_Xt.p, cc, h->dm, h->d_wt.p, h->d_yt.p, h->d_HB.p, h->d_G.p, st));
            KGWAS_HIP(hipEventRecord(h->ev[2], st));
            KGWAS_HIP(launch_lmm_refine(h->d_Xt.p, h->d_G.p, vars, cc, h->dm, h->d_d.p, h->d_wt.p, h->d_yt.p, h->d_grid.p, h->d_base.p, h->l0,
                                        h->d_lrt.p, h->d_lam.p, h->d_p.p, st));
            KGWAS_HIP(hipEventRecord(h->ev[3], st));
            KGWAS_HIP(hipMemcpyAsync(o_lrt.data(), h->d_lrt.p, cc * sizeof(double), hipMemcpyDeviceToHost, st));
            KGWAS_HIP(hipMemcpyAsync(o_lam.data(), h->d_lam.p, cc * sizeof(double), hipMemcpyDeviceToHost, st));
            KGWAS_HIP(hipMemcpyAsync(o_p.data(), h->d_p.p, cc * sizeof(double), hipMemcpyDeviceToHost, st));
            KGWAS_HIP(hipMemcpyAsync(o_vars.data(), vars, cc * sizeof(LmmVariant), hipMemcpyDeviceToHost, st));
            KGWAS_HIP(hipMemcpyAsync(o_row.data(), d_row + sub, cc * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
            KGWAS_HIP(hipMemcpyAsync(o_kmer.data(), d_kmer + sub, cc * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
            KGWAS_HIP(hipStreamSynchronize(st));
            float ms[3] = {0, 0, 0};
            for (int e = 0; e < 3; e++) KGWAS_HIP(hipEventElapsedTime(&ms[e], h->ev[e], h->ev[e + 1]));
            h->st.rotate_ms += ms[0];
            h->st.grid_ms += ms[1];
            h->st.refine_ms += ms[2];
            h->st.chunks++;
            for (uint32_t v = 0; v < cc; v++) heap_offer(heap, best_n, TableHit{o_lrt[v], o_lam[v], o_p[v], o_vars[v].af, o_row[v], o_kmer[v]});
        }
    };
    table_pass(h, t, col, n_acc, min_count, maf, best_n, "kgwas_lmm_test_table", 1, prepare, per_piece, rows_read, rows_tested);
    sort_by_row(heap);
    kept.swap(heap);
}

// The same for n_pheno columns Y[n_pheno][n] in one pass over the table: the best best_n per column, each with the rows and the
// bits test_table gives for that column alone. Per sub-chunk the rotation and the grid sums without y run once; per block of
// LMM_PBLOCK columns the xt yt sums, the refinement and the select kernel, which hands the host only the (column, row) pairs that
// can still enter the column's heap: all of them while the heap is not full, then those with lrt above the heap's worst as the
// host knew it before the launch. The heaps still decide; the per-row arrays stay on the device.
void test_table_multi(kgwas_lmm* h, uint32_t n_pheno, const double* Y, kgwas_table* t, const uint64_t* col, uint64_t n_acc,
                      uint64_t min_count, double maf, uint64_t best_n, std::vector<std::vector<TableHit>>& kept, double* logl0,
                      double* lambda0, uint64_t& rows_read, uint64_t& rows_tested, uint64_t& pairs_shipped) {
    const std::string who = "kgwas_lmm_test_table_multi";
    if (!n_pheno) throw Error(KGWAS_ERR_ARG, who + ": n_pheno is 0");  // (before the table's checks)
    const uint64_t chunk = h->chunk, ldi = h->dm.ldi, cap = (uint64_t)LMM_PBLOCK * chunk;
    const bool select = opt_int("KGWAS_LMM_TABLE_SELECT", 1) != 0;
    std::vector<std::vector<TableHit>> heaps(n_pheno);
    hipEvent_t se[3] = {nullptr, nullptr, nullptr};  // around a sub-chunk's rotation and shared grid sums
    struct EventGuard {
        hipEvent_t* e;
        ~EventGuard() {
            for (int k = 0; k < 3; k++)
                if (e[k]) (void)hipEventDestroy(e[k]);
        }
    } eg{se};
    pairs_shipped = 0;
    auto prepare = [&] {
        multi_prepare(h, n_pheno, Y, logl0, lambda0, who.c_str());
        if (!h->select_ready) {
            const uint64_t n_blocks = (cap + LMM_TABLE_BLOCK - 1) / LMM_TABLE_BLOCK;
            h->d_sel_cnt.alloc(n_blocks);
            h->d_sel_off.alloc(n_blocks);
            h->d_sel_total.alloc(1);
            h->d_sel_cols.alloc(LMM_PBLOCK);
            h->d_sel_rec.alloc(cap);
            h->h_sel_rec.alloc(cap);
            h->select_ready = true;
        }
        for (hipEvent_t& e : se) KGWAS_HIP(hipEventCreate(&e));
        for (std::vector<TableHit>& hp : heaps) hp.reserve((size_t)std::min<uint64_t>(best_n, 1u << 14));
    };
    auto per_piece = [&](uint32_t total, const uint8_t* d_codes, const LmmVariant* d_vars, const uint64_t* d_row, const uint64_t* d_kmer) {
        hipStream_t st = h->stream;
        for (uint64_t sub = 0; sub < total; sub += chunk) {
            const uint32_t cc = (uint32_t)std::min<uint64_t>(chunk, total - sub);
            const LmmVariant* vars = d_vars + sub;
            KGWAS_HIP(hipEventRecord(se[0], st));
            KGWAS_HIP(launch_lmm_rotate(d_codes + sub * h->dm.bpsp, vars, cc, h->dm, h->d_U.p, h->d_Xt.p, st));
            KGWAS_HIP(hipEventRecord(se[1], st));
            KGWAS_HIP(launch_lmm_grid_shared(h->d_Xt.p, cc, h->dm, h->d_wt.p, h->d_HB.p, h->d_Gx.p, st));
            KGWAS_HIP(hipEventRecord(se[2], st));
            for (uint32_t p0 = 0; p0 < n_pheno; p0 += LMM_PBLOCK) {
                const uint32_t pb = std::min(LMM_PBLOCK, n_pheno - p0);
                const double* Ytb = h->d_Ytm.p + (uint64_t)p0 * ldi;
                // what the host knows of the block's heaps now; a NaN lrt ranks as -inf (ranks_before)
                LmmSelectCol sc[LMM_PBLOCK];
                for (uint32_t k = 0; k < pb; k++) {
                    const std::vector<TableHit>& hp = heaps[p0 + k];
                    const bool open = !select || hp.size() < best_n;
                    const double worst = open ? 0.0 : hp.front().lrt;
                    sc[k] = LmmSelectCol{std::isnan(worst) ? -INFINITY : worst, open ? 1u : 0u, 0u};
                }
                KGWAS_HIP(hipMemcpyAsync(h->d_sel_cols.p, sc, pb * sizeof(LmmSelectCol), hipMemcpyHostToDevice, st));
                KGWAS_HIP(hipEventRecord(h->ev[1], st));
                KGWAS_HIP(launch_lmm_grid_xy(h->d_Xt.p, cc, h->dm, Ytb, pb, h->d_HB.p, h->d_Gxy.p, st));
                KGWAS_HIP(hipEventRecord(h->ev[2], st));
                KGWAS_HIP(launch_lmm_refine_multi(h->d_Xt.p, h->d_Gx.p, h->d_Gxy.p, vars, cc, h->dm, h->d_d.p, h->d_wt.p, Ytb, pb, h->d_grid.p,
                                                  h->d_basem.p + (uint64_t)p0 * LMM_GRID * LMM_BASE, h->d_nullm.p + 2 * (uint64_t)p0,
                                                  h->d_lrtm.p, h->d_lamm.p, h->d_pm.p, st));
                KGWAS_HIP(launch_lmm_table_select(h->d_lrtm.p, h->d_lamm.p, h->d_pm.p, cc, pb, vars, d_row + sub, d_kmer + sub, h->d_sel_cols.p,
                                                  h->d_sel_cnt.p, h->d_sel_off.p, h->d_sel_total.p, h->d_sel_rec.p, (uint32_t)cap, st));
                KGWAS_HIP(hipEventRecord(h->ev[3], st));
                uint32_t count = 0;
                KGWAS_HIP(hipMemcpyAsync(&count, h->d_sel_total.p, sizeof(count), hipMemcpyDeviceToHost, st));
                KGWAS_HIP(hipStreamSynchronize(st));  // (sc is read by the copy until here)
                if (count > (uint64_t)pb * cc) throw Error(KGWAS_ERR_STATE, who + ": the select kernel counted more survivors than pairs");
                if (count) {
                    KGWAS_HIP(hipMemcpyAsync(h->h_sel_rec.p, h->d_sel_rec.p, count * sizeof(LmmTableRecord), hipMemcpyDeviceToHost, st));
                    KGWAS_HIP(hipStreamSynchronize(st));
                }
                float ms[2] = {0, 0};
                if (p0 == 0) {
                    for (int e = 0; e < 2; e++) KGWAS_HIP(hipEventElapsedTime(&ms[e], se[e], se[e + 1]));
                    h->st.rotate_ms += ms[0];
                    h->st.grid_ms += ms[1];
                }
                for (int e = 0; e < 2; e++) KGWAS_HIP(hipEventElapsedTime(&ms[e], h->ev[e + 1], h->ev[e + 2]));
                h->st.grid_ms += ms[0];
                h->st.refine_ms += ms[1];
                for (uint32_t r = 0; r < count; r++) {
                    const LmmTableRecord& o = h->h_sel_rec.p[r];
                    if (o.col >= pb) throw Error(KGWAS_ERR_STATE, who + ": a survivor record names a column outside its block");
                    heap_offer(heaps[p0 + o.col], best_n, TableHit{o.lrt, o.lam, o.p, o.af, o.row, o.kmer});
                }
                pairs_shipped += count;
            }
            h->st.chunks++;
        }
    };
    table_pass(h, t, col, n_acc, min_count, maf, best_n, who, n_pheno, prepare, per_piece, rows_read, rows_tested);
    for (std::vector<TableHit>& hp : heaps) sort_by_row(hp);
    kept.swap(heaps);
}

kgwas_lmm* create(uint64_t n, const double* K, int device, double lmin, double lmax, uint64_t chunk_variants) {
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

// ---- files ----

std::vector<std::string> split_ws(const std::string& line) {
    std::vector<std::string> f;
    size_t i = 0;
    while (i < line.size()) {
        while (i < line.size() && (line[i] == ' ' || line[i] == '\t' || line[i] == '\r')) i++;
        size_t j = i;
        while (j < line.size() && line[j] != ' ' && line[j] != '\t' && line[j] != '\r') j++;
        if (j > i) f.push_back(line.substr(i, j - i));
        i = j;
    }
    return f;
}

std::vector<std::string> read_lines(const std::string& path, const char* what) {
    std::ifstream f(path);
    if (!f.is_open()) throw Error(KGWAS_ERR_IO, std::string("can't open ") + what + " file: " + path);
    std::vector<std::string> lines;
    for (std::string l; std::getline(f, l);)
        if (l.find_first_not_of(" \t\r") != std::string::npos) lines.push_back(l);
    return lines;
}

std::vector<double> read_kinship(const std::string& path, uint64_t n_expected, const char* counted_in = "the .fam") {
    const std::vector<std::string> lines = read_lines(path, "kinship");
    if (lines.size() != n_expected)
        throw Error(KGWAS_ERR_FORMAT, "kinship file " + path + " has " + std::to_string(lines.size()) + " rows, " + counted_in + " has " +
                                          std::to_string(n_expected) + " individuals");
    std::vector<double> K(n_expected * n_expected);
    for (uint64_t r = 0; r < n_expected; r++) {
        const char* s = lines[r].c_str();
        uint64_t c = 0;
        for (;; c++) {
            char* end = nullptr;
            const double v = strtod(s, &end);
            if (end == s) break;
            if (c < n_expected) K[r * n_expected + c] = v;
            s = end;
        }
        while (*s == ' ' || *s == '\t' || *s == '\r') s++;
        if (*s) throw Error(KGWAS_ERR_FORMAT, "kinship file " + path + ": row " + std::to_string(r + 1) + " holds text that is no number");
        if (c != n_expected)
            throw Error(KGWAS_ERR_FORMAT, "kinship file " + path + ": row " + std::to_string(r + 1) + " has " + std::to_string(c) +
                                              " values, expected " + std::to_string(n_expected));
    }
    return K;
}

// values[i] and keep[i] of every .fam line; the phenotype is field 5 + pheno_col (1-based), "-9" and "NA" are missing
void read_fam(const std::string& path, uint32_t pheno_col, std::vector<double>& values, std::vector<uint8_t>& keep) {
    if (pheno_col < 1) throw Error(KGWAS_ERR_ARG, "the phenotype column (-n) starts at 1");
    const std::vector<std::string> lines = read_lines(path, "fam");
    values.assign(lines.size(), std::nan(""));
    keep.assign(lines.size(), 0);
    for (size_t i = 0; i < lines.size(); i++) {
        const std::vector<std::string> f = split_ws(lines[i]);
        if (f.size() < 5u + pheno_col)
            throw Error(KGWAS_ERR_FORMAT, path + ": line " + std::to_string(i + 1) + " has no phenotype column " + std::to_string(pheno_col));
        const std::string& t = f[4 + pheno_col];
        if (t == "-9" || t == "NA") continue;
        char* end = nullptr;
        const double v = strtod(t.c_str(), &end);
        if (end == t.c_str() || *end || !std::isfinite(v))
            throw Error(KGWAS_ERR_FORMAT, path + ": line " + std::to_string(i + 1) + ": phenotype '" + t + "' is no number");
        values[i] = v;
        keep[i] = 1;
    }
}

uint64_t format_assoc(const char* chr, const char* rs, const char* ps, uint32_t n_miss, const char* a1, const char* a0, double af,
                      double l_mle, double p, char* out, uint64_t cap) {
    char buf[1024];
    int len;
    if (!chr)
        len = snprintf(buf, sizeof(buf), "chr\trs\tps\tn_miss\tallele1\tallele0\taf\tl_mle\tp_lrt\n");
    else
        len = snprintf(buf, sizeof(buf), "%s\t%s\t%s\t%u\t%s\t%s\t%.3f\t%.6e\t%.6e\n", chr, rs, ps, n_miss, a1, a0, af, l_mle, p);
    if (len < 0 || (size_t)len >= sizeof(buf)) throw Error(KGWAS_ERR_FORMAT, "a .bim line is too long");
    if (out && cap >= (uint64_t)len) memcpy(out, buf, (size_t)len);
    return (uint64_t)len;
}

std::string log_path_of(const std::string& out) {
    const std::string suf = ".assoc.txt";
    if (out.size() >= suf.size() && out.compare(out.size() - suf.size(), suf.size(), suf) == 0)
        return out.substr(0, out.size() - suf.size()) + ".log.txt";
    return out + ".log.txt";
}

void add_stats(kgwas_lmm_stats& a, const kgwas_lmm_stats& b) {
    a.eigen_ms += b.eigen_ms;
    a.rotate_ms += b.rotate_ms;
    a.grid_ms += b.grid_ms;
    a.refine_ms += b.refine_ms;
    a.variants_read += b.variants_read;
    a.variants_tested += b.variants_tested;
    a.chunks += b.chunks;
    a.eigendecompositions += b.eigendecompositions;
    a.n_individuals = b.n_individuals;
}

// ---- what run_files and run_file_multi share ----

std::vector<uint32_t> kept_lines(const std::vector<uint8_t>& keep) {
    std::vector<uint32_t> idx;
    for (uint64_t i = 0; i < keep.size(); i++)
        if (keep[i]) idx.push_back((uint32_t)i);
    return idx;
}

kgwas_lmm* create_for_kept(const std::vector<double>& Kfull, uint64_t nf, const std::vector<uint32_t>& idx, int device, double lmin,
                           double lmax, uint64_t chunk_variants) {
    const uint64_t n = idx.size();
    std::vector<double> K(n * n);
    for (uint64_t r = 0; r < n; r++)
        for (uint64_t c = 0; c < n; c++) K[r * n + c] = Kfull[(uint64_t)idx[r] * nf + idx[c]];
    return create(n, K.data(), device, lmin, lmax, chunk_variants);
}

// the .bim lines and the .bed body of <base>, the latter with the codes of the kept individuals idx (of nf .fam lines) alone
void read_bim_bed(const std::string& base, uint64_t nf, const std::vector<uint32_t>& idx, std::vector<std::string>& bim,
                  std::vector<uint8_t>& body) {
    bim = read_lines(base + ".bim", "bim");
    const uint64_t n = idx.size(), M = bim.size(), bps_f = (nf + 3) / 4, bps = (n + 3) / 4;
    {
        std::ifstream f(base + ".bed", std::ios::binary | std::ios::ate);
        if (!f.is_open()) throw Error(KGWAS_ERR_IO, "can't open bed file: " + base + ".bed");
        const uint64_t size = (uint64_t)f.tellg();
        if (size != 3 + M * bps_f)
            throw Error(KGWAS_ERR_FORMAT, base + ".bed has " + std::to_string(size) + " bytes, " + std::to_string(M) + " variants of " +
                                              std::to_string(nf) + " individuals need " + std::to_string(3 + M * bps_f));
        f.seekg(0);
        uint8_t magic[3];
        f.read((char*)magic, 3);
        if (magic[0] != 0x6C || magic[1] != 0x1B || magic[2] != 0x01)
            throw Error(KGWAS_ERR_FORMAT, base + ".bed: not a SNP-major PLINK .bed (magic 6C 1B 01)");
        body.resize(M * bps_f);
        f.read((char*)body.data(), (std::streamsize)body.size());
        if (!f) throw Error(KGWAS_ERR_IO, "short read of " + base + ".bed");
    }
    if (n != nf) {  // the kept individuals' codes, packed again
        std::vector<uint8_t> packed(M * bps, 0);
        for (uint64_t v = 0; v < M; v++) {
            const uint8_t* src = &body[v * bps_f];
            uint8_t* dst = &packed[v * bps];
            for (uint64_t r = 0; r < n; r++) dst[r >> 2] |= (uint8_t)(((src[idx[r] >> 2] >> (2 * (idx[r] & 3))) & 3) << (2 * (r & 3)));
        }
        body.swap(packed);
    }
}

std::string assoc_header() {
    std::string text(format_assoc(nullptr, "", "", 0, "", "", 0, 0, 0, nullptr, 0), '\0');
    format_assoc(nullptr, "", "", 0, "", "", 0, 0, 0, &text[0], text.size());
    return text;
}

// the fields of the .bim lines of the tested ones among variants first .. first + cnt (tested starts at `first`; the others stay empty)
std::vector<std::vector<std::string>> bim_fields(const std::string& base, const std::vector<std::string>& bim, uint64_t first, uint64_t cnt,
                                                 const uint8_t* tested) {
    std::vector<std::vector<std::string>> fields(cnt);
    for (uint64_t v = 0; v < cnt; v++) {
        if (!tested[v]) continue;
        fields[v] = split_ws(bim[first + v]);
        if (fields[v].size() < 6)
            throw Error(KGWAS_ERR_FORMAT, base + ".bim: line " + std::to_string(first + v + 1) + " has fewer than 6 fields");
    }
    return fields;
}

// appends the lines of the tested ones among fields.size() variants (all arrays start at the first of them); returns their number
uint64_t append_assoc(std::string& text, const std::vector<std::vector<std::string>>& fields, const uint32_t* n_miss, const double* af,
                      const double* lam, const double* p, const uint8_t* tested) {
    uint64_t n_tested = 0;
    for (uint64_t v = 0; v < fields.size(); v++) {
        if (!tested[v]) continue;
        const std::vector<std::string>& f = fields[v];
        char line[1024];
        const uint64_t len = format_assoc(f[0].c_str(), f[1].c_str(), f[3].c_str(), n_miss[v], f[4].c_str(), f[5].c_str(), af[v], lam[v],
                                          p[v], line, sizeof(line));
        text.append(line, len);
        n_tested++;
    }
    return n_tested;
}

void write_text(const std::string& path, const std::string& text, const char* mode) {
    FILE* fo = fopen(path.c_str(), mode);
    const bool ok = fo && fwrite(text.data(), 1, text.size(), fo) == text.size();
    if ((fo && fclose(fo) != 0) || !ok) throw Error(KGWAS_ERR_IO, "can't write " + path);
}

void write_log(const std::string& out, const std::string& base, const char* kinship_path, uint64_t nf, uint64_t n, uint64_t M,
               uint64_t n_tested, double lambda0, double l0, double eigen_ms, double rotate_ms, double grid_ms, double refine_ms,
               double total_ms) {
    char log[1024];
    const int ll = snprintf(log, sizeof(log),
                            "lmm_lrt: ML likelihood-ratio test (-lmm 2)\nbfile\t%s\nkinship\t%s\nindividuals_in_fam\t%llu\n"
                            "individuals_used\t%llu\nvariants_read\t%llu\nvariants_tested\t%llu\nlambda0\t%.6e\nlogl_H0\t%.6f\n"
                            "ms: eigen=%.3f rotate=%.3f grid=%.3f refine=%.3f total=%.3f\n",
                            base.c_str(), kinship_path, (unsigned long long)nf, (unsigned long long)n, (unsigned long long)M,
                            (unsigned long long)n_tested, lambda0, l0, eigen_ms, rotate_ms, grid_ms, refine_ms, total_ms);
    FILE* fl = fopen(log_path_of(out).c_str(), "wb");
    if (!fl || ll < 0 || fwrite(log, 1, (size_t)std::min<int>(ll, sizeof(log) - 1), fl) == 0 || fclose(fl) != 0)
        throw Error(KGWAS_ERR_IO, "can't write " + log_path_of(out));
}

void run_files(const char* kinship_path, uint64_t n_beds, const char* const* bases, const char* const* outs, uint32_t pheno_col,
               double maf, double miss, double lmin, double lmax, uint64_t chunk_variants, int device, kgwas_lmm_stats* total) {
    if (!kinship_path || (n_beds && (!bases || !outs))) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_run_files: null argument");
    kgwas_lmm_stats sum{};
    std::vector<double> Kfull;
    std::unique_ptr<kgwas_lmm> h;
    std::vector<uint8_t> keep_cur;
    for (uint64_t b = 0; b < n_beds; b++) {
        const std::string base = bases[b], out = outs[b];
        const double t_start = now_ms();
        std::vector<double> vals;
        std::vector<uint8_t> keep;
        read_fam(base + ".fam", pheno_col, vals, keep);
        const uint64_t nf = vals.size();
        if (Kfull.empty() || Kfull.size() != nf * nf) Kfull = read_kinship(kinship_path, nf);
        const std::vector<uint32_t> idx = kept_lines(keep);
        const uint64_t n = idx.size();
        if (!h || keep != keep_cur) {
            if (h) add_stats(sum, h->st);
            h.reset();
            h.reset(create_for_kept(Kfull, nf, idx, device, lmin, lmax, chunk_variants));
            keep_cur = keep;
        }
        std::vector<double> y(n);
        for (uint64_t r = 0; r < n; r++) y[r] = vals[idx[r]];
        std::vector<std::string> bim;
        std::vector<uint8_t> body;
        read_bim_bed(base, nf, idx, bim, body);
        const uint64_t M = bim.size();
        std::vector<double> lrt(M), lam(M), p(M), af(M);
        std::vector<uint32_t> n_miss(M);
        std::vector<uint8_t> tested(M);
        const kgwas_lmm_stats before = h->st;
        test_bed(h.get(), y.data(), body.data(), M, maf, miss, lrt.data(), lam.data(), p.data(), af.data(), n_miss.data(), tested.data());
        std::string text = assoc_header();
        const uint64_t n_tested =
            append_assoc(text, bim_fields(base, bim, 0, M, tested.data()), n_miss.data(), af.data(), lam.data(), p.data(), tested.data());
        write_text(out, text, "wb");
        write_log(out, base, kinship_path, nf, n, M, n_tested, h->lambda0, h->l0, h->st.eigen_ms, h->st.rotate_ms - before.rotate_ms,
                  h->st.grid_ms - before.grid_ms, h->st.refine_ms - before.refine_ms, now_ms() - t_start);
    }
    if (h) add_stats(sum, h->st);
    if (total) *total = sum;
}

// One bfile, n_cols phenotype columns of its .fam with one missing set: the .bed, the .bim and the kinship matrix are read once,
// K is eigendecomposed once, and every chunk of variants goes through the multi-phenotype pass. Results are written in slabs
// of variants, so that the [column][variant] arrays stay small for a panel of millions of variants.
void run_file_multi(const char* kinship_path, const char* bfile_base, uint32_t n_cols, const uint32_t* cols, const char* const* outs,
                    double maf, double miss, double lmin, double lmax, uint64_t chunk_variants, int device, kgwas_lmm_stats* total) {
    if (!kinship_path || !bfile_base || !cols || !outs) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_run_file_multi: null argument");
    if (!n_cols) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_run_file_multi: no phenotype column given");
    const std::string base = bfile_base;
    const double t_start = now_ms();
    std::vector<std::vector<double>> vals(n_cols);
    std::vector<uint8_t> keep;
    for (uint32_t k = 0; k < n_cols; k++) {
        std::vector<uint8_t> keep_k;
        read_fam(base + ".fam", cols[k], vals[k], keep_k);
        if (k == 0)
            keep = keep_k;
        else if (keep_k != keep)
            throw Error(KGWAS_ERR_FORMAT, base + ".fam: phenotype column " + std::to_string(cols[k]) + " marks other individuals as missing than column " +
                                              std::to_string(cols[0]) + "; columns of one run must share their missing set");
    }
    const uint64_t nf = keep.size();
    const std::vector<double> Kfull = read_kinship(kinship_path, nf);
    const std::vector<uint32_t> idx = kept_lines(keep);
    const uint64_t n = idx.size();
    std::unique_ptr<kgwas_lmm> h(create_for_kept(Kfull, nf, idx, device, lmin, lmax, chunk_variants));
    std::vector<double> Y((uint64_t)n_cols * n);
    for (uint32_t k = 0; k < n_cols; k++)
        for (uint64_t r = 0; r < n; r++) Y[k * n + r] = vals[k][idx[r]];
    std::vector<std::string> bim;
    std::vector<uint8_t> body;
    read_bim_bed(base, nf, idx, bim, body);
    const uint64_t M = bim.size(), bps = (n + 3) / 4;
    std::vector<double> l0(n_cols), lambda0(n_cols);
    multi_prepare(h.get(), n_cols, Y.data(), l0.data(), lambda0.data());
    for (uint32_t k = 0; k < n_cols; k++) write_text(outs[k], assoc_header(), "wb");
    // a slab: whole chunks, about 4 M (variant, column) pairs
    const uint64_t slab = std::max<uint64_t>(1, (1u << 22) / ((uint64_t)n_cols * h->chunk)) * h->chunk;
    std::vector<double> lrt(std::min(slab, M) * n_cols), lam(lrt.size()), p(lrt.size()), af(std::min(slab, M));
    std::vector<uint32_t> n_miss(af.size());
    std::vector<uint8_t> tested(af.size());
    std::vector<uint64_t> n_tested(n_cols, 0);
    for (uint64_t first = 0; first < M; first += slab) {
        const uint64_t cnt = std::min(slab, M - first);
        multi_run(h.get(), n_cols, body.data() + first * bps, cnt, maf, miss, lrt.data(), lam.data(), p.data(), af.data(), n_miss.data(),
                  tested.data());
        const std::vector<std::vector<std::string>> fields = bim_fields(base, bim, first, cnt, tested.data());  // once for all columns
        for (uint32_t k = 0; k < n_cols; k++) {
            std::string text;
            n_tested[k] += append_assoc(text, fields, n_miss.data(), af.data(), &lam[k * cnt], &p[k * cnt], tested.data());
            write_text(outs[k], text, "ab");
        }
    }
    const double total_ms = now_ms() - t_start;
    for (uint32_t k = 0; k < n_cols; k++)  // (the kernels' times are the shared pass's, the same in every column's log)
        write_log(outs[k], base, kinship_path, nf, n, M, n_tested[k], lambda0[k], l0[k], h->st.eigen_ms, h->st.rotate_ms, h->st.grid_ms,
                  h->st.refine_ms, total_ms);
    if (total) *total = h->st;
}

// ---- what run_table and run_table_multi share ----

// The inputs of lmm_lrt --kmers_table, each read once: the phenotype file (its accessions, in its order, are the individuals), the
// open table with its column map, the kinship text.
struct TableRun {
    kgwas_pheno* ph = nullptr;
    kgwas_table* t = nullptr;
    std::string pheno_path;
    uint64_t n_pheno = 0, S = 0, min_count = 0;
    uint32_t klen = 0;
    std::vector<const char*> acc;
    const float* Y = nullptr;
    std::vector<uint64_t> col;
    std::vector<double> K;
    ~TableRun() {
        if (t) kgwas_table_close(t);
        if (ph) kgwas_pheno_free(ph);
    }
    static void ck(int rc) {
        if (rc != KGWAS_OK) throw Error(rc, kgwas_last_error());
    }
    void load_pheno(const char* path) {
        pheno_path = path;
        ck(kgwas_pheno_load(path, &ph));
        ck(kgwas_pheno_info(ph, &n_pheno, &S));
    }
    void need_column(uint32_t pheno_col) const {
        if (pheno_col > n_pheno) throw Error(KGWAS_ERR_FORMAT, pheno_path + " has no phenotype column " + std::to_string(pheno_col));
    }
    void load_values() {
        acc.resize(S);
        for (uint64_t i = 0; i < S; i++) ck(kgwas_pheno_accession(ph, i, &acc[i]));
        ck(kgwas_pheno_values(ph, &Y));
    }
    // y as it would arrive through kmers_table_to_bed's .fam: the loader's float in ostream's default format, parsed as read_fam does
    void column(uint32_t pheno_col, double* y) const {
        for (uint64_t i = 0; i < S; i++) {
            std::ostringstream os;
            os << Y[(uint64_t)(pheno_col - 1) * S + i];
            const std::string text = os.str();
            if (text == "-9" || text == "NA")
                throw Error(KGWAS_ERR_FORMAT, pheno_path + ": the phenotype of " + acc[i] + " is " + text +
                                                  ", which a .fam reads as missing; remove the accession from the phenotype file");
            char* end = nullptr;
            const double v = strtod(text.c_str(), &end);
            if (end == text.c_str() || *end || !std::isfinite(v))
                throw Error(KGWAS_ERR_FORMAT, pheno_path + ": phenotype '" + text + "' of " + acc[i] + " is no number");
            y[i] = v;
        }
    }
    void open_table(const char* table_base, uint32_t kmer_len, const char* kinship_path, double maf, uint64_t mac) {
        ck(kgwas_table_open(table_base, kmer_len, &t));
        col.resize(S);
        ck(kgwas_table_column_map(t, acc.data(), S, col.data()));
        uint64_t S_f = 0, n_rows = 0, W_f = 0;
        ck(kgwas_table_info(t, &S_f, &n_rows, &W_f, &klen));
        check_squeeze_fits("lmm_lrt --kmers_table", S_f, S);
        K = read_kinship(kinship_path, S, "the phenotype file");
        min_count = kgwas_min_count(S, maf, mac);
    }
};

// one column's kept k-mers to `out` in table order, with the bytes run_files writes for them after kmers_table_to_bed, and the log
void write_table_result(const std::string& out, const std::vector<TableHit>& kept, const TableRun& r, const char* table_base,
                        uint32_t pheno_col, const char* kinship_path, uint64_t rows_read, uint64_t rows_tested, uint64_t best_n,
                        double lambda0, double l0, const kgwas_lmm_stats& st, double total_ms) {
    std::string text = assoc_header();
    for (const TableHit& k : kept) {
        char km[33];
        for (uint32_t i = 0; i < r.klen; i++) km[i] = "ACGT"[(k.kmer >> (2 * (r.klen - 1 - i))) & 3];  // bits2kmer31, as kmers_table_to_bed's .bim
        km[r.klen] = 0;
        char line[1024];
        const uint64_t len = format_assoc("0", km, "0", 0, "0", "1", k.af, k.lam, k.p, line, sizeof(line));
        text.append(line, len);
    }
    write_text(out, text, "wb");
    char log[2048];
    const int ll = snprintf(log, sizeof(log),
                            "lmm_lrt: ML likelihood-ratio test (-lmm 2)\nkmers_table\t%s\nphenotypes\t%s\nphenotype_column\t%u\nkinship\t%s\n"
                            "individuals_used\t%llu\nmin_count\t%llu\nrows_read\t%llu\nrows_tested\t%llu\nrows_kept\t%llu\nbest_n\t%llu\n"
                            "lambda0\t%.6e\nlogl_H0\t%.6f\nms: eigen=%.3f rotate=%.3f grid=%.3f refine=%.3f total=%.3f\n",
                            table_base, r.pheno_path.c_str(), pheno_col, kinship_path, (unsigned long long)r.S, (unsigned long long)r.min_count,
                            (unsigned long long)rows_read, (unsigned long long)rows_tested, (unsigned long long)kept.size(),
                            (unsigned long long)best_n, lambda0, l0, st.eigen_ms, st.rotate_ms, st.grid_ms, st.refine_ms, total_ms);
    if (ll < 0) throw Error(KGWAS_ERR_IO, "can't write " + log_path_of(out));
    write_text(log_path_of(out), std::string(log, (size_t)std::min<int>(ll, sizeof(log) - 1)), "wb");
}

// The file layer of lmm_lrt --kmers_table: the accessions and their order are the phenotype file's, y its column pheno_col (from
// 1), the k-mers come straight from <table_base>.table. The best best_n k-mers by the exact test go to `out` in table order, with
// the bytes run_files writes for them after kmers_table_to_bed; a log goes beside it.
void run_table(const char* kinship_path, const char* table_base, uint32_t kmer_len, const char* pheno_path, uint32_t pheno_col,
               uint64_t mac, double maf, uint64_t best_n, double lmin, double lmax, uint64_t chunk_variants, int device, const char* out,
               kgwas_lmm_stats* total) {
    if (!kinship_path || !table_base || !pheno_path || !out) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_run_table: null argument");
    if (pheno_col < 1) throw Error(KGWAS_ERR_ARG, "the phenotype column (-n) starts at 1");
    if (!best_n) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_run_table: best_n is 0");
    const double t_start = now_ms();
    TableRun r;
    r.load_pheno(pheno_path);
    r.need_column(pheno_col);
    r.load_values();
    std::vector<double> y(r.S);
    r.column(pheno_col, y.data());
    r.open_table(table_base, kmer_len, kinship_path, maf, mac);
    std::unique_ptr<kgwas_lmm> h(create(r.S, r.K.data(), device, lmin, lmax, chunk_variants));
    std::vector<TableHit> kept;
    uint64_t rows_read = 0, rows_tested = 0;
    test_table(h.get(), y.data(), r.t, r.col.data(), r.S, r.min_count, maf, best_n, kept, rows_read, rows_tested);
    write_table_result(out, kept, r, table_base, pheno_col, kinship_path, rows_read, rows_tested, best_n, h->lambda0, h->l0, h->st,
                       now_ms() - t_start);
    if (total) *total = h->st;
}

// The same for n_cols columns of the phenotype file (pheno_cols, from 1) in ONE pass over the table: the files are read once, K is
// eigendecomposed once, and outs[k] with its log gets what run_table writes for column pheno_cols[k] (the kernels' times are the
// shared pass's, the same in every column's log).
void run_table_multi(const char* kinship_path, const char* table_base, uint32_t kmer_len, const char* pheno_path, uint32_t n_cols,
                     const uint32_t* cols, const char* const* outs, uint64_t mac, double maf, uint64_t best_n, double lmin, double lmax,
                     uint64_t chunk_variants, int device, kgwas_lmm_stats* total) {
    if (!kinship_path || !table_base || !pheno_path || !cols || !outs) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_run_table_multi: null argument");
    if (!n_cols) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_run_table_multi: no phenotype column given");
    for (uint32_t k = 0; k < n_cols; k++) {
        if (!outs[k]) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_run_table_multi: null argument");
        if (cols[k] < 1) throw Error(KGWAS_ERR_ARG, "phenotype columns start at 1");
    }
    if (!best_n) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_run_table_multi: best_n is 0");
    const double t_start = now_ms();
    TableRun r;
    r.load_pheno(pheno_path);
    for (uint32_t k = 0; k < n_cols; k++) r.need_column(cols[k]);
    r.load_values();
    std::vector<double> Y((uint64_t)n_cols * r.S);
    for (uint32_t k = 0; k < n_cols; k++) r.column(cols[k], &Y[k * r.S]);
    r.open_table(table_base, kmer_len, kinship_path, maf, mac);
    std::unique_ptr<kgwas_lmm> h(create(r.S, r.K.data(), device, lmin, lmax, chunk_variants));
    std::vector<std::vector<TableHit>> kept;
    std::vector<double> l0(n_cols), lambda0(n_cols);
    uint64_t rows_read = 0, rows_tested = 0, shipped = 0;
    test_table_multi(h.get(), n_cols, Y.data(), r.t, r.col.data(), r.S, r.min_count, maf, best_n, kept, l0.data(), lambda0.data(), rows_read,
                     rows_tested, shipped);
    const double total_ms = now_ms() - t_start;
    for (uint32_t k = 0; k < n_cols; k++)
        write_table_result(outs[k], kept[k], r, table_base, cols[k], kinship_path, rows_read, rows_tested, best_n, lambda0[k], l0[k], h->st,
                           total_ms);
    if (total) *total = h->st;
}

}  // namespace

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

int kgwas_lmm_test_bed_multi(kgwas_lmm* h, uint32_t n_pheno, const double* Y, const uint8_t* bed_body, uint64_t n_variants, double maf,
                             double miss, double* lrt, double* lambda, double* p, double* logl0, double* lambda0, double* af,
                             uint32_t* n_miss, uint8_t* tested) {
    return guarded([&] {
        if (!h || (!Y && n_pheno) || (!bed_body && n_variants)) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_test_bed_multi: null argument");
        multi_prepare(h, n_pheno, Y, logl0, lambda0);
        multi_run(h, n_pheno, bed_body, n_variants, maf, miss, lrt, lambda, p, af, n_miss, tested);
    });
}

int kgwas_lmm_run_file_multi(const char* kinship_path, const char* bfile_base, uint32_t n_cols, const uint32_t* pheno_cols,
                             const char* const* out_paths, double maf, double miss, double lmin, double lmax, uint64_t chunk_variants,
                             int32_t device, kgwas_lmm_stats* total) {
    return guarded([&] {
        run_file_multi(kinship_path, bfile_base, n_cols, pheno_cols, out_paths, maf, miss, lmin, lmax, chunk_variants, device, total);
    });
}

int kgwas_lmm_run_files(const char* kinship_path, uint64_t n_beds, const char* const* bfile_bases, const char* const* out_paths,
                        uint32_t pheno_col, double maf, double miss, double lmin, double lmax, uint64_t chunk_variants, int32_t device,
                        kgwas_lmm_stats* total) {
    return guarded([&] { run_files(kinship_path, n_beds, bfile_bases, out_paths, pheno_col, maf, miss, lmin, lmax, chunk_variants, device, total); });
}

int kgwas_lmm_test_table(kgwas_lmm* h, const double* y, kgwas_table* t, const uint64_t* col, uint64_t n_acc, uint64_t min_count, double maf,
                         uint64_t best_n, uint64_t* row, uint64_t* kmer, double* lrt, double* lambda, double* p, double* af,
                         uint64_t* n_kept, uint64_t* rows_read, uint64_t* rows_tested) {
    return guarded([&] {
        if (!h || !y || !t || !col) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_test_table: null argument");
        std::vector<TableHit> kept;
        uint64_t n_read = 0, n_tested = 0;
        test_table(h, y, t, col, n_acc, min_count, maf, best_n, kept, n_read, n_tested);
        for (uint64_t i = 0; i < kept.size(); i++) {
            if (row) row[i] = kept[i].row;
            if (kmer) kmer[i] = kept[i].kmer;
            if (lrt) lrt[i] = kept[i].lrt;
            if (lambda) lambda[i] = kept[i].lam;
            if (p) p[i] = kept[i].p;
            if (af) af[i] = kept[i].af;
        }
        if (n_kept) *n_kept = kept.size();
        if (rows_read) *rows_read = n_read;
        if (rows_tested) *rows_tested = n_tested;
    });
}

int kgwas_lmm_run_table(const char* kinship_path, const char* table_base, uint32_t kmer_len, const char* pheno_path, uint32_t pheno_col,
                        uint64_t mac, double maf, uint64_t best_n, double lmin, double lmax, uint64_t chunk_variants, int32_t device,
                        const char* out_path, kgwas_lmm_stats* total) {
    return guarded([&] {
        run_table(kinship_path, table_base, kmer_len, pheno_path, pheno_col, mac, maf, best_n, lmin, lmax, chunk_variants, device, out_path,
                  total);
    });
}

int kgwas_lmm_test_table_multi(kgwas_lmm* h, uint32_t n_pheno, const double* Y, kgwas_table* t, const uint64_t* col, uint64_t n_acc,
                               uint64_t min_count, double maf, uint64_t best_n, uint64_t* row, uint64_t* kmer, double* lrt, double* lambda,
                               double* p, double* af, uint64_t* n_kept, double* logl0, double* lambda0, uint64_t* rows_read,
                               uint64_t* rows_tested, uint64_t* pairs_shipped) {
    return guarded([&] {
        if (!h || (!Y && n_pheno) || !t || !col) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_test_table_multi: null argument");
        std::vector<std::vector<TableHit>> kept;
        uint64_t n_read = 0, n_tested = 0, n_shipped = 0;
        test_table_multi(h, n_pheno, Y, t, col, n_acc, min_count, maf, best_n, kept, logl0, lambda0, n_read, n_tested, n_shipped);
        for (uint32_t k = 0; k < n_pheno; k++) {
            const uint64_t at = (uint64_t)k * best_n;
            for (uint64_t i = 0; i < kept[k].size(); i++) {
                if (row) row[at + i] = kept[k][i].row;
                if (kmer) kmer[at + i] = kept[k][i].kmer;
                if (lrt) lrt[at + i] = kept[k][i].lrt;
                if (lambda) lambda[at + i] = kept[k][i].lam;
                if (p) p[at + i] = kept[k][i].p;
                if (af) af[at + i] = kept[k][i].af;
            }
            if (n_kept) n_kept[k] = kept[k].size();
        }
        if (rows_read) *rows_read = n_read;
        if (rows_tested) *rows_tested = n_tested;
        if (pairs_shipped) *pairs_shipped = n_shipped;
    });
}

int kgwas_lmm_run_table_multi(const char* kinship_path, const char* table_base, uint32_t kmer_len, const char* pheno_path, uint32_t n_cols,
                              const uint32_t* pheno_cols, const char* const* out_paths, uint64_t mac, double maf, uint64_t best_n,
                              double lmin, double lmax, uint64_t chunk_variants, int32_t device, kgwas_lmm_stats* total) {
    return guarded([&] {
        run_table_multi(kinship_path, table_base, kmer_len, pheno_path, n_cols, pheno_cols, out_paths, mac, maf, best_n, lmin, lmax,
                        chunk_variants, device, total);
    });
}

int kgwas_lmm_get_stats(const kgwas_lmm* h, kgwas_lmm_stats* out) {
    return guarded([&] {
        if (!h || !out) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_get_stats: null argument");
        *out = h->st;
    });
}

void kgwas_lmm_destroy(kgwas_lmm* h) { delete h; }

int kgwas_lmm_read_kinship(const char* path, uint64_t n_expected, double* K) {
    return guarded([&] {
        if (!path || !K) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_read_kinship: null argument");
        const std::vector<double> k = read_kinship(path, n_expected);
        memcpy(K, k.data(), k.size() * sizeof(double));
    });
}

int kgwas_lmm_read_fam(const char* path, uint32_t pheno_col, uint64_t cap, double* values, uint8_t* keep, uint64_t* n_lines) {
    return guarded([&] {
        if (!path || !n_lines) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_read_fam: null argument");
        std::vector<double> v;
        std::vector<uint8_t> k;
        read_fam(path, pheno_col, v, k);
        *n_lines = v.size();
        for (uint64_t i = 0; i < std::min<uint64_t>(cap, v.size()); i++) {
            if (values) values[i] = v[i];
            if (keep) keep[i] = k[i];
        }
    });
}

uint64_t kgwas_lmm_format_assoc(const char* chr, const char* rs, const char* ps, uint32_t n_miss, const char* allele1, const char* allele0,
                                double af, double l_mle, double p_lrt, char* out, uint64_t cap) {
    uint64_t need = 0;
    guarded([&] {
        if (chr && (!rs || !ps || !allele1 || !allele0)) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_format_assoc: null argument");
        need = format_assoc(chr, rs, ps, n_miss, allele1, allele0, af, l_mle, p_lrt, out, cap);
    });
    return need;
}

}  // extern "C"
