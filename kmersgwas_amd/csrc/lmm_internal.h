// lmm_internal.h — what lmm.cpp (the device session, the .bed passes and the back-end steps), lmm_table.cpp (the k-mers table
// route) and lmm_files.cpp (the file layer) share: the handle and what they call in each other. Nothing else includes it.
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "common.h"
#include "device.h"
#include "lmm_kernels.h"

// Times the stages of the work on the handle's stream into the buckets of kgwas_lmm_stats. begin() opens an interval, end(bucket)
// closes it into that bucket and opens the next one; once the stream is synchronised collect() adds every closed interval to its
// bucket and forgets them all. Copies stay outside: they are issued before begin() or after the last end().
class LmmStageTimer {
  public:
    using Bucket = double kgwas_lmm_stats::*;
    void begin(hipStream_t st) { stamp(st); }
    void end(Bucket bucket, hipStream_t st) {
        stamp(st);
        closed.push_back({used - 2, bucket});
    }
    void collect(kgwas_lmm_stats& stats);

  private:
    struct Interval {
        size_t from;  // events[from] .. events[from + 1]
        Bucket bucket;
    };
    void stamp(hipStream_t st);
    std::vector<kgwas::Event> events;  // created when first needed, reused after every collect()
    size_t used = 0;
    std::vector<Interval> closed;
};

struct kgwas_lmm {
    int device = 0;
    uint64_t n = 0;
    kgwas::LmmDims dm{};
    double lmin = 0, lmax = 0;
    uint32_t chunk = 0;
    std::vector<double> U, d;
    std::vector<double> y_cur;
    bool have_null = false;
    double l0 = 0, lambda0 = 0;
    bool have_null_reml = false;  // -lmm 4: the REML null model of y_cur (fit_null_reml); falls with have_null
    double l0_reml = 0, lambda0_reml = 0, vg = 0, ve = 0;
    kgwas_lmm_stats st{};
    bool on_device = false;
    LmmStageTimer timer;
    kgwas::DevBuf<double> d_U, d_d, d_wt, d_yt, d_HB, d_grid, d_base, d_null, d_Xt, d_G, d_lrt, d_lam, d_p;
    kgwas::DevBuf<uint8_t> d_bed, d_codes;
    kgwas::DevBuf<kgwas::LmmVariant> d_vars;
    // The buffers below are allocated by the first pass that needs them.
    // ensure_multi_chunk: per chunk the shared grid sums, per chunk and block of LMM_PBLOCK columns the xt yt sums and the results
    bool have_multi_chunk = false;
    kgwas::DevBuf<double> d_Gx, d_Gxy, d_lrtm, d_lamm, d_pm;
    std::vector<double> h_outm;
    void ensure_multi_chunk();
    // ensure_multi_cols: per phenotype column Yt, the base sums and the null model
    uint32_t multi_cols = 0;
    kgwas::DevBuf<double> d_Ytm, d_basem, d_nullm;
    void ensure_multi_cols(uint32_t n_pheno);
    // ensure_select, the selection of the multi-phenotype table pass: per block of 256 pairs the counts and offsets, the
    // survivors' number, the block's thresholds, and the records on the device and in pinned host memory
    bool have_select = false;
    kgwas::DevBuf<uint32_t> d_sel_cnt, d_sel_off, d_sel_total;
    kgwas::DevBuf<kgwas::LmmSelectCol> d_sel_cols;
    kgwas::DevBuf<kgwas::LmmTableRecord> d_sel_rec;
    kgwas::PinBuf<kgwas::LmmTableRecord> h_sel_rec;
    void ensure_select();
    // ensure_wald, -lmm 4: per chunk beta, se, l_remle, p_wald, p_score ([5][chunk]); the REML null model's four numbers
    bool have_wald = false;
    kgwas::DevBuf<double> d_wald, d_null_reml;
    void ensure_wald();
    kgwas::LmmWaldOut wald_out() const {
        return {d_wald.p, d_wald.p + chunk, d_wald.p + 2 * (uint64_t)chunk, d_wald.p + 3 * (uint64_t)chunk, d_wald.p + 4 * (uint64_t)chunk};
    }
    // kgwas_lmm_set_covariates: q > 0 columns of W in place of W = 1. d_Wt[q][ldi] = the rotated columns of W's orthonormal basis,
    // d_basec the records of the grid points (in place of d_base), d_G grows to chunk x (q + 2) x LMM_HB_COLS. log_det_R = log |det R|
    // of W = Q R: the REML likelihood of W is that of Q less this.
    uint32_t q = 0;
    double log_det_R = 0;
    uint64_t g_rows = 3;  // rows per variant d_G has room for
    kgwas::DevBuf<double> d_Wt, d_basec;
    // what the launchers take as (q, W, base): the rotated fixed effects and the grid points' base rows in use
    const double* fixed_t() const { return q ? d_Wt.p : d_wt.p; }
    double* base_rows() const { return q ? d_basec.p : d_base.p; }
    kgwas::Stream stream;  // (behind the buffers its work reads and writes: it goes first)
    ~kgwas_lmm() {
        if (on_device) (void)hipSetDevice(device);  // (before any member is released)
    }
};

namespace kgwas {
namespace lmm {

struct TableHit {  // one tested row's result
    double lrt, lam, p, af;
    uint64_t row, kmer;
};

struct Destroy {
    void operator()(kgwas_lmm* h) const { kgwas_lmm_destroy(h); }
};
using Handle = std::unique_ptr<kgwas_lmm, Destroy>;

// ---- lmm.cpp: the session and the .bed passes (what each does stands at its definition) ----
kgwas_lmm* create(uint64_t n, const double* K, int device, double lmin, double lmax, uint64_t chunk_variants);
void fit_null(kgwas_lmm* h, const double* y);
// -lmm 4's five further outputs of a .bed pass (host arrays over all variants; any may be null). With `wald` the pass runs the
// -lmm 4 refinement; lrt, lam, p, af, n_miss and tested are the same either way.
struct WaldArrays {
    double *beta, *se, *lam_remle, *p_wald, *p_score;
};
void fit_null_reml(kgwas_lmm* h, const double* y);
// W[n][q] -> Qw[n][q], an orthonormal basis of its columns (modified Gram-Schmidt in column order, every projection done twice), and
// log |det R| of W = Qw R. Refuses q > LMM_MAXC, values that are not finite, n < q + 2, a rank-deficient W and a W whose span does
// not hold the constant vector; `who` starts the message. Host only: the file layer calls it before any device work.
void orthonormal_covariates(uint64_t n, uint32_t q, const double* W, std::vector<double>& Qw, double& log_det_R, const std::string& who);
void set_covariates(kgwas_lmm* h, uint32_t q, const double* W);
void test_bed(kgwas_lmm* h, const double* y, const uint8_t* body, uint64_t nv, double maf, double miss, double* lrt, double* lam,
              double* p, double* af, uint32_t* n_miss, uint8_t* tested, const WaldArrays* wald = nullptr);
void multi_prepare(kgwas_lmm* h, uint32_t n_pheno, const double* Y, double* logl0, double* lambda0,
                   const char* who = "kgwas_lmm_test_bed_multi");
void multi_run(kgwas_lmm* h, uint32_t n_pheno, const uint8_t* body, uint64_t nv, double maf, double miss, double* lrt, double* lam,
               double* p, double* af, uint32_t* n_miss, uint8_t* tested);
// ---- lmm.cpp: the back-end steps the .bed passes share with the table route ----
void single_backend(kgwas_lmm* h, const uint8_t* codes, const LmmVariant* vars, uint32_t cc, bool wald = false);
void multi_front(kgwas_lmm* h, const uint8_t* codes, const LmmVariant* vars, uint32_t cc);
void multi_block(kgwas_lmm* h, const LmmVariant* vars, uint32_t cc, uint32_t p0, uint32_t pb);
// ---- lmm_table.cpp ----
void test_table(kgwas_lmm* h, const double* y, kgwas_table* t, const uint64_t* col, uint64_t n_acc, uint64_t min_count, double maf,
                uint64_t best_n, std::vector<TableHit>& kept, uint64_t& rows_read, uint64_t& rows_tested);
void test_table_unique(kgwas_lmm* h, const double* y, kgwas_table* t, const uint64_t* col, uint64_t n_acc, uint64_t min_count, double maf,
                       uint64_t best_n, uint64_t max_patterns, std::vector<TableHit>& kept, uint64_t& rows_read, uint64_t& rows_tested,
                       kgwas_lmm_unique_stats& u);
void test_table_multi(kgwas_lmm* h, uint32_t n_pheno, const double* Y, kgwas_table* t, const uint64_t* col, uint64_t n_acc,
                      uint64_t min_count, double maf, uint64_t best_n, std::vector<std::vector<TableHit>>& kept, double* logl0,
                      double* lambda0, uint64_t& rows_read, uint64_t& rows_tested, uint64_t& pairs_shipped);
void test_table_multi_skip(kgwas_lmm* h, uint32_t n_pheno, const double* Y, kgwas_table* t, const uint64_t* col, uint64_t n_acc,
                           uint64_t min_count, double maf, uint64_t best_n, uint64_t max_patterns, std::vector<std::vector<TableHit>>& kept,
                           double* logl0, double* lambda0, uint64_t& rows_read, uint64_t& rows_tested, uint64_t& pairs_shipped,
                           kgwas_lmm_skip_stats& u);
// ---- lmm_files.cpp ----
std::vector<double> read_kinship(const std::string& path, uint64_t n_expected, const char* counted_in = "the .fam");
// GEMMA's -c file: one row per individual, whitespace-separated numbers, NA missing. values[rows][q]; keep[r] = 0 where row r has an NA
void read_covariates(const std::string& path, std::vector<double>& values, std::vector<uint8_t>& keep, uint32_t& q);

}  // namespace lmm
}  // namespace kgwas
