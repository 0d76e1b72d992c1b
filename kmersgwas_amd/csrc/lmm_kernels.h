// lmm_kernels.h — launchers of lmm_kernels.hip (the device side of lmm_lrt) and the layout they share with lmm.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace kgwas {

constexpr uint32_t LMM_GRID = 101;      // grid points over log lambda: 100 intervals (emma.R's ngrids)
constexpr uint32_t LMM_HB_COLS = 208;   // the h table's columns: h at the 101 points, then dh/dlog lambda at them, then 6 of zeros
constexpr uint32_t LMM_BASE = 8;        // per grid point: sum h, sum log h, Sww, Swy, Syy, then Sww', Swy', Syy' (weights dh)
constexpr uint32_t LMM_MAXC = 8;        // covariates: the most columns of W (kgwas_lmm_set_covariates)
// With covariates a grid point has a record of LMM_BASEC doubles in place of its LMM_BASE sums (A = Wt^T H Wt, b = Wt^T H yt, dA and
// db the same with weights dh; matrices are [j][k] with row stride LMM_MAXC, entries past q are zero):
constexpr uint32_t LMM_REC_SH = 0;       //   sum h
constexpr uint32_t LMM_REC_SLOG = 1;     //   sum log h
constexpr uint32_t LMM_REC_RSS0 = 2;     //   yy - b^T A^-1 b
constexpr uint32_t LMM_REC_LOGDET = 3;   //   log |A|
constexpr uint32_t LMM_REC_TR = 4;       //   tr(A^-1 dA)
constexpr uint32_t LMM_REC_DYY = 5;      //   dyy
constexpr uint32_t LMM_REC_DRSS0 = 6;    //   RSS0': the dh-weighted quadratic form of (A^-1 b, -1)
constexpr uint32_t LMM_REC_AINV = 7;     //   A^-1
constexpr uint32_t LMM_REC_DA = LMM_REC_AINV + LMM_MAXC * LMM_MAXC;  // dA
constexpr uint32_t LMM_REC_A0 = LMM_REC_DA + LMM_MAXC * LMM_MAXC;    // A^-1 b
constexpr uint32_t LMM_REC_DB = LMM_REC_A0 + LMM_MAXC;               // db
constexpr uint32_t LMM_REC_B = LMM_REC_DB + LMM_MAXC;                // b
constexpr uint32_t LMM_BASEC = LMM_REC_B + LMM_MAXC;                 // 159
constexpr uint32_t LMM_VTILE = 32;      // variants per wave of the rotation; chunk buffers are padded to it
constexpr uint32_t LMM_REFINE_STEPS = 12;
constexpr uint32_t LMM_PTILE = 4;       // phenotype columns a wave of lmm_grid_xy_kernel holds accumulators for
constexpr uint32_t LMM_PBLOCK = 32;     // phenotype columns per launch of the multi-phenotype pass: Gxy is chunk x 32 x 208 doubles,
                                        // 545 MB at the default chunk of 10 240 variants

struct LmmVariant {  // what lmm_prep leaves per variant
    double val[4];   // value of .bed code 0..3, centred: 2 - mean, 0 (missing), 1 - mean, 0 - mean
    double af;       // mean / 2
    uint32_t n_miss;
    uint32_t tested;
};

// Shapes: n individuals; ldi = n rounded up to 64 (row stride of U, Xt; length of d, wt, yt, zero past n); U has n rounded up to
// 16 rows (zero past n); bpsp = bytes per variant of the padded code rows (a multiple of 4, zero past the .bed's bytes).
struct LmmDims {
    uint32_t n, ldi, n16, bps, bpsp;
};

// bed[nv][bps] -> codes[nv][bpsp], vars[nv] (counts, af, tested by maf / miss / constant, values)
hipError_t launch_lmm_prep(const uint8_t* bed, uint32_t nv, LmmDims dm, double maf, double miss, uint8_t* codes, LmmVariant* vars,
                           hipStream_t st);
// Xt[v][i] = sum_k U[k][i] val_v[code_v[k]], v < nv rounded up to LMM_VTILE (rows past nv are zero)
hipError_t launch_lmm_rotate(const uint8_t* codes, const LmmVariant* vars, uint32_t nv, LmmDims dm, const double* U, double* Xt,
                             hipStream_t st);
// The fixed effects W of the launchers below that take (q, W): q = 0 is W = 1, `W` = wt[ldi] = U^T 1, and a grid point has LMM_BASE
// sums; 1 <= q <= LMM_MAXC is covariates (n x q, orthonormal columns whose span holds the constant vector), `W` = Wt[q][ldi] = the
// rotated columns (zero past n), a grid point has a record of LMM_BASEC doubles, and G has q + 2 rows per variant. Any other q is
// refused (hipErrorInvalidValue), and so is q > 0 with more than one phenotype column.
// Yt[np][ldi] -> base[np][LMM_GRID][LMM_BASE] (q = 0) or base[LMM_GRID][LMM_BASEC] (q > 0, np = 1) from d, W and the grid's lambda[g]
hipError_t launch_lmm_base(LmmDims dm, uint32_t q, const double* d, const double* W, const double* Yt, uint32_t np, const double* lambda,
                           double* base, hipStream_t st);
// G[v][3][LMM_HB_COLS]: sums over i of HB[i][c] * (xt^2, xt wt, xt yt); q > 0: G[v][q + 2][LMM_HB_COLS], rows xt^2, xt wt_0 .. xt wt_{q-1}, xt yt
hipError_t launch_lmm_grid(const double* Xt, uint32_t nv, LmmDims dm, uint32_t q, const double* W, const double* yt, const double* HB,
                           double* G, hipStream_t st);
// Gx[v][2][LMM_HB_COLS]: the xt^2 and xt wt rows of launch_lmm_grid's G at q = 0, the same bits
hipError_t launch_lmm_grid_shared(const double* Xt, uint32_t nv, LmmDims dm, const double* wt, const double* HB, double* Gx,
                                  hipStream_t st);
// Gxy[p][v][LMM_HB_COLS], p < np <= LMM_PBLOCK, v < nv: the xt yt row of launch_lmm_grid's G for yt = Yt[p], the same bits
hipError_t launch_lmm_grid_xy(const double* Xt, uint32_t nv, LmmDims dm, const double* Yt, uint32_t np, const double* HB, double* Gxy,
                              hipStream_t st);
// the null models of np columns: out[p] = (l0, lambda0), each with the bits of a call with np = 1
hipError_t launch_lmm_null(LmmDims dm, uint32_t q, const double* d, const double* W, const double* Yt, uint32_t np, const double* lambda,
                           const double* base, double* out, hipStream_t st);
// per tested variant: lrt, lambda, p (NaN for the others)
hipError_t launch_lmm_refine(const double* Xt, const double* G, const LmmVariant* vars, uint32_t nv, LmmDims dm, uint32_t q,
                             const double* d, const double* W, const double* yt, const double* lambda, const double* base, double l0,
                             double* lrt, double* lam, double* p, hipStream_t st);
// -lmm 4. The REML null model of yt: out[0..4) = lR0, lambda0_remle, vg, ve
hipError_t launch_lmm_null_reml(LmmDims dm, uint32_t q, const double* d, const double* W, const double* yt, const double* lambda,
                                const double* base, double* out, hipStream_t st);
// -lmm 4. launch_lmm_refine's lrt, lam and p with their bits, and per tested variant the REML effect estimate, its standard error,
// l_remle, the Wald p (both at l_remle) and the score p at lam0, the null model's ML lambda (NaN for the others)
struct LmmWaldOut {
    double *beta, *se, *lam, *p_wald, *p_score;
};
hipError_t launch_lmm_refine_all(const double* Xt, const double* G, const LmmVariant* vars, uint32_t nv, LmmDims dm, uint32_t q,
                                 const double* d, const double* W, const double* yt, const double* lambda, const double* base, double l0,
                                 double lam0, double* lrt, double* lam, double* p, LmmWaldOut w, hipStream_t st);
// launch_lmm_refine at q = 0 per (variant, column) of a block of np <= LMM_PBLOCK columns, results at [p][v] (row stride nv); Yt,
// base and null (pairs l0, lambda0) start at the block's first column
hipError_t launch_lmm_refine_multi(const double* Xt, const double* Gx, const double* Gxy, const LmmVariant* vars, uint32_t nv, LmmDims dm,
                                   const double* d, const double* wt, const double* Yt, uint32_t np, const double* lambda,
                                   const double* base, const double* null, double* lrt, double* lam, double* p, hipStream_t st);

// lmm_table_kernels.hip: the front end of the k-mers table route. rows[n_rows][stride] are table rows (k-mer word, then the
// presence words), sq[n_rows][2 W_m] their bits squeezed to phenotype order (launch_squeeze, zero past dm.n). A row is tested iff
// dm.n >= min_count && n1 >= min_count && n1 <= dm.n - min_count (kmers_table_to_bed) and launch_lmm_prep would test its .bed
// row at this maf. For the tested rows alone, in row order: codes[t][bpsp], vars[t] (both with the bits launch_lmm_prep leaves
// for that .bed row), row_out[t] = first_row + row, kmer_out[t] = its k-mer word; total[0] = their number. Scratch: n1flag
// [n_rows], block_cnt and block_off [n_rows / LMM_TABLE_BLOCK rounded up]. 0 < n_rows < 2^31.
constexpr uint32_t LMM_TABLE_BLOCK = 256;
hipError_t launch_lmm_table_front(const uint64_t* rows, uint64_t stride, const uint32_t* sq, uint32_t n_rows, uint32_t W_m, LmmDims dm,
                                  uint64_t first_row, uint32_t min_count, double maf, uint32_t* n1flag, uint32_t* block_cnt,
                                  uint32_t* block_off, uint32_t* total, uint8_t* codes, LmmVariant* vars, uint64_t* row_out,
                                  uint64_t* kmer_out, hipStream_t st);

// lmm_table_kernels.hip: the first stage of the selection of the multi-phenotype table pass. After launch_lmm_refine_multi over a
// sub-chunk of cc compacted tested rows and a block of pb <= LMM_PBLOCK columns (lrt, lam, p at [column][row], row stride cc), the
// pair (column c, row v) survives iff cols[c].open != 0 (the column's host heap is not full) or lrt[c][v] > cols[c].thr (the lrt of
// the worst hit that heap kept when the host last looked; a NaN lrt never passes it). Survivors become records in (column, row)
// order, the same content in every run: count[0] = their number, rec[0 .. count). No store goes past rec[cap). Scratch: block_cnt
// and block_off [pb cc / LMM_TABLE_BLOCK rounded up]. cc > 0, pb cc < 2^31.
struct LmmSelectCol {  // per column of the block
    double thr;
    uint32_t open, pad;
};
struct LmmTableRecord {  // everything the host heap needs of one surviving (column, row) pair
    double lrt, lam, p, af;
    uint64_t row, kmer;  // the table row index and its k-mer word
    uint32_t col, pad;   // the column within the block; pad = 0
};
hipError_t launch_lmm_table_select(const double* lrt, const double* lam, const double* p, uint32_t cc, uint32_t pb, const LmmVariant* vars,
                                   const uint64_t* row, const uint64_t* kmer, const LmmSelectCol* cols, uint32_t* block_cnt,
                                   uint32_t* block_off, uint32_t* count, LmmTableRecord* rec, uint32_t cap, hipStream_t st);

// lmm_table_kernels.hip: the pattern table ("The pattern table"), which kgwas_lmm_test_table_unique (the pattern
// cache) and kgwas_lmm_test_table_multi_skip (the dead-pattern skip) both keep on the device for one call. Its key is a compacted
// code row, codes[t][bpsp] of launch_lmm_table_front. A slot holds a 64-bit tag (0: empty), an owner word and the code row; the
// cache adds lrt, lam, p of the pattern (res), the skip one state word (0 live, 1 dead; it only ever goes from 0 to 1). `slots` is a
// power of two >= 64. Before the first piece of a call every tag (and state) is 0 and every owner LMM_CACHE_NO_OWNER; between
// pieces every owner of a slot in use is 0.
constexpr uint32_t LMM_CACHE_PROBES = 16;               // slots a row looks at before it gives up
constexpr uint32_t LMM_CACHE_NONE = 0xFFFFFFFFu;        // slot_of of a row that reached no slot
constexpr uint32_t LMM_CACHE_NO_OWNER = 0xFFFFFFFFu;
enum : uint32_t {                    // what a tested row of a piece is to the table
    LMM_ROW_OWNER = 0,               //   the first row of its tag in a new slot: computed (the cache keeps its result in the slot)
    LMM_ROW_CACHED = 1,              //   no state: its code row equals its slot's: not computed, it takes the slot's result
    LMM_ROW_DEAD = LMM_ROW_CACHED,   //   state: its code row equals its slot's and the slot was dead when the piece began: not computed
    LMM_ROW_COLLIDED = 2,            //   its slot holds another code row with its tag: computed
    LMM_ROW_REJECTED = 3,            //   no slot within LMM_CACHE_PROBES: computed
    LMM_ROW_LIVE = 4                 //   state: its code row equals its slot's and the slot was live (a new owner's copies too): computed
};
struct LmmCache {
    unsigned long long* tag;  // [slots]
    uint32_t* owner;          // [slots] compact index + 1 of the smallest row that reached the slot in this piece
    uint32_t* key;            // [slots][bpsp / 4]
    double* res;              // [slots][3]: lrt, lam, p (the cache; nullptr for the skip)
    uint32_t* state;          // [slots] (the skip; nullptr for the cache)
    uint32_t slots;
};
inline uint64_t lmm_cache_slot_bytes(LmmDims dm) { return 8 + 8 + dm.bpsp + 3 * sizeof(double); }  // (the owner word padded to 8)
inline uint64_t lmm_skip_slot_bytes(LmmDims dm) { return 8 + 4 + 4 + dm.bpsp; }                    // tag, owner, state, the code row
// What the look-up leaves of a piece, and its scratch. Every per-row array has room for the piece's tested rows, block_cnt and
// block_off for their number / LMM_TABLE_BLOCK rounded up.
struct LmmPiece {
    unsigned long long* row_tag;     // [t] the row's tag: a mix of its code row, cut to tag_mask, never 0
    uint32_t *slot_of, *cls;         // [t] its slot (LMM_CACHE_NONE: none) and its class
    uint32_t *block_cnt, *block_off;
    uint32_t* total2;                // [1] the number of rows to compute: every class but LMM_ROW_CACHED / LMM_ROW_DEAD
    uint8_t* codes2;                 // [t2][bpsp] those rows, compacted in row order
    LmmVariant* vars2;               // [t2]
    uint32_t* back;                  // [t2] = t
    uint64_t *row2, *kmer2;          // [t2] row[t], kmer[t] (optional: both or neither)
};
// The look-up of a piece's `total` compacted rows fills pc; row and kmer are read only where pc.row2 and pc.kmer2 are given. With
// c.state an equal code row is LMM_ROW_DEAD or LMM_ROW_LIVE by its slot's state as the piece found it, without it LMM_ROW_CACHED.
// 0 < total < 2^31.
hipError_t launch_lmm_pattern_lookup(const uint8_t* codes, const LmmVariant* vars, const uint64_t* row, const uint64_t* kmer, uint32_t total,
                                     LmmDims dm, uint64_t tag_mask, LmmCache c, LmmPiece pc, hipStream_t st);

// The pattern cache. After the back end over the sub-chunk pc.back[first .. first + cc) of the rows to compute: their lrt, lam, p go
// to the piece's arrays r_* at the rows' places, and an owner's into its slot too.
hipError_t launch_lmm_cache_scatter(const double* lrt, const double* lam, const double* p, uint32_t first, uint32_t cc, uint32_t total,
                                    LmmCache c, LmmPiece pc, double* r_lrt, double* r_lam, double* r_p, hipStream_t st);
// After the piece's last sub-chunk: the rows from cache take their slot's result, and the piece's new slots get owner 0.
hipError_t launch_lmm_cache_fanout(uint32_t total, LmmCache c, LmmPiece pc, double* r_lrt, double* r_lam, double* r_p, hipStream_t st);

// The dead-pattern skip. After launch_lmm_refine_multi over a sub-chunk of cc rows and a block of pb columns: shipped[v] = 1 where
// launch_lmm_table_select ships a pair of row v of this block (the same rule on the same cols); the other rows' words are left as
// they are, so over the blocks of a sub-chunk the words, zero at its start, become "any pair shipped".
hipError_t launch_lmm_skip_flag(const double* lrt, const LmmSelectCol* cols, uint32_t cc, uint32_t pb, uint32_t* shipped, hipStream_t st);
// After the last column block of the sub-chunk pc.back[first .. first + cc): an owner's or a live row's slot becomes dead where the
// row shipped no pair, and an owner's slot gets owner 0.
hipError_t launch_lmm_skip_mark(const uint32_t* shipped, uint32_t first, uint32_t cc, uint32_t total, LmmCache c, LmmPiece pc,
                                hipStream_t st);
// dead[0] = the number of dead slots. Scratch: block_cnt and block_off [c.slots / LMM_TABLE_BLOCK].
hipError_t launch_lmm_skip_count_dead(LmmCache c, uint32_t* block_cnt, uint32_t* block_off, uint32_t* dead, hipStream_t st);

}  // namespace kgwas
