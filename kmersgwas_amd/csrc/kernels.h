// kernels.h — host-visible launch interface of the gfx950 kernels (kernels.hip).
// Internal to libkgwas; the public boundary is include/kgwas.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "env.h"
#include "launch.h"

namespace kgwas {

// One candidate record shipped device -> host (sparse mode).
struct Cand {
    uint64_t kmer;
    double score;
    uint64_t row;  // global file row index
};

// Where the scorer reads a row's squeezed bits from.
//   direct mode  : the .table rows in place  (stride 2*(1+W_f) dwords, bits start at dword 2)
//   squeezed mode: the squeeze kernel's output (stride 2*W_m dwords, bits start at dword 0)
struct RowSrc {
    const uint32_t* base;
    uint64_t stride_dw;
    uint32_t off_dw;
    uint32_t avail_dw;  // dwords of bit data present in a row
};

// The MAC-passing rows of a launch are counted in TESTED_SHARDS counters (block b adds to counter b % TESTED_SHARDS, the
// host sums them): a single counter takes one device-scope atomic per block or wave, and those serialise at the memory
// side (1.3e5 of them made an 8 M-row launch of the bit-sliced filter ten times slower than its arithmetic).
constexpr uint32_t TESTED_SHARDS = 256;

struct ScoreArgs {
    RowSrc src;
    const uint32_t* dmask;      // [2*W_m] AND mask per squeezed dword (0 where no data exists)
    const uint64_t* file_rows;  // the .table rows (for k-mer ids)
    uint64_t file_stride_w;     // 1 + W_f
    uint64_t n_rows;            // rows in this launch
    uint64_t first_row;         // global file row of row 0
    uint32_t S;                 // phenotyped accessions
    uint32_t W_m;               // 64-bit words per squeezed row (even)
    uint32_t n_pheno;
    uint32_t min_count;
    const float* Yperm;   // VALU kernel: [n_pheno][L] permuted, padded (L = 64*W_m)
    const float* Ymfma;   // MFMA kernel: [n_ctiles][L][16] chain-step major
    const float* sums;    // [n_pheno] float32 sequential sums
    const double* thr;    // [n_pheno] stale heap minima (sparse mode)
    // dense outputs (null in sparse mode)
    double* dense;        // [n_pheno][n_rows]
    uint32_t* n1_out;     // [n_rows] masked popcount
    uint64_t* kmer_out;   // [n_rows]
    // sparse outputs (null in dense mode)
    Cand* cand;           // [n_pheno][cap]
    uint32_t* cand_cnt;   // [n_pheno]
    uint32_t cap;
    unsigned long long* tested;  // MAC-passing rows, accumulated ([TESTED_SHARDS]; the exact scorers use [0])
    // Device-side threshold tracking (sparse mode, optional): every shipped candidate is counted in a
    // per-column histogram over the top bits of its score; thr_update_kernel raises thr[p] between
    // chunks to the largest bin boundary with >= topn[p] candidates at or above it.
    uint32_t* hist;             // [n_pheno][hist_bins] or null
    const uint32_t* hist_base;  // [n_pheno] (bits(score) >> HIST_SHIFT) of bin 0
    uint32_t hist_bins;
    // Output of the coarse path (rescore + compaction): the chunk's candidates in (column, row) order.
    double* so_score;    // [key_cap] or null
    uint64_t* so_kmer;   // [key_cap]
    uint32_t* so_row;    // [key_cap] chunk-local row
};

constexpr int HIST_SHIFT = 44;          // 8 mantissa bits per bin: 0.4 % score resolution
constexpr uint32_t HIST_BINS = 16384;   // 64 binades above the threshold at sparse start

// thr[p] = max(thr[p], thr_host[p], largest bin boundary with >= topn[p] counted scores at or above it).
hipError_t launch_copy_to_host(const void* src, void* dst_dev, size_t bytes, hipStream_t st);  // dst_dev: device address of mapped pinned memory
// device pointers of the (mapped) pinned destination
// a chunk's counts, tested-row shards and current thresholds into mapped host buffers, one launch (n_* = 0: skip that part)
hipError_t launch_chunk_tail(const uint32_t* meta, uint32_t n_meta, uint32_t* h_meta, const unsigned long long* tested, uint32_t n_tested,
                             unsigned long long* h_tested, const double* thr, uint32_t n_thr, double* h_thr, hipStream_t st);
// launch_thr_update and launch_chunk_tail in one launch (block p: column p's threshold, also into h_thr[p] unless h_thr is null;
// block 0: the counts and the tested-row shards)
hipError_t launch_thr_tail(const uint32_t* hist, const uint32_t* hist_base, uint32_t bins, const uint64_t* topn, const double* thr_host, double* thr,
                           uint32_t n_pheno, const uint32_t* meta, uint32_t n_meta, uint32_t* h_meta, const unsigned long long* tested,
                           uint32_t n_tested, unsigned long long* h_tested, double* h_thr, hipStream_t st);
hipError_t launch_records_to_host(const double* sc, const uint64_t* km, const uint32_t* rw, uint32_t n, double* h_sc, uint64_t* h_km, uint32_t* h_rw,
                                  hipStream_t st);
hipError_t launch_thr_update(const uint32_t* hist, const uint32_t* hist_base, uint32_t bins, const uint64_t* topn,
                             const double* thr_host, double* thr, uint32_t n_pheno, hipStream_t st);

// Dense start: thr_a[p] = thr_b[p] = thr_host_copy[p] = the topn[p]-th largest score of column p among the chunk's
// MAC-passing rows (dense: [n_pheno][n_rows]); info[0] = MAC-passing rows, info[1] = 1 if one of their scores is NaN.
// Columns with fewer than topn[p] such rows are left alone.
hipError_t launch_dense_select(const double* dense, const uint32_t* n1, uint32_t n_rows, uint32_t n_pheno, uint32_t S, uint32_t min_count,
                               const uint64_t* topn, double* thr_a, double* thr_b, double* thr_host_copy, uint32_t* info, hipStream_t st);

// Scoring kernels. rows_per_block only matters for the MFMA kernel (multiple of 128).
hipError_t launch_score_valu(const ScoreArgs& a, hipStream_t st);
// nb_full = leading 128-sample blocks whose four dwords all exist in the row and need no masking.
hipError_t launch_score_mfma(const ScoreArgs& a, uint32_t rows_per_block, uint32_t nb_full, hipStream_t st);
size_t mfma_lds_bytes(uint32_t W_m);

// Coarse int8 filter (score_coarse.hip). Survivors are bits of a [column][row] bitmap; launch_bitmap_keys lists them,
// and launch_rescore scores them exactly, column by column in row order (survivors.hip, below).
// Per-slot constants of the coarse filter (score_coarse.hip); a slot is one of the PG*16 operand columns of an LDS
// group. y_i ~ c + u*(254*q0_i + q1_i) (two slices) or c + u*q0_i (one slice), c = sum/N. A pair survives iff
// |Dc| >= sqrt(thr)*kalpha*sqrt(d) - iu*E(N1), constants already rounded in the conservative direction by the host.
struct CoarseCol {
    double kalpha;  // (1 - 2^-19) / (N * u)
    float iu;       // 1 / u, rounded up
    int32_t pheno;  // phenotype column in this slot; -1: padding or the group's ones column (slot PG*16-1 -> N1)
};
struct CoarseArgs {
    RowSrc src;
    uint64_t n_rows;
    uint32_t S, n_pheno, min_count;
    uint32_t n_kgroups;     // 512-sample groups = ceil(W_m / 8)
    uint32_t n_lgroups;     // LDS groups of T/NS x 16 operand columns
    uint32_t n_slices;      // int8 slices per column: 1 or 2
    const int8_t* Bq;       // [n_lgroups][n_kgroups][8][T][64 lanes][16] int8 slices, see score_coarse.hip
    const CoarseCol* cols;  // [n_lgroups][T/NS*16]
    const double* thr;      // [n_pheno]
    unsigned long long* bitmap;  // survivors: [n_pheno][words_per_col] 64-bit words, bit r of word w = chunk row 64 w + r; zeroed by the caller
    uint64_t words_per_col;
    unsigned long long* tested;
    // E(N1) = eg_max + min(rall_max, N1 * rmax_max) bounds |yigi_ref - yc| / u_p for every column (units of Dc,
    // each the maximum over the columns, rounded up): float32 summation error of the reference chains, the larger
    // one-sign sum of the quantisation residuals, the largest residual.
    float eg_max, rall_max, rmax_max;
};
size_t coarse_lds_bytes(uint32_t n_kgroups, uint32_t T);
hipError_t launch_coarse(const CoarseArgs& a, uint32_t T, uint32_t rows_per_block, hipStream_t st);
// Block-scaled coarse filter (score_mx.hip): FP4 table bits x FP6 / FP4 phenotype slices on
// v_mfma_scale_f32_16x16x128_f8f6f4, the slices of a column accumulated into ONE float32 accumulator through the block
// scales; same survivors' bitmap, same per-slot constants (CoarseCol, in accumulator units) and error terms as the int8
// filter. Samples are taken in n_full = S / 512 whole groups of 512 (four MFMA steps each) and n_quarter <= 4 quarter groups of
// 128 (one step each).
struct MxArgs {
    RowSrc src;
    uint64_t n_rows;
    uint32_t S, n_pheno, min_count;
    uint32_t n_full, n_quarter;
    uint32_t n_lgroups;     // LDS groups of CT x 16 operand columns
    uint32_t n_slices;      // 1: FP6 only, 2: FP6 + second slice
    uint32_t s1_fp6;        // second slice in FP6 (else FP4)
    uint32_t scale0;        // E8M0 block scale of the first slice, replicated in all four bytes (the second slice's is 2^0)
    const uint8_t* Bq;      // [n_lgroups][4 n_full + n_quarter steps][CT][step bytes], see score_mx.hip
    const CoarseCol* cols;  // [n_lgroups][CT*16]
    const double* thr;      // [n_pheno]
    unsigned long long* bitmap;  // as CoarseArgs
    uint64_t words_per_col;
    unsigned long long* tested;
    float eg_max, rall_max, rmax_max;  // as CoarseArgs, in accumulator units
};
size_t mx_lds_bytes(uint32_t n_steps, uint32_t CT, uint32_t n_slices, uint32_t s1_fp6);
// Operand bytes of one (MFMA step, column tile), for the kernels and the operand builder alike: the FP6 slice is 64 lanes x
// 16 B, then 64 lanes x 8 B (1536); the second slice follows in the same layout, an FP4 one with its 16-byte pieces only.
__host__ __device__ constexpr uint32_t mx_step_bytes(uint32_t n_slices, uint32_t s1_fp6) {
    return n_slices == 1 ? 1536u : (s1_fp6 ? 2u * 1536u : 1536u + 1024u);
}
hipError_t launch_mx(const MxArgs& a, uint32_t CT, uint32_t rows_per_block, hipStream_t st);
// The same filter with its operands STREAMED through an LDS ring instead of resident (score_mxs.hip): the waves of a block keep
// the accumulators of ALL column tiles of an operand group (NG column groups of CT tiles: up to 14 tiles, 222 columns), so a row
// is loaded and expanded once per operand group however many samples there are. a.Bq: [n_lgroups][step][NG][CT][2560 B],
// a.cols: [n_lgroups][NG][CT * 16] (each column group with its own ones column in its last slot); two slices, FP6 + FP4 only.
// form (NG = 1, CT > 7 only): 1 = eight waves of 32 rows, 2 = four waves of 64 rows.
bool mxs_supported(uint32_t CT, uint32_t NG, uint32_t n_slices, uint32_t s1_fp6);
size_t mxs_lds_bytes(uint32_t CT, uint32_t NG);
hipError_t launch_mxs(const MxArgs& a, uint32_t CT, uint32_t NG, uint32_t form, uint32_t rows_per_block, hipStream_t st);

// Narrow filter (score_narrow.hip): scans with one to four phenotype columns. FP4 table bits x three FP8 slices per
// column on v_mfma_scale_f32_16x16x128_f8f6f4; operand row 4 p + k = slice k of phenotype column p, row 4 p + 3 = ones
// (N1), so that lane (table row, p) of the accumulator tile holds everything its pair needs. Survivors go to the same
// bitmap as the wide filters' (in row order: launch_narrow_keys lists them).
constexpr int NARROW_SLICES = 3;
constexpr uint32_t NARROW_MAX_COLS = 4;
struct NarrowCol {
    double w[NARROW_SLICES];  // 2 * u_k: the accumulators are in units of 0.5
    double t1;                // N * c - sum  (c = sum / N rounded to double: tiny)
    double eg, rall, rmax;    // E(N1) = eg + min(rall, N1 * rmax) >= |yigi_ref - yc|, rounded up (phenotype units)
    double pad;               // absolute slack for the double-precision evaluation on both sides
    float wf[3];              // float32 pre-screen: the slice weights ...
    float slackf;             // ... and everything the pre-screen leaves out, as an upper bound on |r| (rounded up)
};
struct NarrowArgs {
    RowSrc src;
    uint64_t n_rows;
    uint32_t S, n_pheno, min_count;
    uint32_t n_kgroups;        // 512-sample groups
    const uint8_t* Bn;         // [n_kgroups * 4 steps][64 lanes][32] FP8 E4M3 slice operands, see score_narrow.hip
    const NarrowCol* cols;     // [n_pheno]
    const double* thr;         // [n_pheno]
    unsigned long long* bitmap;  // survivors: [n_pheno][words_per_col] 64-bit words, bit r of word w = chunk row 64 w + r; zeroed by the caller
    uint64_t words_per_col;
    unsigned long long* tested;
    uint32_t row_off;          // chunk row of this launch's first row (a launch that starts inside a chunk), a multiple of 64
    uint32_t* seg_cnt;         // [n_pheno][n_segs] survivors per 65 536-row segment of the chunk (atomic adds; zeroed by the caller), or null
    uint32_t n_segs;
    uint64_t slack_rows;       // rows of the same buffer that follow the launch's rows (readable: the staged kernel may read whole KB past its last row)
    uint32_t pack1;            // one column whose operand rows are replicated in all four column slots: lane (r, kb) tests row 16 kb + r of the pass
};
size_t narrow_lds_bytes(uint32_t n_kgroups);
hipError_t launch_narrow(const NarrowArgs& a, uint32_t rows_per_block, hipStream_t st);

// ---- behind the filters (survivors.hip): bitmap -> keys -> exact records, and the next chunk's prep launch ----------------
// The bitmap's set bits as row-ordered keys (column << row_bits | row), column after column, with each column's range
// (surv_off, surv_cnt) and the total (key_count; above key_cap = overflow, the ranges are then emptied). No sort: counts
// per 65 536-row block, a scan, a scatter. The words are always the wide filters' nibble-transposed ones (quarter word kg,
// nibble rt = rows 16 rt + 4 kg ..+3: filter_emit in filter_common.h); the scatter puts them back in row order. tile_pref[n_pheno + 1]: launch_rescore's tile table (first tile of each column). blk_scratch: n_pheno * (ceil(n_rows / 65536) + 1) words;
// blk_mask: 4 x 64 bits per (column, block) - the count kernel marks the threads whose words hold a survivor, the scatter kernel
// loads only those and CLEARS them: the bitmap is all zero again behind this call (the caller zeroes it once, not per chunk).
hipError_t launch_bitmap_keys(unsigned long long* bitmap, uint64_t words_per_col, uint64_t n_rows, uint32_t n_pheno, uint32_t* blk_scratch,
                              unsigned long long* blk_mask, uint32_t* keys_sorted, uint32_t key_cap, uint32_t row_bits, uint32_t* surv_off,
                              uint32_t* surv_cnt, uint32_t* key_count, uint32_t* tile_pref, hipStream_t st);
// The same for the narrow filter (one to four columns), whose kernels have already counted the survivors per segment
// (NarrowArgs::seg_cnt): ONE launch instead of four - every (segment, column) block adds up the counts before it and
// writes its keys; block (0, 0) writes the ranges, the tile table and meta (records = survivors: see launch_rescore_direct).
hipError_t launch_narrow_keys(const unsigned long long* bitmap, uint64_t words_per_col, uint64_t n_rows, uint32_t n_pheno, const uint32_t* seg_cnt,
                              uint32_t* keys_sorted, uint32_t key_cap, uint32_t row_bits, uint32_t* surv_off, uint32_t* surv_cnt,
                              uint32_t* key_count, uint32_t* tile_pref, uint32_t* meta, const unsigned long long* tested_shards, hipStream_t st);
// Survivors (sorted keys, per-column ranges; a sparse-mode ScoreArgs with Yperm set) -> exact candidates compacted in (column, row) order into a.so_score /
// a.so_kmer / a.so_row (HBM); meta[0..P) = candidates per column, meta[P..2P) = their offsets, meta[2P] = total,
// meta[2P + 1] = survivor keys emitted. tile_pref [P + 1], tile_cnt [key_cap / 256 + P + 1], tmp_score [key_cap].
hipError_t launch_rescore(const ScoreArgs& a, const uint32_t* keys, const uint32_t* surv_off, const uint32_t* surv_cnt,
                          uint32_t row_bits, uint32_t* tile_pref, uint32_t* tile_cnt, double* tmp_score,
                          const uint32_t* key_count, uint32_t* meta, hipStream_t st);
// Scans of a few columns: every survivor's record goes straight to its place in the key order (a.so_score = exact score or
// -inf for a survivor that is no candidate - the host's replay skips those), no tile scan, no compaction; meta was written
// by launch_narrow_keys (records per column = survivors per column).
hipError_t launch_rescore_direct(const ScoreArgs& a, const uint32_t* keys, const uint32_t* surv_off, const uint32_t* surv_cnt,
                                 uint32_t row_bits, const uint32_t* tile_pref, hipStream_t st);
// Counters of the next chunk and its survivors' bitmap (bitmap_words 64-bit words, may be 0) zeroed in one launch;
// seg_cnt (n_seg_words, may be 0): the narrow filter's per-segment survivor counts. tu.hist != null: the kernel's first
// blocks also raise the thresholds from the histograms (thr_update_kernel's work without a launch of its own: the chunk
// that follows is filtered against everything counted before it).
struct PrepThr {
    const uint32_t* hist;
    const uint32_t* hist_base;
    uint32_t bins;
    const uint64_t* topn;
    const double* thr_host;
    double* thr;
};
hipError_t launch_chunk_prep(uint32_t* cand_cnt, uint32_t n_pheno, unsigned long long* tested, uint32_t* key_count,
                             unsigned long long* bitmap, uint64_t bitmap_words, uint32_t* seg_cnt, uint32_t n_seg_words, const PrepThr& tu,
                             hipStream_t st);

// --pattern_counter: append hash_presence_absence_pattern of every MAC-passing row to out[*out_count ...];
// count_distinct_u64 sorts the collected hashes in place (device) and returns how many are distinct.
hipError_t launch_pattern_hash(const RowSrc& src, const uint32_t* dmask, uint64_t n_rows, uint32_t S, uint32_t W_m,
                               uint32_t min_count, uint64_t* out, unsigned long long* out_count, hipStream_t st);
hipError_t count_distinct_u64(uint64_t* keys, uint64_t n, uint64_t* result, hipStream_t st);

// kmers_table_to_bed (bed_kernels.hip): per squeezed row its popcount and pattern hash; the PLINK bytes.
hipError_t launch_bed_rowinfo(const uint32_t* sq, uint64_t n_rows, uint32_t W_m, uint32_t* n1_out, uint64_t* hash_out,
                              hipStream_t st);
hipError_t launch_bed_bytes(const uint32_t* sq, uint64_t n_rows, uint32_t W_m, uint32_t bytes_per_row, uint8_t* out,
                            hipStream_t st);

// SNP scorer (snp_kernels.hip): .bed bytes -> three bit planes per SNP ([snp][3][ndw]); planes -> scores[p][snp].
hipError_t launch_snp_planes(const uint8_t* bed, uint64_t n_snps, uint32_t bytes_per_snp, const uint32_t* byte_idx,
                             const uint32_t* shift, uint32_t S, uint32_t ndw, uint32_t* planes, hipStream_t st);
hipError_t launch_snp_score(const uint32_t* planes, uint64_t n_snps, uint32_t ndw, const float* Yperm, uint32_t L, uint32_t n_pheno,
                            double mac, double* scores, hipStream_t st);

// SNP kinship (snpkin_kernels.hip): a chunk's .bed bytes -> per-SNP missing-call values params[snp] and every sample's
// values vals[snp][S] (32 bytes each), used SNPs counted into n_used[TESTED_SHARDS]; then the pair sums of the lower-triangular
// tiles (tiles[i] = first row, first column; rows_per_wave 4 or 8 rows x 64 columns) advanced over the chunk's SNPs in order.
uint32_t snpkin_vals_stride(uint32_t S);  // entries per SNP: S + 8
size_t snpkin_vals_bytes(uint32_t S, uint32_t chunk_snps);
size_t snpkin_params_bytes(uint32_t chunk_snps);
hipError_t launch_snpkin_prep(const uint8_t* bed, uint32_t n_snps, uint32_t bytes_per_snp, uint32_t S, void* params, void* vals,
                              unsigned long long* n_used, hipStream_t st);
hipError_t launch_snpkin_accumulate(int rows_per_wave, const uint8_t* bed, uint32_t n_snps, uint32_t bytes_per_snp, uint32_t S,
                                    const void* params, const void* vals, const uint2* tiles, uint32_t n_tiles, double* sums,
                                    hipStream_t st);

// filter_kmers (filter_kernels.hip), on one device piece of n_rows table rows (stride 1 + W_f words) and the sorted list
// L[0, n): fk_match gives each row lower_bound / count in L, its run-head mark (r + 1 where the key differs from the previous
// row's, carry_key before row 0 when has_prev) and atomically the piece's first descent (*first_desc, preset to
// 0xFFFFFFFF). spl[j] = L[j * B], j < ns <= FK_SPLITTERS, is staged in LDS. fk_select max-scans the marks into run_start,
// flags the rows the merge-join emits before the first descent (carry_run: rows of the piece's first run seen before it),
// compacts their offsets into sel / *n_sel and fills info[0..3] (last row's run length and key; at a descent d > 0, row
// d - 1's). fk_keys copies keys of rows [r0, n_rows) to keys[0 ..); fk_gather copies rows sel[0, m) whole; fk_format writes
// their text lines (k + 2 S_f + 1 bytes each) to text, whose size must be a multiple of 16 bytes covering m lines.
constexpr uint32_t FK_SPLITTERS = 4096;
hipError_t launch_fk_match(const uint64_t* rows, uint64_t stride, uint32_t n_rows, const uint64_t* L, uint64_t n,
                           const uint64_t* spl, uint32_t ns, uint64_t B, uint64_t carry_key, bool has_prev, uint64_t* lb,
                           uint64_t* cnt, uint32_t* head, uint32_t* first_desc, hipStream_t st);
size_t fk_scan_temp_bytes(uint32_t max_rows);  // temp storage of fk_select (0: the query failed)
hipError_t launch_fk_select(const uint64_t* rows, uint64_t stride, uint32_t n_rows, const uint64_t* cnt, const uint32_t* head,
                            uint32_t* run_start, uint64_t carry_run, const uint32_t* first_desc, uint8_t* emit, uint32_t* sel,
                            uint32_t* n_sel, uint64_t* info, void* temp, size_t temp_bytes, hipStream_t st);
hipError_t launch_fk_keys(const uint64_t* rows, uint64_t stride, uint32_t r0, uint32_t n_rows, uint64_t* keys, hipStream_t st);
hipError_t launch_fk_gather(const uint64_t* rows, uint64_t stride, const uint32_t* sel, uint32_t m, uint64_t* out, hipStream_t st);
hipError_t launch_fk_format(const uint64_t* rows, uint64_t stride, const uint32_t* sel, uint32_t m, uint32_t k, uint32_t S_f,
                            void* text, hipStream_t st);

// build_kmers_table (build_kernels.hip), on one piece of the all-k-mers list resident on the device: A[0, n) raw words,
// rows n x stride words (stride = 1 + ceil(accessions / 64)). bt_init masks A's flag bits in place and writes rows[r] = [A[r]]
// [zeros]. bt_match takes m raw words of one accession (its flag bits are masked on the fly) and ORs the accession's bit into
// row lower_bound(A, x) wherever that row's key is x; A must not descend, and spl[j] = A[j * B] for all ns = ceil(n / B) <=
// FK_SPLITTERS splitters (masked). *descends (zeroed by the caller) is set to 1 when a word is below the one before it
// (carry_key before word 0 when has_prev).
hipError_t launch_bt_init(uint64_t* A, uint64_t n, uint64_t stride, uint64_t* rows, hipStream_t st);
hipError_t launch_bt_match(const uint64_t* A, uint64_t n, const uint64_t* spl, uint32_t ns, uint64_t B, const uint64_t* slice,
                           uint32_t m, uint64_t carry_key, bool has_prev, uint64_t* rows, uint64_t stride, uint64_t accession,
                           uint32_t* descends, hipStream_t st);

// list_kmers_found_in_multiple_samples (list_kernels.hip), on one piece whose raw words lie in `words` as n_seg segments
// (seg_off / seg_len: one read block of one accession's slice each, non-descending). ll_check looks at one segment as it lands:
// flags[0] = 1 when it descends (carry_key before word 0 when has_prev), flags[1] = min(file) over words with flag 0 (preset
// 0xFFFFFFFF). ll_splitters sorts m regularly sampled keys into `sample`; bucket b of nb is the key range [sample[b m / nb],
// sample[(b + 1) m / nb]). ll_count, one workgroup per bucket, counts the bucket's words per key in an LDS table of `slots`
// (a power of two <= LL_MAX_SLOTS), applies mac and need[count_all] (the smallest count of a strand side that passes, or
// LL_NEED_NONE), stages the passing keys and the no-pass records (key, packed counts: all | canonical << 21 | non-canonical
// << 42) at bk_base[b] and adds the distinct keys to stats: the three (N + 1)^2 matrices (canonical, non-canonical, both), the
// N + 1 shareness counts, TESTED_SHARDS counters of keys below mac. flags[2] = 1: a table filled (nothing of that bucket is
// written), flags[3] = 1: a key counted more than N times (*err_key = the smallest, preset to all ones). bk_* have nb + 1
// entries and are zeroed by the caller. ll_gather scans bk_pass / bk_np into off_pass / off_np (entry nb = the totals) and
// copies the staged records to the contiguous outputs; ll_commit adds a piece's stats to the run's and zeroes them.
constexpr uint32_t LL_MAX_SLOTS = 4096;
constexpr uint32_t LL_NEED_NONE = 0xFFFFFFFFu;
struct ListArgs {
    const uint64_t* words;
    const uint32_t* seg_off;
    const uint32_t* seg_len;
    uint32_t n_seg;
    const uint64_t* sample;
    uint32_t m, nb, slots;
    uint64_t N, mac;
    const uint32_t* need;  // [N + 1]
    uint64_t* stage_pass;  // [words in the piece], as stage_np_key and stage_np_cnt
    uint64_t* stage_np_key;
    uint64_t* stage_np_cnt;
    uint32_t* bk_base;  // [nb + 1], as bk_pass and bk_np
    uint32_t* bk_pass;
    uint32_t* bk_np;
    unsigned long long* stats;  // [3 (N + 1)^2 + (N + 1) + TESTED_SHARDS]
    uint32_t* flags;            // [4]
    unsigned long long* err_key;
};
hipError_t launch_ll_check(const uint64_t* words, uint32_t m, uint64_t carry_key, bool has_prev, uint32_t file, uint32_t* flags,
                           hipStream_t st);
size_t ll_temp_bytes(uint32_t max_sample, uint32_t max_buckets);  // temp storage of ll_splitters and ll_gather (0: the query failed)
hipError_t launch_ll_splitters(const uint64_t* words, uint64_t total, uint32_t m, uint64_t* sample_raw, uint64_t* sample, void* temp,
                               size_t temp_bytes, hipStream_t st);
size_t ll_count_lds_bytes(uint32_t slots);
hipError_t launch_ll_count(const ListArgs& a, hipStream_t st);
hipError_t launch_ll_gather(const ListArgs& a, uint32_t* off_pass, uint32_t* off_np, uint64_t* out_pass, uint64_t* out_np_key,
                            uint64_t* out_np_cnt, void* temp, size_t temp_bytes, hipStream_t st);
hipError_t launch_ll_commit(unsigned long long* total, unsigned long long* piece, uint64_t n, hipStream_t st);

// count_kmers_with_strand (count_kernels.hip), on a base stream resident on the device: bytes, A C G T in either case are bases
// and every other byte separates reads. ck_encode appends the sort words (key << 1) | orient (orient 0: the window is its own
// canonical form) of the windows of kmer_len bases whose canonical key lies in [lo, hi) to words[0, cap), claiming room from
// ctr[0]; ctr[1] counts the orient-1 words among them (both zeroed by the caller). A claim that ends above cap writes nothing:
// ctr[0] > cap afterwards means the pass did not fit, and ctr still holds the true counts. ck_sample writes the canonical keys
// of m regularly spaced windows (all ones where the window is not counted), ck_sort_sample sorts them on all 64 bits. ck_sort
// sorts a pass's n <= CK_MAX_PASS_WORDS words on bits [0, 2 kmer_len + 1). ck_heads writes the positions of the run heads (a
// word whose key differs from its predecessor's) to heads, off[ceil(n / 2048)] = their number; ck_reduce turns run r into its
// count and flags (0x4000... an orient-0 word, 0x8000... an orient-1 word), keeps it iff ci <= count <= cx, writes the kept
// key | flags in order to out (which may be `sorted`; res may not), off[ceil(n_runs / 2048)] = their number, and adds to
// counts[0..6] as kgwas_count_kmers_* documents them. blk and off have ck_blocks(max words of a pass) entries.
constexpr uint64_t CK_MAX_PASS_WORDS = 1ull << 30;
uint32_t ck_blocks(uint64_t max_words);
size_t ck_temp_bytes(uint64_t max_words, uint32_t max_sample, uint32_t kmer_len);  // temp storage of the sorts and scans (0: the query failed)
hipError_t launch_ck_encode(const uint8_t* bases, uint64_t n, uint32_t kmer_len, uint64_t lo, uint64_t hi, uint64_t* words, uint64_t cap,
                            unsigned long long* ctr, hipStream_t st);
hipError_t launch_ck_sample(const uint8_t* bases, uint64_t n, uint32_t kmer_len, uint32_t m, uint64_t* sample, hipStream_t st);
hipError_t launch_ck_sort_sample(const uint64_t* raw, uint64_t* sorted, uint32_t m, void* temp, size_t temp_bytes, hipStream_t st);
hipError_t launch_ck_sort(const uint64_t* words, uint64_t* sorted, uint64_t n, uint32_t kmer_len, void* temp, size_t temp_bytes, hipStream_t st);
hipError_t launch_ck_heads(const uint64_t* sorted, uint64_t n, uint32_t* blk, uint32_t* off, uint32_t* heads, void* temp, size_t temp_bytes,
                           hipStream_t st);
hipError_t launch_ck_reduce(const uint64_t* sorted, uint64_t n, const uint32_t* heads, uint32_t n_runs, uint64_t ci, uint64_t cx, uint64_t* res,
                            uint32_t* blk, uint32_t* off, uint64_t* out, unsigned long long* counts, void* temp, size_t temp_bytes, hipStream_t st);

// Squeeze: out[r][2*W_m dwords] bit i = file bit colmap[i] (colmap[i] == 0xFFFFFFFF -> 0). A block stages 64 file rows
// and 64 squeezed rows in LDS: it exists while W_f + W_m <= SQUEEZE_MAX_WORDS (all of the table phenotyped: up to 10 176
// accessions; any subset or order: up to 20 288 accessions in the table). check_squeeze_fits throws KGWAS_ERR_ARG beyond.
constexpr uint64_t SQUEEZE_MAX_WORDS = 319;
void check_squeeze_fits(const char* who, uint64_t S_f, uint64_t S);
hipError_t launch_squeeze(const uint64_t* file_rows, uint64_t file_stride_w, uint64_t n_rows, const uint32_t* colmap,
                          uint32_t W_m, uint32_t W_f, uint32_t* out, hipStream_t st);

// Synthetic rows.
hipError_t launch_synth(uint64_t* rows, uint64_t first_row, uint64_t n_rows, uint64_t n_acc, uint64_t seed,
                        hipStream_t st);

// Kinship: transpose+filter, then Hamming Gram accumulation into H (S_pad x S_pad u64).
//  T: [S_pad][n_rw] u32, n_rw = ceil(n_rows/64)*2
hipError_t launch_kin_transpose(const uint64_t* file_rows, uint64_t file_stride_w, uint64_t n_rows, uint32_t S_f,
                                uint32_t S_pad, uint32_t min_count, uint32_t* T, uint64_t n_rw,
                                unsigned long long* n_used, hipStream_t st);
// rows per transpose block the LDS allows for this table shape (256, 128, 64; 0 = too many accessions)
uint32_t kin_transpose_rows_per_block(uint64_t file_stride_w, uint32_t S_pad);
// scratch: kin_gram_scratch_bytes(S_pad) bytes (the row slices' partial tiles, reduced into H by a second kernel)
size_t kin_gram_scratch_bytes(uint32_t S_pad);
hipError_t launch_kin_gram(const uint32_t* T, uint64_t n_rw, uint32_t S_pad, unsigned long long* H, void* scratch, size_t scratch_bytes,
                           hipStream_t st);

// clump_kmers (ld_kernels.hip): which pairs of presence/absence rows have r^2 >= tm / 10^6, decided in integers.
//  prep: rows[N][stride_w] (words 0..W-1 of a row are its bits, bit i = accession i) -> P[n_chunks][N_pad] 16-byte chunks of 128
//        accessions (bits at or past n and rows at or past N zero), n1[N_pad] the counts, pq[N_pad] = n1 (n - n1), tq[N_pad] = tm pq.
//        N_pad is a multiple of 128 >= N, n_chunks a multiple of 4 >= ceil(n / 128), n <= 8192, tm <= 10^6.
//  link: rows a of [row0, row0 + n_rows), row0 a multiple of 64, against every row b: out[(a - row0) * pitch_dw + b / 32] bit b % 32
//        = (b > a and the pair is linked). out holds ceil(n_rows / 64) * 64 rows of pitch_dw dwords, pitch_dw a multiple of 4 with
//        32 pitch_dw >= N_pad; every dword of it is written. popcount = true: n11 from the vector ALU instead of the matrix cores
//        (the ablation; the same bits).
// The operands of `count` rows as the launchers take them (device.h's LdOperands owns the memory): P, n1, pq, tq as above with
// N = count and N_pad = pad.
struct LdView {
    void* P;
    uint32_t *n1, *pq;
    uint64_t* tq;
    uint64_t count, pad;
    uint32_t n_chunks;
};
hipError_t launch_ld_prep(const uint64_t* rows, uint64_t stride_w, uint64_t W, uint32_t n, uint32_t tm, const LdView& ops, hipStream_t st);
hipError_t launch_ld_link(const LdView& ops, uint32_t n, uint64_t row0, uint64_t n_rows, uint32_t* out, uint64_t pitch_dw, bool popcount,
                          hipStream_t st);

// proxy_kmers (ld_kernels.hip): L = A.count <= 4096 leads (operands PA[n_chunks][L_pad], n1A, pqA from launch_ld_prep, L_pad a multiple
// of 64) against a piece of R = B.count <= 2^20 rows (PB[n_chunks][R_pad], n1B, tqB, R_pad a multiple of 128); every pair is tested.
//  rect : out[b * pitch_q + a / 64] bit a % 64 = (lead a and row b are linked); out holds R_pad rows of pitch_q >= L_pad / 64 words,
//         the first L_pad / 64 of each are written.
//  count: bcnt[ceil(R / 256)] the records per block of 256 rows, boff[.. + 1] the records before a block and, last, the total.
//  write: the records numbered [win_lo, win_lo + cap) in (row, lead) order, from the blocks [blk0, blk1), to rec[number - win_lo].
//         kmers (may be null: 0): row r's k-mer word is kmers[r * kmer_stride]. The record's layout is kgwas_proxy_record's.
struct ProxyRecord {
    uint64_t row, kmer;
    uint32_t lead, n1, n11, pad;
};
hipError_t launch_ld_rect(const LdView& A, const LdView& B, uint32_t n, uint64_t* out, uint64_t pitch_q, bool popcount, hipStream_t st);
hipError_t launch_ld_proxy_count(const uint64_t* bits, uint64_t pitch_q, uint64_t R, uint32_t* bcnt, uint32_t* boff, hipStream_t st);
hipError_t launch_ld_proxy_write(const uint64_t* bits, uint64_t pitch_q, const uint32_t* boff, uint32_t blk0, uint32_t blk1, uint32_t win_lo,
                                 uint32_t cap, const LdView& A, const LdView& B, const uint64_t* kmers, uint64_t kmer_stride, uint64_t row_base,
                                 ProxyRecord* rec, hipStream_t st);

// The scan of the count / scan / write scheme, shared by proxy_kmers and locate_kmers: boff[b] = bcnt[0] + .. + bcnt[b - 1] for
// b <= n_blocks (boff[n_blocks]: the total), by one workgroup.
hipError_t launch_block_offsets(const uint32_t* bcnt, uint32_t n_blocks, uint32_t* boff, hipStream_t st);

// locate_kmers (locate_kernels.hip). A LocateList is the queries' patterns sorted by (key, id): keys[n] the sort
// key (d = 0: the code itself, and codes == keys; d = 1: the first ceil(k / 2) bases for H, the last floor(k / 2) for L), codes[n]
// the pattern's whole code, ids[n] = kmer << 1 | strand, and spl[ns] = keys[j * B] the splitters, ns = ceil(n / B) <=
// LOCATE_SPLITTERS. An empty list has n = ns = 0.
//  count: the windows at positions [0, n_win) of bases[0, n_buf), n_win <= n_buf, n_win <= LOCATE_MAX_PIECE (a window has at most
//         3 k + 1 <= 94 hits - the codes within one mismatch of it, and no two patterns share a code -, so a piece's records are
//         below 2^32); bcnt[tile] the records of a tile of 4096 positions, boff[.. + 1] the records before a tile and, last, the
//         total; *windows += the windows of k bases.
//  write: the records numbered [win_lo, win_lo + cap) in (pos, kmer, strand) order, from the tiles [tile0, tile1), to
//         rec[number - win_lo]; pos = pos0 + the window's position. The record's layout is kgwas_locate_record's.
constexpr uint32_t LOCATE_SPLITTERS = 2048;
constexpr uint64_t LOCATE_MAX_PIECE = 1ull << 25;
struct LocateList {
    const uint64_t *spl, *keys, *codes;
    const uint32_t* ids;
    uint64_t n, B;
    uint32_t ns;
};
struct LocateRecord {
    uint64_t pos;
    uint32_t kmer;
    uint8_t strand, mismatches, offset, pad;
};
uint32_t locate_tiles(uint64_t n_win);
hipError_t launch_locate_count(const uint8_t* bases, uint64_t n_buf, uint64_t n_win, uint32_t kmer_len, uint32_t mismatches, const LocateList& H,
                               const LocateList& L, uint32_t* bcnt, uint32_t* boff, unsigned long long* windows, hipStream_t st);
hipError_t launch_locate_write(const uint8_t* bases, uint64_t n_buf, uint64_t n_win, uint32_t kmer_len, uint32_t mismatches, const LocateList& H,
                               const LocateList& L, const uint32_t* boff, uint32_t tile0, uint32_t tile1, uint32_t win_lo, uint32_t cap, uint64_t pos0,
                               LocateRecord* rec, hipStream_t st);

// fetch_reads (fetch_kernels.hip). A piece is bases[0, n), n <= LOCATE_MAX_PIECE, whole reads that each end with
// '\n'; n_reads is the count of its newlines, which the host knows. Q is ONE LocateList of the queries' canonical codes (codes ==
// keys), ids[i] = query << 1 | (the canonical code is the reverse complement of the query as spelled).
//  filter: filter[FETCH_FILTER_WORDS] = the presence bitmap of Q's keys.
//  mark:   marks[tiles * 256] (16 bits per lane: a plain bitmap over the piece's positions) = the windows that spell a query;
//          kmer_windows[query] += its hit windows, *windows += the windows of k bases; nlcnt[tiles] / nloff[tiles + 1] the tiles'
//          newline counts and their scan. filter == nullptr: no prefilter.
//  count:  starts[n_reads + 1] from nloff; bcnt[block] the kept reads among a block of 256 reads, boff[.. + 1] their scan.
//  write:  the records numbered [win_lo, win_lo + cap) in read order, from the read blocks [blk0, blk1), to rec[number - win_lo];
//          read = read0 + the read's number in the piece. The record's layout is kgwas_fetch_record's.
constexpr uint32_t FETCH_FILTER_BITS = 18;
constexpr uint32_t FETCH_FILTER_WORDS = 1u << (FETCH_FILTER_BITS - 5);
struct FetchRecord {
    uint64_t read;
    uint32_t n_hits, first_pos, kmer;
    uint8_t strand, pad[3];
};
inline uint32_t fetch_read_blocks(uint32_t n_reads) { return (n_reads + 255u) / 256u; }
hipError_t launch_fetch_filter(const LocateList& Q, uint32_t* filter, hipStream_t st);
hipError_t launch_fetch_mark(const uint8_t* bases, uint64_t n, uint32_t kmer_len, const LocateList& Q, const uint32_t* filter, uint16_t* marks,
                             uint32_t* nlcnt, uint32_t* nloff, unsigned long long* kmer_windows, unsigned long long* windows, hipStream_t st);
hipError_t launch_fetch_count(const uint8_t* bases, uint64_t n, uint32_t kmer_len, uint32_t min_hits, const uint16_t* marks, const uint32_t* nloff,
                              uint32_t n_reads, uint32_t* starts, uint32_t* bcnt, uint32_t* boff, hipStream_t st);
hipError_t launch_fetch_write(const uint8_t* bases, uint64_t n, uint32_t kmer_len, uint32_t min_hits, const LocateList& Q, const uint16_t* marks,
                              const uint32_t* starts, uint32_t n_reads, const uint32_t* boff, uint32_t blk0, uint32_t blk1, uint32_t win_lo, uint32_t cap,
                              uint64_t read0, FetchRecord* rec, hipStream_t st);

}  // namespace kgwas
