// lmm_table.cpp — the k-mers table route of kgwas_lmm_* (lmm_lrt --kmers_table): every row of a k-mers table goes
// through the mixed-model test without a .bed in between.
//
// test_table: per piece of rows the device squeezes them to phenotype order, flags the rows that kmers_table_to_bed would write
//            AND prep would test, and compacts those into code rows and LmmVariants with prep's bits (lmm_table_kernels.hip);
//            rotate, grid and refine then run over them unchanged (lmm.cpp's single_backend). The host keeps the best N by
//            (lrt, table row);
// test_table_unique: test_table with a pattern cache on the device (--pattern_cache): a code row met before is not rotated again;
// test_table_multi_skip: test_table_multi with a table of the patterns that can no longer ship a pair (--pattern_skip): a row with
//            such a pattern is not computed again;
// test_table_multi: several phenotype columns against ONE table in one pass (the phenotype and its permutations). The front end and
//            the rotation run once per row, the xt yt sums and the refinement per block of LMM_PBLOCK columns (lmm.cpp's
//            multi_front and multi_block), and a select kernel hands the host only the (column, row) pairs that can still enter a
//            column's best N. Every kept row and number has the bits of test_table's for that column.
#include <algorithm>
#include <cmath>
#include <condition_variable>
#include <exception>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "kernels.h"
#include "lmm_internal.h"
#include "piece_reader.h"

using namespace kgwas;
using namespace kgwas::lmm;

namespace {

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

// What test_table, test_table_unique, test_table_multi and test_table_multi_skip share: the checks, the pieces and the front end.
// Per piece the rows are squeezed, flagged and compacted (lmm_table_kernels.hip). prepare(piece) runs after the checks and before
// any device work (the null models; `piece` is the most rows a piece has, and so the most tested rows per_piece gets);
// per_piece(total, codes, vars, row, kmer) gets a piece's compacted tested rows on the device, total > 0 of them, and is done
// with them when it returns. `who` starts the messages; a tested row counts `weight` times in the stats' variants_tested.
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
    const uint64_t piece = piece_rows(n_rows, 1 + W_f, 64ull << 20, 1u << 18, 1u << 20, "KGWAS_LMM_PIECE_ROWS");  // about 64 MiB, at most 2^18
    prepare(piece);
    KGWAS_HIP(hipSetDevice(h->device));
    const uint64_t stride = 1 + W_f;
    const uint64_t n_blocks = (piece + LMM_TABLE_BLOCK - 1) / LMM_TABLE_BLOCK;

    Squeezer sq;
    DevBuf<uint32_t> d_sq, d_n1flag, d_bcnt, d_boff, d_total;
    DevBuf<uint64_t> d_rows, d_row, d_kmer;
    DevBuf<uint8_t> d_codes;
    DevBuf<LmmVariant> d_vars;
    sq.create(col, S, W_f);
    d_rows.alloc(piece * stride);
    d_sq.alloc(piece * sq.words_per_row());
    d_n1flag.alloc(piece);
    d_bcnt.alloc(n_blocks);
    d_boff.alloc(n_blocks);
    d_total.alloc(1);
    d_codes.alloc(piece * h->dm.bpsp);
    d_vars.alloc(piece);
    d_row.alloc(piece);
    d_kmer.alloc(piece);
    PieceReader reader(t, n_rows, piece, stride);

    hipStream_t st = h->stream;
    rows_read = rows_tested = 0;
    for (uint64_t k = 0, pos = 0; pos < n_rows; k++, pos += piece) {
        const uint64_t c = std::min(piece, n_rows - pos);
        const uint64_t* h_rows = reader.wait(k);
        uint32_t total = 0;
        KGWAS_HIP(hipMemcpyAsync(d_rows.p, h_rows, c * stride * 8, hipMemcpyHostToDevice, st));
        h->timer.begin(st);
        sq.run(d_rows.p, stride, c, d_sq.p, st);
        KGWAS_HIP(launch_lmm_table_front(d_rows.p, stride, d_sq.p, (uint32_t)c, sq.W_m, h->dm, pos, (uint32_t)std::min<uint64_t>(min_count, 0xFFFFFFFFu),
                                         maf, d_n1flag.p, d_bcnt.p, d_boff.p, d_total.p, d_codes.p, d_vars.p, d_row.p, d_kmer.p, st));
        h->timer.end(&kgwas_lmm_stats::rotate_ms, st);
        KGWAS_HIP(hipMemcpyAsync(&total, d_total.p, sizeof(total), hipMemcpyDeviceToHost, st));
        KGWAS_HIP(hipStreamSynchronize(st));
        reader.release(k);  // the rows are on the device: the buffer goes back to the reader
        h->timer.collect(h->st);
        if (total > c) throw Error(KGWAS_ERR_STATE, who + ": the front end counted more tested rows than rows");
        if (total) per_piece(total, (const uint8_t*)d_codes.p, (const LmmVariant*)d_vars.p, (const uint64_t*)d_row.p, (const uint64_t*)d_kmer.p);
        rows_read += c;
        rows_tested += total;
        h->st.variants_read += c;
        h->st.variants_tested += total * weight;
    }
}

// The results of up to `rows` compacted tested rows on their way from the device to a heap of the single-phenotype routes.
struct RowStage {
    std::vector<double> lrt, lam, p;
    std::vector<LmmVariant> vars;
    std::vector<uint64_t> row, kmer;
    void resize(uint64_t rows) { lrt.resize(rows), lam.resize(rows), p.resize(rows), vars.resize(rows), row.resize(rows), kmer.resize(rows); }
    // copies n rows' six arrays to the host, waits for the stream, collects the open timer interval and offers the rows in row order
    void offer(kgwas_lmm* h, uint32_t n, const double* d_lrt, const double* d_lam, const double* d_p, const LmmVariant* d_vars,
               const uint64_t* d_row, const uint64_t* d_kmer, std::vector<TableHit>& heap, uint64_t best_n) {
        hipStream_t st = h->stream;
        KGWAS_HIP(hipMemcpyAsync(lrt.data(), d_lrt, n * sizeof(double), hipMemcpyDeviceToHost, st));
        KGWAS_HIP(hipMemcpyAsync(lam.data(), d_lam, n * sizeof(double), hipMemcpyDeviceToHost, st));
        KGWAS_HIP(hipMemcpyAsync(p.data(), d_p, n * sizeof(double), hipMemcpyDeviceToHost, st));
        KGWAS_HIP(hipMemcpyAsync(vars.data(), d_vars, n * sizeof(LmmVariant), hipMemcpyDeviceToHost, st));
        KGWAS_HIP(hipMemcpyAsync(row.data(), d_row, n * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        KGWAS_HIP(hipMemcpyAsync(kmer.data(), d_kmer, n * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        KGWAS_HIP(hipStreamSynchronize(st));
        h->timer.collect(h->st);
        for (uint32_t v = 0; v < n; v++) heap_offer(heap, best_n, TableHit{lrt[v], lam[v], p[v], vars[v].af, row[v], kmer[v]});
    }
};

// The pattern table of test_table_unique and test_table_multi_skip (lmm_table_kernels.hip, "the pattern table"): the slots on the
// device, which live for one call, and what a look-up leaves of a piece. The constructor checks max_patterns and takes the power
// of two of slots below it, at least 64, before any device work; alloc() allocates for pieces of `piece` rows and empties the table
// on the handle's stream.
class PatternTable {
  public:
    enum Extra { RESULTS, STATE };  // what a slot holds beside its tag, owner and code row: lrt, lam, p, or a state word
    struct Found {
        uint64_t kinds[LMM_ROW_LIVE + 1];  // the piece's rows per class
        uint32_t total2;                   // the rows to compute
    };
    LmmCache cache{};
    LmmPiece pc{};
    std::vector<uint32_t> cls;  // the host's copy of the classes of the piece looked up last

    PatternTable(kgwas_lmm* h, const std::string& who, uint64_t max_patterns, Extra extra) : h_(h), who_(who), extra_(extra) {
        if (max_patterns < 64) throw Error(KGWAS_ERR_ARG, who + ": max_patterns is below 64");
        uint32_t slots = 64;
        while (slots < (1u << 30) && 2ull * slots <= max_patterns) slots *= 2;
        cache.slots = slots;
        const long long tag_bits = opt_int("KGWAS_LMM_PATTERN_TAG_BITS", 64);
        tag_mask_ = tag_bits >= 1 && tag_bits < 64 ? (1ull << tag_bits) - 1 : ~0ull;
    }

    // with_rows: the look-up also compacts the rows' table index and k-mer word (row2, kmer2)
    void alloc(uint64_t piece, bool with_rows) {
        const uint64_t slots = cache.slots, bpsp = h_->dm.bpsp;
        hipStream_t st = h_->stream;
        KGWAS_HIP(hipSetDevice(h_->device));
        cls.resize(piece);
        tag_.alloc(slots), owner_.alloc(slots), key_.alloc(slots * (bpsp / 4));
        res_.alloc(extra_ == RESULTS ? 3 * slots : 0), state_.alloc(extra_ == STATE ? slots : 0);
        row_tag_.alloc(piece), slot_of_.alloc(piece), cls_.alloc(piece), back_.alloc(piece);
        // (the block counts serve the piece's compaction and the count of the dead slots)
        bcnt_.alloc(std::max<uint64_t>(piece, slots) / LMM_TABLE_BLOCK + 1), boff_.alloc(bcnt_.n), total2_.alloc(1);
        codes2_.alloc(piece * bpsp), vars2_.alloc(piece);
        if (with_rows) row2_.alloc(piece), kmer2_.alloc(piece);
        cache = LmmCache{tag_.p, owner_.p, key_.p, res_.p, state_.p, cache.slots};
        pc = LmmPiece{row_tag_.p, slot_of_.p, cls_.p, bcnt_.p, boff_.p, total2_.p, codes2_.p, vars2_.p, back_.p, row2_.p, kmer2_.p};
        KGWAS_HIP(hipMemsetAsync(tag_.p, 0, slots * sizeof(unsigned long long), st));
        KGWAS_HIP(hipMemsetAsync(owner_.p, 0xFF, slots * sizeof(uint32_t), st));  // LMM_CACHE_NO_OWNER
        if (state_.p) KGWAS_HIP(hipMemsetAsync(state_.p, 0, slots * sizeof(uint32_t), st));
    }

    // The look-up of a piece's compacted tested rows (timed into rotate_ms, with the front end and the rotation): every row's class,
    // on the device and in cls, and the rows to compute - `what`, for the message - in pc. The stream is idle when it returns.
    Found lookup(uint32_t total, const uint8_t* d_codes, const LmmVariant* d_vars, const uint64_t* d_row, const uint64_t* d_kmer,
                 const char* what) {
        hipStream_t st = h_->stream;
        if (total > cls.size()) throw Error(KGWAS_ERR_STATE, who_ + ": a piece has more tested rows than the piece has rows");
        Found f{};
        h_->timer.begin(st);
        KGWAS_HIP(launch_lmm_pattern_lookup(d_codes, d_vars, d_row, d_kmer, total, h_->dm, tag_mask_, cache, pc, st));
        h_->timer.end(&kgwas_lmm_stats::rotate_ms, st);
        KGWAS_HIP(hipMemcpyAsync(&f.total2, pc.total2, sizeof(f.total2), hipMemcpyDeviceToHost, st));
        KGWAS_HIP(hipMemcpyAsync(cls.data(), pc.cls, total * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        KGWAS_HIP(hipStreamSynchronize(st));
        h_->timer.collect(h_->st);
        const uint32_t last = extra_ == STATE ? LMM_ROW_LIVE : LMM_ROW_REJECTED;
        for (uint32_t v = 0; v < total; v++) {
            if (cls[v] > last) throw Error(KGWAS_ERR_STATE, who_ + ": a row of no class");
            f.kinds[cls[v]]++;
        }
        if (total - f.kinds[LMM_ROW_CACHED] != f.total2)
            throw Error(KGWAS_ERR_STATE, who_ + ": the rows' classes and the rows to " + what + " differ");
        return f;
    }

    // the number of dead slots (STATE), timed into rotate_ms; collects the intervals still open
    uint32_t count_dead() {
        hipStream_t st = h_->stream;
        uint32_t dead = 0;
        h_->timer.begin(st);
        KGWAS_HIP(launch_lmm_skip_count_dead(cache, pc.block_cnt, pc.block_off, pc.total2, st));
        h_->timer.end(&kgwas_lmm_stats::rotate_ms, st);
        KGWAS_HIP(hipMemcpyAsync(&dead, pc.total2, sizeof(dead), hipMemcpyDeviceToHost, st));
        KGWAS_HIP(hipStreamSynchronize(st));
        h_->timer.collect(h_->st);
        return dead;
    }

  private:
    kgwas_lmm* const h_;
    const std::string who_;
    const Extra extra_;
    uint64_t tag_mask_ = ~0ull;
    DevBuf<unsigned long long> tag_, row_tag_;
    DevBuf<uint32_t> owner_, key_, state_, slot_of_, cls_, back_, bcnt_, boff_, total2_;
    DevBuf<double> res_;
    DevBuf<uint8_t> codes2_;
    DevBuf<LmmVariant> vars2_;
    DevBuf<uint64_t> row2_, kmer2_;
};

// What the four kgwas_lmm_test_table* calls write beside their own arguments: every output is optional. kept[k] goes to the
// arrays from element k best_n on, its size to n_kept[k].
struct TableOut {
    uint64_t *row, *kmer;
    double *lrt, *lambda, *p, *af;
    uint64_t *n_kept, *rows_read, *rows_tested, *pairs_shipped;
    void write(const std::vector<TableHit>* kept, uint32_t n_cols, uint64_t best_n, uint64_t n_read, uint64_t n_tested,
               uint64_t n_shipped = 0) const {
        for (uint32_t k = 0; k < n_cols; k++) {
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
    }
};

}  // namespace

// Every row of table t against y: the best best_n tested rows by lrt, in table row order. The compacted rows of a piece go
// through rotate, grid and refine in sub-chunks of at most h->chunk. The host keeps a heap of best_n results with the worst on top.
void kgwas::lmm::test_table(kgwas_lmm* h, const double* y, kgwas_table* t, const uint64_t* col, uint64_t n_acc, uint64_t min_count,
                            double maf, uint64_t best_n, std::vector<TableHit>& kept, uint64_t& rows_read, uint64_t& rows_tested) {
    const uint64_t chunk = h->chunk;
    std::vector<TableHit> heap;
    RowStage out;
    auto prepare = [&](uint64_t) {
        fit_null(h, y);
        heap.reserve((size_t)std::min<uint64_t>(best_n, 1u << 20));
        out.resize(chunk);
    };
    auto per_piece = [&](uint32_t total, const uint8_t* d_codes, const LmmVariant* d_vars, const uint64_t* d_row, const uint64_t* d_kmer) {
        for (uint64_t sub = 0; sub < total; sub += chunk) {
            const uint32_t cc = (uint32_t)std::min<uint64_t>(chunk, total - sub);
            h->timer.begin(h->stream);
            single_backend(h, d_codes + sub * h->dm.bpsp, d_vars + sub, cc);
            out.offer(h, cc, h->d_lrt.p, h->d_lam.p, h->d_p.p, d_vars + sub, d_row + sub, d_kmer + sub, heap, best_n);
            h->st.chunks++;
        }
    };
    table_pass(h, t, col, n_acc, min_count, maf, best_n, "kgwas_lmm_test_table", 1, prepare, per_piece, rows_read, rows_tested);
    sort_by_row(heap);
    kept.swap(heap);
}

// test_table with a pattern cache of at most max_patterns slots (PatternTable with a result per slot): each distinct code row
// among the tested rows goes through rotate, grid and refine once, every other row with that code row takes the stored lrt, lam
// and p (lmm_table_kernels.hip, "the pattern cache"). Equal code rows give equal LmmVariants and so equal results, whatever their
// chunk and place, and the host is offered every tested row in row order as in test_table: kept has test_table's
// bytes for any cache size, piece and chunk, with colliding tags and with a full cache too. The cache lives for this call: the
// results depend on y and W. u is written only when the call succeeds.
void kgwas::lmm::test_table_unique(kgwas_lmm* h, const double* y, kgwas_table* t, const uint64_t* col, uint64_t n_acc, uint64_t min_count,
                                   double maf, uint64_t best_n, uint64_t max_patterns, std::vector<TableHit>& kept, uint64_t& rows_read,
                                   uint64_t& rows_tested, kgwas_lmm_unique_stats& u) {
    const std::string who = "kgwas_lmm_test_table_unique";
    PatternTable table(h, who, max_patterns, PatternTable::RESULTS);
    const uint64_t chunk = h->chunk, bpsp = h->dm.bpsp;
    std::vector<TableHit> heap;
    kgwas_lmm_unique_stats us{};
    us.slots = table.cache.slots;
    RowStage out;
    DevBuf<double> d_rlrt, d_rlam, d_rp;  // every tested row's result, at its place in the piece
    auto prepare = [&](uint64_t piece) {
        fit_null(h, y);
        heap.reserve((size_t)std::min<uint64_t>(best_n, 1u << 20));
        out.resize(piece);  // the host and device buffers hold a piece, not a chunk
        table.alloc(piece, false);
        d_rlrt.alloc(piece), d_rlam.alloc(piece), d_rp.alloc(piece);
    };
    auto per_piece = [&](uint32_t total, const uint8_t* d_codes, const LmmVariant* d_vars, const uint64_t* d_row, const uint64_t* d_kmer) {
        hipStream_t st = h->stream;
        const PatternTable::Found f = table.lookup(total, d_codes, d_vars, nullptr, nullptr, "rotate");
        const LmmPiece& pc = table.pc;
        h->timer.begin(st);
        for (uint64_t sub = 0; sub < f.total2; sub += chunk) {
            const uint32_t cc = (uint32_t)std::min<uint64_t>(chunk, f.total2 - sub);
            single_backend(h, pc.codes2 + sub * bpsp, pc.vars2 + sub, cc);
            KGWAS_HIP(launch_lmm_cache_scatter(h->d_lrt.p, h->d_lam.p, h->d_p.p, (uint32_t)sub, cc, total, table.cache, pc, d_rlrt.p, d_rlam.p,
                                               d_rp.p, st));
            h->timer.end(&kgwas_lmm_stats::rotate_ms, st);
            h->st.chunks++;
        }
        // after the last sub-chunk: an owner may stand in a later sub-chunk than its copies
        KGWAS_HIP(launch_lmm_cache_fanout(total, table.cache, pc, d_rlrt.p, d_rlam.p, d_rp.p, st));
        h->timer.end(&kgwas_lmm_stats::rotate_ms, st);
        out.offer(h, total, d_rlrt.p, d_rlam.p, d_rp.p, d_vars, d_row, d_kmer, heap, best_n);
        us.patterns_cached += f.kinds[LMM_ROW_OWNER];
        us.rows_from_cache += f.kinds[LMM_ROW_CACHED];
        us.rows_collided += f.kinds[LMM_ROW_COLLIDED];
        us.rows_rejected += f.kinds[LMM_ROW_REJECTED];
        us.rows_rotated += f.total2;
    };
    table_pass(h, t, col, n_acc, min_count, maf, best_n, who, 1, prepare, per_piece, rows_read, rows_tested);
    sort_by_row(heap);
    kept.swap(heap);
    u = us;
}

namespace {

// What test_table_multi and test_table_multi_skip share: the columns' heaps and the pass of a run of compacted tested rows through
// the back end and the select stage. Per sub-chunk of at most h->chunk rows the rotation and the grid sums without y run once; per
// block of LMM_PBLOCK columns the xt yt sums, the refinement and the select kernel, which hands the host only the (column, row)
// pairs that can still enter the column's heap: all of them while the heap is not full, then those with lrt above the heap's worst
// as the host knew it before the launch. The heaps still decide; the per-row arrays stay on the device. `hooks` adds launches
// around that: begin_sub(cc) before a sub-chunk's rotation, after_block(cc, p0, pb) behind a block's select kernels (timed with
// them; h->d_lrtm and h->d_sel_cols are still the block's) and end_sub(sub, cc) behind the sub-chunk's last block. With `cuts`
// (ascending, from 0 to total, no step above h->chunk) the sub-chunks are the runs between two cuts, an empty one left out.
struct MultiPass {
    kgwas_lmm* h;
    uint32_t n_pheno;
    uint64_t best_n;
    std::string who;
    bool select = opt_int("KGWAS_LMM_TABLE_SELECT", 1) != 0;
    std::vector<std::vector<TableHit>> heaps;
    uint64_t pairs_shipped = 0;
    struct NoHooks {
        void begin_sub(uint32_t) {}
        void after_block(uint32_t, uint32_t, uint32_t) {}
        void end_sub(uint64_t, uint32_t) {}
    };

    void prepare(const double* Y, double* logl0, double* lambda0) {
        multi_prepare(h, n_pheno, Y, logl0, lambda0, who.c_str());
        h->ensure_select();
        heaps.resize(n_pheno);
        for (std::vector<TableHit>& hp : heaps) hp.reserve((size_t)std::min<uint64_t>(best_n, 1u << 14));
    }

    template <class Hooks>
    void run(uint32_t total, const uint8_t* d_codes, const LmmVariant* d_vars, const uint64_t* d_row, const uint64_t* d_kmer, Hooks& hooks,
             const std::vector<uint32_t>* cuts = nullptr) {
        const uint64_t chunk = h->chunk, cap = (uint64_t)LMM_PBLOCK * chunk;
        hipStream_t st = h->stream;
        size_t cut = 0;
        for (uint64_t sub = 0, end = 0; sub < total; sub = end) {
            if (cuts && ++cut >= cuts->size()) throw Error(KGWAS_ERR_STATE, who + ": the sub-chunks end before their piece");
            end = cuts ? (*cuts)[cut] : std::min<uint64_t>(sub + chunk, total);
            if (end < sub || end - sub > chunk || end > total) throw Error(KGWAS_ERR_STATE, who + ": a sub-chunk outside its piece");
            if (end == sub) continue;
            const uint32_t cc = (uint32_t)(end - sub);
            const LmmVariant* vars = d_vars + sub;
            hooks.begin_sub(cc);
            h->timer.begin(st);
            multi_front(h, d_codes + sub * h->dm.bpsp, vars, cc);
            for (uint32_t p0 = 0; p0 < n_pheno; p0 += LMM_PBLOCK) {
                const uint32_t pb = std::min(LMM_PBLOCK, n_pheno - p0);
                // what the host knows of the block's heaps now; a NaN lrt ranks as -inf (ranks_before)
                LmmSelectCol sc[LMM_PBLOCK];
                for (uint32_t k = 0; k < pb; k++) {
                    const std::vector<TableHit>& hp = heaps[p0 + k];
                    const bool open = !select || hp.size() < best_n;
                    const double worst = open ? 0.0 : hp.front().lrt;
                    sc[k] = LmmSelectCol{std::isnan(worst) ? -INFINITY : worst, open ? 1u : 0u, 0u};
                }
                KGWAS_HIP(hipMemcpyAsync(h->d_sel_cols.p, sc, pb * sizeof(LmmSelectCol), hipMemcpyHostToDevice, st));
                multi_block(h, vars, cc, p0, pb);
                KGWAS_HIP(launch_lmm_table_select(h->d_lrtm.p, h->d_lamm.p, h->d_pm.p, cc, pb, vars, d_row + sub, d_kmer + sub, h->d_sel_cols.p,
                                                  h->d_sel_cnt.p, h->d_sel_off.p, h->d_sel_total.p, h->d_sel_rec.p, (uint32_t)cap, st));
                hooks.after_block(cc, p0, pb);
                h->timer.end(&kgwas_lmm_stats::refine_ms, st);  // (the select kernels are timed with the refinement)
                uint32_t count = 0;
                KGWAS_HIP(hipMemcpyAsync(&count, h->d_sel_total.p, sizeof(count), hipMemcpyDeviceToHost, st));
                KGWAS_HIP(hipStreamSynchronize(st));  // (sc is read by the copy until here)
                h->timer.collect(h->st);
                if (count > (uint64_t)pb * cc) throw Error(KGWAS_ERR_STATE, who + ": the select kernel counted more survivors than pairs");
                if (count) {
                    KGWAS_HIP(hipMemcpyAsync(h->h_sel_rec.p, h->d_sel_rec.p, count * sizeof(LmmTableRecord), hipMemcpyDeviceToHost, st));
                    KGWAS_HIP(hipStreamSynchronize(st));
                }
                for (uint32_t r = 0; r < count; r++) {
                    const LmmTableRecord& o = h->h_sel_rec.p[r];
                    if (o.col >= pb) throw Error(KGWAS_ERR_STATE, who + ": a survivor record names a column outside its block");
                    heap_offer(heaps[p0 + o.col], best_n, TableHit{o.lrt, o.lam, o.p, o.af, o.row, o.kmer});
                }
                pairs_shipped += count;
            }
            hooks.end_sub(sub, cc);
            h->st.chunks++;
        }
    }

    void finish(std::vector<std::vector<TableHit>>& kept) {
        for (std::vector<TableHit>& hp : heaps) sort_by_row(hp);
        kept.swap(heaps);
    }
};

}  // namespace

// The same for n_pheno columns Y[n_pheno][n] in one pass over the table: the best best_n per column, each with the rows and the
// bits test_table gives for that column alone (MultiPass).
void kgwas::lmm::test_table_multi(kgwas_lmm* h, uint32_t n_pheno, const double* Y, kgwas_table* t, const uint64_t* col, uint64_t n_acc,
                                  uint64_t min_count, double maf, uint64_t best_n, std::vector<std::vector<TableHit>>& kept,
                                  double* logl0, double* lambda0, uint64_t& rows_read, uint64_t& rows_tested, uint64_t& pairs_shipped) {
    const std::string who = "kgwas_lmm_test_table_multi";
    if (!n_pheno) throw Error(KGWAS_ERR_ARG, who + ": n_pheno is 0");  // (before the table's checks)
    MultiPass mp{h, n_pheno, best_n, who};
    MultiPass::NoHooks none;
    pairs_shipped = 0;
    auto prepare = [&](uint64_t) { mp.prepare(Y, logl0, lambda0); };
    auto per_piece = [&](uint32_t total, const uint8_t* d_codes, const LmmVariant* d_vars, const uint64_t* d_row, const uint64_t* d_kmer) {
        mp.run(total, d_codes, d_vars, d_row, d_kmer, none);
        pairs_shipped = mp.pairs_shipped;
    };
    table_pass(h, t, col, n_acc, min_count, maf, best_n, who, n_pheno, prepare, per_piece, rows_read, rows_tested);
    mp.finish(kept);
}

// test_table_multi that skips dead patterns (lmm_table_kernels.hip, "the dead-pattern skip"): a PatternTable of at most max_patterns
// slots with a state word per slot remembers the code rows met and whether an occurrence that went through all n_pheno columns
// shipped no pair. Such a pattern is dead: the heaps were all full, their worst lrt only rises and equal code rows
// give equal lrt in every column, so every later occurrence would ship nothing either, and from the next piece on
// it is left out of the rows that go through MultiPass::run, in test_table_multi's sub-chunks less their dead rows. kept, logl0,
// lambda0 and pairs_shipped are test_table_multi's, byte for byte. The table lives for this call: what ships depends on Y. u is
// written only when the call succeeds.
void kgwas::lmm::test_table_multi_skip(kgwas_lmm* h, uint32_t n_pheno, const double* Y, kgwas_table* t, const uint64_t* col,
                                       uint64_t n_acc, uint64_t min_count, double maf, uint64_t best_n, uint64_t max_patterns,
                                       std::vector<std::vector<TableHit>>& kept, double* logl0, double* lambda0, uint64_t& rows_read,
                                       uint64_t& rows_tested, uint64_t& pairs_shipped, kgwas_lmm_skip_stats& u) {
    const std::string who = "kgwas_lmm_test_table_multi_skip";
    if (!n_pheno) throw Error(KGWAS_ERR_ARG, who + ": n_pheno is 0");  // (before the table's checks)
    PatternTable table(h, who, max_patterns, PatternTable::STATE);
    MultiPass mp{h, n_pheno, best_n, who};
    kgwas_lmm_skip_stats us{};
    us.slots = table.cache.slots;
    pairs_shipped = 0;
    DevBuf<uint32_t> d_shipped;  // per sub-chunk: the rows that shipped a pair
    std::vector<uint32_t> cuts;
    auto prepare = [&](uint64_t piece) {
        mp.prepare(Y, logl0, lambda0);
        table.alloc(piece, true);
        d_shipped.alloc(h->chunk);
    };
    struct Hooks {
        kgwas_lmm* h;
        const PatternTable& table;
        uint32_t* shipped;
        uint32_t total;  // the piece's tested rows
        void begin_sub(uint32_t cc) { KGWAS_HIP(hipMemsetAsync(shipped, 0, cc * sizeof(uint32_t), h->stream)); }
        void after_block(uint32_t cc, uint32_t, uint32_t pb) {
            KGWAS_HIP(launch_lmm_skip_flag(h->d_lrtm.p, h->d_sel_cols.p, cc, pb, shipped, h->stream));
        }
        void end_sub(uint64_t sub, uint32_t cc) {  // (timed with the refinement; collected with the next interval that is)
            h->timer.begin(h->stream);
            KGWAS_HIP(launch_lmm_skip_mark(shipped, (uint32_t)sub, cc, total, table.cache, table.pc, h->stream));
            h->timer.end(&kgwas_lmm_stats::refine_ms, h->stream);
        }
    };
    auto per_piece = [&](uint32_t total, const uint8_t* d_codes, const LmmVariant* d_vars, const uint64_t* d_row, const uint64_t* d_kmer) {
        const PatternTable::Found f = table.lookup(total, d_codes, d_vars, d_row, d_kmer, "compute");
        // The sub-chunks are test_table_multi's, cut every h->chunk tested rows, less their dead rows: every computed row meets the
        // thresholds it meets there, so the pairs shipped are the same ones.
        cuts.assign(1, 0u);
        for (uint32_t v = 0, dead = 0; v < total; v++) {
            dead += table.cls[v] == LMM_ROW_DEAD;
            if ((v + 1) % h->chunk == 0 || v + 1 == total) cuts.push_back(v + 1 - dead);
        }
        us.patterns_cached += f.kinds[LMM_ROW_OWNER];
        us.rows_skipped += f.kinds[LMM_ROW_DEAD];
        us.rows_collided += f.kinds[LMM_ROW_COLLIDED];
        us.rows_rejected += f.kinds[LMM_ROW_REJECTED];
        us.rows_rotated += f.total2;
        Hooks hooks{h, table, d_shipped.p, total};
        const LmmPiece& pc = table.pc;
        if (f.total2) mp.run(f.total2, pc.codes2, pc.vars2, pc.row2, pc.kmer2, hooks, &cuts);
        pairs_shipped = mp.pairs_shipped;
    };
    table_pass(h, t, col, n_acc, min_count, maf, best_n, who, n_pheno, prepare, per_piece, rows_read, rows_tested);
    const uint32_t dead = table.count_dead();  // (collects the last sub-chunk's mark too)
    if (dead > us.patterns_cached) throw Error(KGWAS_ERR_STATE, who + ": more dead slots than slots in use");
    us.patterns_dead = dead;
    mp.finish(kept);
    u = us;
}

extern "C" {

int kgwas_lmm_test_table(kgwas_lmm* h, const double* y, kgwas_table* t, const uint64_t* col, uint64_t n_acc, uint64_t min_count, double maf,
                         uint64_t best_n, uint64_t* row, uint64_t* kmer, double* lrt, double* lambda, double* p, double* af,
                         uint64_t* n_kept, uint64_t* rows_read, uint64_t* rows_tested) {
    return guarded([&] {
        if (!h || !y || !t || !col) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_test_table: null argument");
        std::vector<TableHit> kept;
        uint64_t n_read = 0, n_tested = 0;
        test_table(h, y, t, col, n_acc, min_count, maf, best_n, kept, n_read, n_tested);
        TableOut{row, kmer, lrt, lambda, p, af, n_kept, rows_read, rows_tested, nullptr}.write(&kept, 1, best_n, n_read, n_tested);
    });
}

int kgwas_lmm_test_table_unique(kgwas_lmm* h, const double* y, kgwas_table* t, const uint64_t* col, uint64_t n_acc, uint64_t min_count,
                                double maf, uint64_t best_n, uint64_t* row, uint64_t* kmer, double* lrt, double* lambda, double* p, double* af,
                                uint64_t* n_kept, uint64_t* rows_read, uint64_t* rows_tested, uint64_t max_patterns,
                                kgwas_lmm_unique_stats* u) {
    return guarded([&] {
        if (!h || !y || !t || !col) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_test_table_unique: null argument");
        std::vector<TableHit> kept;
        uint64_t n_read = 0, n_tested = 0;
        kgwas_lmm_unique_stats us{};
        test_table_unique(h, y, t, col, n_acc, min_count, maf, best_n, max_patterns, kept, n_read, n_tested, us);
        TableOut{row, kmer, lrt, lambda, p, af, n_kept, rows_read, rows_tested, nullptr}.write(&kept, 1, best_n, n_read, n_tested);
        if (u) *u = us;
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
        TableOut{row, kmer, lrt, lambda, p, af, n_kept, rows_read, rows_tested, pairs_shipped}.write(kept.data(), n_pheno, best_n, n_read,
                                                                                                     n_tested, n_shipped);
    });
}

int kgwas_lmm_test_table_multi_skip(kgwas_lmm* h, uint32_t n_pheno, const double* Y, kgwas_table* t, const uint64_t* col, uint64_t n_acc,
                                    uint64_t min_count, double maf, uint64_t best_n, uint64_t* row, uint64_t* kmer, double* lrt,
                                    double* lambda, double* p, double* af, uint64_t* n_kept, double* logl0, double* lambda0,
                                    uint64_t* rows_read, uint64_t* rows_tested, uint64_t* pairs_shipped, uint64_t max_patterns,
                                    kgwas_lmm_skip_stats* u) {
    return guarded([&] {
        if (!h || (!Y && n_pheno) || !t || !col) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_test_table_multi_skip: null argument");
        std::vector<std::vector<TableHit>> kept;
        uint64_t n_read = 0, n_tested = 0, n_shipped = 0;
        kgwas_lmm_skip_stats us{};
        test_table_multi_skip(h, n_pheno, Y, t, col, n_acc, min_count, maf, best_n, max_patterns, kept, logl0, lambda0, n_read, n_tested,
                              n_shipped, us);
        TableOut{row, kmer, lrt, lambda, p, af, n_kept, rows_read, rows_tested, pairs_shipped}.write(kept.data(), n_pheno, best_n, n_read,
                                                                                                     n_tested, n_shipped);
        if (u) *u = us;
    });
}

}  // extern "C"
