// clump.cpp — kgwas_kmers_ld and kgwas_clump_kmers_run: the significant k-mers of an association file grouped by exact r^2
// (DESIGN.md 4.13). A tool of this project's own: the reference ends with the list of k-mers that pass the threshold.
//
// ld_blocks   the link matrix's upper triangle of rows on the device, block of rows by block: ld_link_kernel on one stream, the
//             block's copy back on a second with an event of its own, the consumer on the host - block i is consumed while block
//             i + 1 is computed. Two device blocks and two pinned blocks take turns.
// run         assoc file -> hits in p order -> the table and their rows from it (table_session.h: kgwas_filter_kmers' search) ->
//             squeezed to the phenotype's accessions -> ld_blocks -> the streaming clump pass (clump_host.h) -> the output and its log.
#include <cstring>
#include <functional>

#include "clump_host.h"
#include "device.h"
#include "kernels.h"
#include "table_session.h"

using namespace kgwas;
using namespace kgwas::clump;

namespace {

constexpr uint64_t LD_BLOCK_BYTES = 256ull << 20;

// consume(row0, rows, block, pitch_dw): rows [row0, row0 + rows) of the link matrix, on the host, valid until it returns
typedef std::function<void(uint64_t, uint64_t, const uint32_t*, uint64_t)> Consume;

// d_rows[N][stride_w]: words 0..W-1 of a row are its bits. n1_out (host, may be null) gets the counts; *kernel_ms the kernels' time.
void ld_blocks(const uint64_t* d_rows, uint64_t stride_w, uint64_t W, uint64_t N, uint64_t n, uint32_t tm, uint64_t tile_rows, uint32_t* n1_out,
               double* kernel_ms, const Consume& consume) {
    if (kernel_ms) *kernel_ms = 0;
    if (!N) return;
    const bool popcount = opt_set("KGWAS_LD_POPCOUNT");  // the ablation: n11 on the vector ALU (the same bits)
    const uint64_t N_pad = (N + 127) / 128 * 128, pitch = N_pad / 32;
    if (!tile_rows) tile_rows = std::max<uint64_t>(64, LD_BLOCK_BYTES / (pitch * 4) / 64 * 64);
    tile_rows = std::min((tile_rows + 63) / 64 * 64, (N + 63) / 64 * 64);
    const uint64_t n_blocks = (N + tile_rows - 1) / tile_rows;

    LdOperands ops;
    DevBuf<uint32_t> d_adj[2];
    PinBuf<uint32_t> h_adj[2];
    Event ev_start[2], ev_done[2], ev_copied[2], p0, p1;  // (start, done and p0, p1 time the kernels alone)
    ops.alloc(N_pad, n);
    const LdView v = ops.view(N, N_pad);
    for (int i = 0; i < 2 && (uint64_t)i < n_blocks; i++) {
        d_adj[i].alloc(tile_rows * pitch);
        h_adj[i].alloc(tile_rows * pitch);
        ev_start[i].create();
        ev_done[i].create();
        ev_copied[i].create(hipEventDisableTiming | hipEventBlockingSync);
    }
    p0.create();
    p1.create();
    Stream s_run, s_copy;  // (declared after the buffers their work uses: they go first, idle)
    s_run.create(hipStreamNonBlocking);
    s_copy.create(hipStreamNonBlocking);

    KGWAS_HIP(hipEventRecord(p0, s_run));
    KGWAS_HIP(launch_ld_prep(d_rows, stride_w, W, (uint32_t)n, tm, v, s_run));
    KGWAS_HIP(hipEventRecord(p1, s_run));
    double ms_sum = 0;
    auto rows_of = [&](uint64_t i) { return std::min(tile_rows, N - i * tile_rows); };
    auto finish = [&](uint64_t i) {  // block i is on the host: hand it over
        float ms = 0;
        KGWAS_HIP(hipEventSynchronize(ev_copied[i & 1]));
        KGWAS_HIP(hipEventElapsedTime(&ms, ev_start[i & 1], ev_done[i & 1]));
        ms_sum += ms;
        consume(i * tile_rows, rows_of(i), h_adj[i & 1].p, pitch);
    };
    for (uint64_t i = 0; i < n_blocks; i++) {
        const int k = (int)(i & 1);
        if (i >= 2) KGWAS_HIP(hipStreamWaitEvent(s_run, ev_copied[k], 0));  // the device block is free once its last copy is through
        KGWAS_HIP(hipEventRecord(ev_start[k], s_run));
        KGWAS_HIP(launch_ld_link(v, (uint32_t)n, i * tile_rows, rows_of(i), d_adj[k].p, pitch, popcount, s_run));
        KGWAS_HIP(hipEventRecord(ev_done[k], s_run));
        KGWAS_HIP(hipStreamWaitEvent(s_copy, ev_done[k], 0));
        // (the pinned block k was consumed in the turn before this one, before anything was queued here)
        KGWAS_HIP(hipMemcpyAsync(h_adj[k].p, d_adj[k].p, (rows_of(i) + 63) / 64 * 64 * pitch * 4, hipMemcpyDeviceToHost, s_copy));
        KGWAS_HIP(hipEventRecord(ev_copied[k], s_copy));
        if (i >= 1) finish(i - 1);
    }
    finish(n_blocks - 1);
    if (n1_out) KGWAS_HIP(hipMemcpyAsync(n1_out, v.n1, N * 4, hipMemcpyDeviceToHost, s_run));
    KGWAS_HIP(hipStreamSynchronize(s_run));
    float ms = 0;
    KGWAS_HIP(hipEventElapsedTime(&ms, p0, p1));
    if (kernel_ms) *kernel_ms = ms_sum + ms;
}

void kmers_ld(const uint64_t* bits, uint64_t n_kmers, uint64_t W, uint64_t n_acc, uint32_t tm, int32_t device, uint64_t tile_rows, uint32_t* adj,
              uint32_t* n1) {
    if (!bits || !adj) throw Error(KGWAS_ERR_ARG, "kgwas_kmers_ld: null argument");
    check_clump_shape("kgwas_kmers_ld", n_kmers, n_acc, tm);
    if (W < (n_acc + 63) / 64) throw Error(KGWAS_ERR_ARG, "kgwas_kmers_ld: words_per_row is too small for n_acc");
    if (!n_kmers) return;
    use_device(device);
    DevBuf<uint64_t> d_rows;
    d_rows.alloc(n_kmers * W);
    KGWAS_HIP(hipMemcpy(d_rows.p, bits, n_kmers * W * 8, hipMemcpyHostToDevice));
    const uint64_t n_dw = (n_kmers + 31) / 32;
    double kernel_ms = 0;
    ld_blocks(d_rows.p, W, W, n_kmers, n_acc, tm, tile_rows, n1, &kernel_ms, [&](uint64_t row0, uint64_t rows, const uint32_t* blk, uint64_t pitch) {
        for (uint64_t r = 0; r < rows; r++) memcpy(adj + (row0 + r) * n_dw, blk + r * pitch, n_dw * 4);
    });
    if (opt_set("KGWAS_LD_TIMING")) fprintf(stderr, "[kgwas] kmers_ld: k-mers=%llu accessions=%llu kernels_ms=%.3f\n", (unsigned long long)n_kmers, (unsigned long long)n_acc, kernel_ms);
}

void run(const char* table_base, uint32_t kmer_len, const char* pheno_path, const char* assoc_path, uint32_t tm, double p_max, int32_t device,
         uint64_t tile_rows, const char* out_path, kgwas_clump_stats* st) {
    if (!table_base || !assoc_path || !out_path) throw Error(KGWAS_ERR_ARG, "kgwas_clump_kmers_run: null argument");
    if (tm == 0 || tm > 1000000) throw Error(KGWAS_ERR_ARG, "kgwas_clump_kmers_run: r2_millionths must be within 1..1000000");
    if (kmer_len < 1 || kmer_len > 32) throw Error(KGWAS_ERR_ARG, "kgwas_clump_kmers_run: k-mers of 1 to 32 bases are supported");
    if (std::isnan(p_max)) throw Error(KGWAS_ERR_ARG, "kgwas_clump_kmers_run: p_max is not a number");
    const double t_start = now_ms();
    // 1, 2: the hits, before the table is looked for
    const std::vector<Hit> hits = read_assoc(assoc_path, kmer_len, kgwas_kmer_encode);
    const std::vector<uint32_t> order = p_order(hits, p_max);
    const uint64_t N = order.size();
    TableSession ts;
    if (pheno_path) ts.load_pheno(pheno_path);
    ts.open_table(table_base, kmer_len);
    ts.refuse_duplicate_accessions();
    ts.check_squeeze_fits("clump_kmers");
    const std::vector<uint64_t> mask = ts.accession_mask();
    const uint64_t n = ts.S, W_f = ts.W_f, stride = ts.stride();
    check_clump_shape("clump_kmers", N, n, tm);

    kgwas_clump_stats s{};
    s.hits_read = hits.size();
    s.hits_used = N;
    s.accessions = n;
    PlacedRows placed;  // the hits' rows, in p order
    std::vector<uint32_t> n1(N);
    Clumper cl(N);
    if (N) {
        // 3: the rows, by the table's own search
        double t = now_ms();
        std::vector<uint64_t> codes(N);
        for (uint64_t i = 0; i < N; i++) codes[i] = hits[order[i]].code;
        placed = ts.rows_of_codes(codes, device);
        if (placed.missing != PlacedRows::NONE)
            throw Error(KGWAS_ERR_FORMAT, "the k-mer " + hits[order[placed.missing]].rs + " of " + assoc_path + " is not in the table " + table_base);
        s.search_ms = now_ms() - t;

        // 4, 5: squeeze, then the link matrix block by block; 6: the clump pass as the blocks arrive
        use_device(device);
        DevBuf<uint64_t> d_rows;
        DevBuf<uint32_t> d_sq;
        Squeezer sq;
        d_rows.alloc(N * stride);
        KGWAS_HIP(hipMemcpy(d_rows.p, placed.rows.data(), N * stride * 8, hipMemcpyHostToDevice));
        const uint64_t* d_bits = d_rows.p + 1;
        uint64_t d_stride = stride, d_W = W_f;
        if (pheno_path) {
            sq.create(ts.col.data(), n, W_f);
            d_sq.alloc(N * sq.words_per_row());
            sq.run(d_rows.p, stride, N, d_sq.p, nullptr);
            KGWAS_HIP(hipStreamSynchronize(nullptr));
            d_bits = reinterpret_cast<const uint64_t*>(d_sq.p);
            d_stride = d_W = sq.W_m;
        }
        double clump_ms = 0, kernel_ms = 0;
        ld_blocks(d_bits, d_stride, d_W, N, n, tm, tile_rows, n1.data(), &kernel_ms, [&](uint64_t row0, uint64_t nr, const uint32_t* blk, uint64_t pitch) {
            const double t0 = now_ms();
            cl.block(row0, nr, blk, pitch);
            clump_ms += now_ms() - t0;
        });
        s.ld_ms = kernel_ms;
        s.clump_ms = clump_ms;
    }
    s.clumps = cl.leads.size();
    s.linked_pairs = cl.pairs;

    // 7: one line per used hit, in the file's order
    std::vector<uint32_t> clump_no(N, 0), size_of(cl.leads.size(), 0), place_of(hits.size(), 0xFFFFFFFFu);
    for (uint64_t k = 0; k < cl.leads.size(); k++) clump_no[cl.leads[k]] = (uint32_t)(k + 1);
    for (uint64_t i = 0; i < N; i++) {
        place_of[order[i]] = (uint32_t)i;
        size_of[clump_no[cl.lead_of[i]] - 1]++;
    }
    for (uint32_t z : size_of) s.largest_clump = std::max<uint64_t>(s.largest_clump, z);
    std::string text = header_line();
    for (size_t h = 0; h < hits.size(); h++) {
        const uint32_t i = place_of[h];
        if (i == 0xFFFFFFFFu) continue;
        const uint32_t l = cl.lead_of[i];
        const uint32_t n11 = count_and(&placed.rows[i * stride + 1], &placed.rows[l * stride + 1], mask.data(), W_f);
        append_line(text, hits[h], clump_no[l], hits[order[l]], l == i, n, n1[i], n1[l], n11);
    }
    write_text(out_path, text);
    // 8: the log
    char log[4096];
    const int ll = snprintf(log, sizeof(log),
                            "clump_kmers: k-mers grouped by exact r2 (linked iff r2 >= the threshold)\nkmers_table\t%s\nkmers_len\t%u\nphenotypes\t%s\n"
                            "assoc\t%s\nr2\t%s\np_max\t%g\naccessions\t%llu\nhits_read\t%llu\nhits_used\t%llu\nclumps\t%llu\nlargest_clump\t%llu\n"
                            "linked_pairs\t%llu\nms: search=%.3f ld=%.3f clump=%.3f total=%.3f\n",
                            table_base, kmer_len, pheno_path ? pheno_path : "(none: every accession of the table)", assoc_path, r2_text(tm).c_str(), p_max,
                            (unsigned long long)s.accessions, (unsigned long long)s.hits_read, (unsigned long long)s.hits_used,
                            (unsigned long long)s.clumps, (unsigned long long)s.largest_clump, (unsigned long long)s.linked_pairs, s.search_ms, s.ld_ms,
                            s.clump_ms, now_ms() - t_start);
    if (ll < 0) throw Error(KGWAS_ERR_IO, std::string("can't write ") + out_path + ".log.txt");
    write_text(std::string(out_path) + ".log.txt", std::string(log, std::min((size_t)ll, sizeof(log) - 1)));
    if (st) *st = s;
}

}  // namespace

extern "C" {

int kgwas_r2_millionths(const char* text, uint32_t* r2_millionths_out) {
    return guarded([&] {
        if (!text || !r2_millionths_out) throw Error(KGWAS_ERR_ARG, "kgwas_r2_millionths: null argument");
        *r2_millionths_out = r2_millionths(text);
    });
}

int kgwas_kmers_ld(const uint64_t* bits, uint64_t n_kmers, uint64_t words_per_row, uint64_t n_acc, uint32_t r2_millionths, int32_t device,
                   uint64_t tile_rows, uint32_t* adj, uint32_t* n1) {
    return guarded([&] { kmers_ld(bits, n_kmers, words_per_row, n_acc, r2_millionths, device, tile_rows, adj, n1); });
}

int kgwas_clump_kmers_run(const char* table_base, uint32_t kmer_len, const char* pheno_path, const char* assoc_path, uint32_t r2_millionths,
                          double p_max, int32_t device, uint64_t tile_rows, const char* out_path, kgwas_clump_stats* st) {
    return guarded([&] { run(table_base, kmer_len, pheno_path, assoc_path, r2_millionths, p_max, device, tile_rows, out_path, st); });
}

}  // extern "C"
