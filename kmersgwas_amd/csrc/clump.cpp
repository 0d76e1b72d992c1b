// clump.cpp — kgwas_kmers_ld and kgwas_clump_kmers_run: the significant k-mers of an association file grouped by exact r^2
// (DESIGN.md 4.13). A tool of this project's own: the reference ends with the list of k-mers that pass the threshold.
//
// ld_blocks   the link matrix's upper triangle of rows on the device, block of rows by block: ld_link_kernel on one stream, the
//             block's copy back on a second with an event of its own, the consumer on the host - block i is consumed while block
//             i + 1 is computed. Two device blocks and two pinned blocks take turns.
// run         assoc file -> hits in p order -> their rows from the table (kgwas_filter_kmers' search) -> squeezed to the
//             phenotype's accessions -> ld_blocks -> the streaming clump pass (clump_host.h) -> the output and its log.
#include <chrono>
#include <cstring>
#include <functional>

#include "clump_host.h"
#include "device.h"
#include "kernels.h"

using namespace kgwas;
using namespace kgwas::clump;

namespace {

constexpr uint64_t LD_MAX_ACC = 8192, LD_MAX_KMERS = 1ull << 20, LD_BLOCK_BYTES = 256ull << 20;

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

void check_ld_shape(const char* who, uint64_t n_kmers, uint64_t n_acc, uint32_t tm) {
    const std::string w(who);
    if (n_acc == 0 || n_acc > LD_MAX_ACC)
        throw Error(KGWAS_ERR_ARG, w + ": " + std::to_string(n_acc) + " accessions: the exact r2 test is built for 1 to " + std::to_string(LD_MAX_ACC) +
                                       " (its integers are sized for them)");
    if (tm == 0 || tm > 1000000) throw Error(KGWAS_ERR_ARG, w + ": r2_millionths must be within 1..1000000");
    if (n_kmers > LD_MAX_KMERS) throw Error(KGWAS_ERR_ARG, w + ": " + std::to_string(n_kmers) + " k-mers: at most " + std::to_string(LD_MAX_KMERS) + " are clumped at once");
}

// consume(row0, rows, block, pitch_dw): rows [row0, row0 + rows) of the link matrix, on the host, valid until it returns
typedef std::function<void(uint64_t, uint64_t, const uint32_t*, uint64_t)> Consume;

// d_rows[N][stride_w]: words 0..W-1 of a row are its bits. n1_out (host, may be null) gets the counts; *kernel_ms the kernels' time.
void ld_blocks(const uint64_t* d_rows, uint64_t stride_w, uint64_t W, uint64_t N, uint64_t n, uint32_t tm, uint64_t tile_rows, uint32_t* n1_out,
               double* kernel_ms, const Consume& consume) {
    if (kernel_ms) *kernel_ms = 0;
    if (!N) return;
    const bool popcount = opt_set("KGWAS_LD_POPCOUNT");  // the ablation: n11 on the vector ALU (the same bits)
    const uint64_t N_pad = (N + 127) / 128 * 128, pitch = N_pad / 32;
    const uint32_t n_chunks = (uint32_t)((n + 511) / 512 * 4);
    if (!tile_rows) tile_rows = std::max<uint64_t>(64, LD_BLOCK_BYTES / (pitch * 4) / 64 * 64);
    tile_rows = std::min((tile_rows + 63) / 64 * 64, (N + 63) / 64 * 64);
    const uint64_t n_blocks = (N + tile_rows - 1) / tile_rows;

    DevBuf<uint4> d_P;
    DevBuf<uint32_t> d_n1, d_pq, d_adj[2];
    DevBuf<uint64_t> d_tq;
    PinBuf<uint32_t> h_adj[2];
    Event ev_start[2], ev_done[2], ev_copied[2], p0, p1;  // (start, done and p0, p1 time the kernels alone)
    d_P.alloc((size_t)n_chunks * N_pad);
    d_n1.alloc(N_pad);
    d_pq.alloc(N_pad);
    d_tq.alloc(N_pad);
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
    KGWAS_HIP(launch_ld_prep(d_rows, stride_w, W, N, (uint32_t)n, n_chunks, N_pad, tm, d_P.p, d_n1.p, d_pq.p, d_tq.p, s_run));
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
        KGWAS_HIP(launch_ld_link(d_P.p, d_n1.p, d_pq.p, d_tq.p, N, N_pad, (uint32_t)n, n_chunks, i * tile_rows, rows_of(i), d_adj[k].p, pitch, popcount, s_run));
        KGWAS_HIP(hipEventRecord(ev_done[k], s_run));
        KGWAS_HIP(hipStreamWaitEvent(s_copy, ev_done[k], 0));
        // (the pinned block k was consumed in the turn before this one, before anything was queued here)
        KGWAS_HIP(hipMemcpyAsync(h_adj[k].p, d_adj[k].p, (rows_of(i) + 63) / 64 * 64 * pitch * 4, hipMemcpyDeviceToHost, s_copy));
        KGWAS_HIP(hipEventRecord(ev_copied[k], s_copy));
        if (i >= 1) finish(i - 1);
    }
    finish(n_blocks - 1);
    if (n1_out) KGWAS_HIP(hipMemcpyAsync(n1_out, d_n1.p, N * 4, hipMemcpyDeviceToHost, s_run));
    KGWAS_HIP(hipStreamSynchronize(s_run));
    float ms = 0;
    KGWAS_HIP(hipEventElapsedTime(&ms, p0, p1));
    if (kernel_ms) *kernel_ms = ms_sum + ms;
}

void kmers_ld(const uint64_t* bits, uint64_t n_kmers, uint64_t W, uint64_t n_acc, uint32_t tm, int32_t device, uint64_t tile_rows, uint32_t* adj,
              uint32_t* n1) {
    if (!bits || !adj) throw Error(KGWAS_ERR_ARG, "kgwas_kmers_ld: null argument");
    check_ld_shape("kgwas_kmers_ld", n_kmers, n_acc, tm);
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

struct TableOwner {
    kgwas_table* t = nullptr;
    kgwas_pheno* ph = nullptr;
    ~TableOwner() {
        if (t) kgwas_table_close(t);
        if (ph) kgwas_pheno_free(ph);
    }
};
void ck(int rc) {
    if (rc != KGWAS_OK) throw Error(rc, kgwas_last_error());
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
    TableOwner own;
    uint64_t n_pheno = 0, S = 0;
    std::vector<const char*> acc;
    if (pheno_path) {
        ck(kgwas_pheno_load(pheno_path, &own.ph));
        ck(kgwas_pheno_info(own.ph, &n_pheno, &S));
        acc.resize(S);
        for (uint64_t i = 0; i < S; i++) ck(kgwas_pheno_accession(own.ph, i, &acc[i]));
    }
    ck(kgwas_table_open(table_base, kmer_len, &own.t));
    uint64_t S_f = 0, n_rows = 0, W_f = 0;
    uint32_t klen = 0;
    ck(kgwas_table_info(own.t, &S_f, &n_rows, &W_f, &klen));
    std::vector<uint64_t> col, mask(W_f, 0);
    if (pheno_path) {
        col.resize(S);
        ck(kgwas_table_column_map(own.t, acc.data(), S, col.data()));
        for (uint64_t i = 0; i < S; i++) {
            if (mask[col[i] / 64] >> (col[i] % 64) & 1) throw Error(KGWAS_ERR_FORMAT, std::string(pheno_path) + " lists the accession " + acc[i] + " twice");
            mask[col[i] / 64] |= 1ull << (col[i] % 64);
        }
        check_squeeze_fits("clump_kmers", S_f, S);
    } else {
        S = S_f;
        for (uint64_t i = 0; i < S_f; i++) mask[i / 64] |= 1ull << (i % 64);
    }
    const uint64_t n = S;
    check_ld_shape("clump_kmers", N, n, tm);

    kgwas_clump_stats s{};
    s.hits_read = hits.size();
    s.hits_used = N;
    s.accessions = n;
    const uint64_t stride = 1 + W_f;
    std::vector<uint64_t> rows(N * stride);  // the hits' rows, in p order
    std::vector<uint32_t> n1(N);
    Clumper cl(N);
    if (N) {
        // 3: the rows, by the table's own search
        double t = now_ms();
        std::vector<uint64_t> codes(N), found(N * stride);
        for (uint64_t i = 0; i < N; i++) codes[i] = hits[order[i]].code;
        uint64_t n_found = 0;
        ck(kgwas_filter_kmers(own.t, codes.data(), N, device, nullptr, found.data(), &n_found));
        std::unordered_map<uint64_t, uint64_t> at;  // code -> place in p order
        for (uint64_t i = 0; i < N; i++) at.emplace(codes[i], i);
        std::vector<uint8_t> have(N, 0);
        for (uint64_t i = 0; i < n_found; i++) {
            const auto it = at.find(found[i * stride]);
            if (it == at.end() || have[it->second]) continue;  // (a key the table holds twice: its first row)
            have[it->second] = 1;
            memcpy(&rows[it->second * stride], &found[i * stride], stride * 8);
        }
        for (uint64_t i = 0; i < N; i++)
            if (!have[i]) throw Error(KGWAS_ERR_FORMAT, "the k-mer " + hits[order[i]].rs + " of " + assoc_path + " is not in the table " + table_base);
        s.search_ms = now_ms() - t;

        // 4, 5: squeeze, then the link matrix block by block; 6: the clump pass as the blocks arrive
        use_device(device);
        DevBuf<uint64_t> d_rows;
        DevBuf<uint32_t> d_colmap, d_sq;
        d_rows.alloc(N * stride);
        KGWAS_HIP(hipMemcpy(d_rows.p, rows.data(), N * stride * 8, hipMemcpyHostToDevice));
        const uint64_t* d_bits = d_rows.p + 1;
        uint64_t d_stride = stride, d_W = W_f;
        if (pheno_path) {
            const uint32_t W_m = (uint32_t)(2 * ((S + 127) / 128));
            std::vector<uint32_t> colmap(64ull * W_m, 0xFFFFFFFFu);
            for (uint64_t i = 0; i < S; i++) colmap[i] = (uint32_t)col[i];
            d_colmap.alloc(colmap.size());
            KGWAS_HIP(hipMemcpy(d_colmap.p, colmap.data(), colmap.size() * 4, hipMemcpyHostToDevice));
            d_sq.alloc(N * 2 * W_m);
            KGWAS_HIP(launch_squeeze(d_rows.p, stride, N, d_colmap.p, W_m, (uint32_t)W_f, d_sq.p, nullptr));
            KGWAS_HIP(hipStreamSynchronize(nullptr));
            d_bits = reinterpret_cast<const uint64_t*>(d_sq.p);
            d_stride = d_W = W_m;
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
        const uint32_t n11 = count_and(&rows[i * stride + 1], &rows[l * stride + 1], mask.data(), W_f);
        append_line(text, hits[h], clump_no[l], hits[order[l]], l == i, n, n1[i], n1[l], n11);
    }
    auto write_text = [](const std::string& path, const std::string& body) {
        FILE* fo = fopen(path.c_str(), "wb");
        const bool ok = fo && fwrite(body.data(), 1, body.size(), fo) == body.size();
        if ((fo && fclose(fo) != 0) || !ok) throw Error(KGWAS_ERR_IO, "can't write " + path);
    };
    write_text(out_path, text);
    // 8: the log
    char r2_text[16], log[4096];
    snprintf(r2_text, sizeof(r2_text), "%u.%06u", tm / 1000000u, tm % 1000000u);
    const int ll = snprintf(log, sizeof(log),
                            "clump_kmers: k-mers grouped by exact r2 (linked iff r2 >= the threshold)\nkmers_table\t%s\nkmers_len\t%u\nphenotypes\t%s\n"
                            "assoc\t%s\nr2\t%s\np_max\t%g\naccessions\t%llu\nhits_read\t%llu\nhits_used\t%llu\nclumps\t%llu\nlargest_clump\t%llu\n"
                            "linked_pairs\t%llu\nms: search=%.3f ld=%.3f clump=%.3f total=%.3f\n",
                            table_base, kmer_len, pheno_path ? pheno_path : "(none: every accession of the table)", assoc_path, r2_text, p_max,
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
