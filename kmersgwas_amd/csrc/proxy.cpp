// proxy.cpp — kgwas_kmers_ld_proxies and kgwas_proxy_kmers_run: every k-mer of the table in LD with a lead k-mer.
// A tool of this project's own: clump_kmers ends with one lead per signal, this finds the k-mers that travel with each lead.
//
// search   few leads against many rows in one streaming pass. The leads' operands are prepared once and stay on the device; the rows
//          come in pieces through two device buffers that take turns: piece k + 1 is copied on a stream of its own while piece k is
//          squeezed, prepared, linked (ld_rect_kernel: one bit per pair) and compacted into records, which come back in rounds of at
//          most the record buffer's size. What leaves the device is the records alone, in (row, lead) order, the same in every run.
// run      leads file -> the table and their rows from it (table_session.h: kgwas_filter_kmers' search) -> search over the whole
//          table (PieceReader) -> the records bucketed per lead (proxy_host.h) -> the output and its log.
#include <cstring>
#include <functional>

#include "device.h"
#include "kernels.h"
#include "piece_reader.h"
#include "proxy_host.h"
#include "table_session.h"

using namespace kgwas;
using namespace kgwas::proxy;

namespace {

static_assert(sizeof(ProxyRecord) == sizeof(kgwas_proxy_record) && sizeof(ProxyRecord) == 32, "the device's record is the header's");

constexpr uint64_t PROXY_MAX_PIECE = 1ull << 18, PROXY_RECORDS = 1ull << 20;  // a piece: about 64 MiB of rows, at most 2^18
// records of the device buffer (KGWAS_PROXY_RECORDS: the tests' hook)
uint32_t record_cap() {
    const long long forced = opt_int("KGWAS_PROXY_RECORDS", 0);
    return (uint32_t)(forced > 0 ? std::min<long long>(forced, 1ll << 26) : (long long)PROXY_RECORDS);
}

// How a row lies in the host's and the device's row arrays: `stride` words, the bits in words [bit_off, bit_off + W); with a
// colmap (col != null) the rows are squeezed to n accessions in its order first.
struct RowLayout {
    uint64_t stride = 0, bit_off = 0, W = 0;
    const uint64_t* col = nullptr;  // [n] table columns in phenotype order, or null
    bool kmers = false;             // word 0 of a row is its k-mer
};

struct SearchTimes {
    double kernel_ms = 0, copy_ms = 0;
    uint64_t rounds = 0;
};

// wait(k) -> piece k's rows on the host, release(k): they are on the device. consume(records, count): valid until it returns.
typedef std::function<const uint64_t*(uint64_t)> WaitPiece;
typedef std::function<void(uint64_t)> ReleasePiece;
typedef std::function<void(const kgwas_proxy_record*, uint64_t)> ConsumeRecords;

void search(const RowLayout& lay, const uint64_t* lead_rows, uint64_t L, uint64_t n, uint32_t tm, uint64_t n_rows, uint64_t piece, uint32_t* n1_leads,
            const WaitPiece& wait, const ReleasePiece& release, const ConsumeRecords& consume, SearchTimes& times) {
    const bool popcount = opt_set("KGWAS_LD_POPCOUNT");  // the ablation: n11 on the vector ALU (the same records)
    const uint32_t cap = (uint32_t)std::min<uint64_t>(record_cap(), piece * L);  // (a piece has at most piece * L <= 2^30 records)
    const uint64_t L_pad = (L + 63) / 64 * 64, pitch_q = L_pad / 64, P_pad = (piece + 127) / 128 * 128, max_blocks = (piece + 255) / 256;
    const uint64_t n_pieces = (n_rows + piece - 1) / piece;

    DevBuf<uint64_t> d_leads, d_rows[2], d_bits;
    DevBuf<uint32_t> d_sqA, d_sqB, d_bcnt, d_boff;
    Squeezer sq;
    LdOperands opsA, opsB;  // the leads', prepared once, and the piece's
    DevBuf<ProxyRecord> d_rec;
    PinBuf<kgwas_proxy_record> h_rec;
    PinBuf<uint32_t> h_boff;
    Event ev_c0[2], ev_c1[2], ev_k0, ev_k1;
    d_leads.alloc(L * lay.stride);
    for (int i = 0; i < 2 && (uint64_t)i < n_pieces; i++) {
        d_rows[i].alloc(piece * lay.stride);
        ev_c0[i].create();
        ev_c1[i].create();
    }
    opsA.alloc(L_pad, n), opsB.alloc(P_pad, n);
    d_bits.alloc(P_pad * pitch_q);
    d_bcnt.alloc(max_blocks), d_boff.alloc(max_blocks + 1), h_boff.alloc(max_blocks + 1);
    d_rec.alloc(cap), h_rec.alloc(cap);
    ev_k0.create(), ev_k1.create();
    if (lay.col) {
        sq.create(lay.col, n, lay.W);
        d_sqA.alloc(L * sq.words_per_row()), d_sqB.alloc(piece * sq.words_per_row());
    }
    Stream s_run, s_copy;  // (declared after the buffers their work uses: they go first, idle)
    s_run.create(hipStreamNonBlocking);
    s_copy.create(hipStreamNonBlocking);

    // the operands of ops.count rows at d (the layout's), squeezed into d_sq first under a colmap, on s_run
    auto prepare = [&](const uint64_t* d, uint32_t* d_sq, const LdView& ops) {
        const uint64_t* bits = d + lay.bit_off;
        uint64_t stride = lay.stride, W = lay.W;
        if (lay.col) {
            sq.run(d, lay.stride, ops.count, d_sq, s_run);
            bits = reinterpret_cast<const uint64_t*>(d_sq);
            stride = W = sq.W_m;
        }
        KGWAS_HIP(launch_ld_prep(bits, stride, W, (uint32_t)n, tm, ops, s_run));
    };
    auto elapsed = [](hipEvent_t a, hipEvent_t b) {
        float ms = 0;
        KGWAS_HIP(hipEventElapsedTime(&ms, a, b));
        return (double)ms;
    };

    // the leads, once
    KGWAS_HIP(hipMemcpyAsync(d_leads.p, lead_rows, L * lay.stride * 8, hipMemcpyHostToDevice, s_run));
    KGWAS_HIP(hipEventRecord(ev_k0, s_run));
    const LdView A = opsA.view(L, L_pad);
    prepare(d_leads.p, d_sqA.p, A);
    KGWAS_HIP(hipEventRecord(ev_k1, s_run));
    if (n1_leads) KGWAS_HIP(hipMemcpyAsync(n1_leads, A.n1, L * 4, hipMemcpyDeviceToHost, s_run));
    KGWAS_HIP(hipStreamSynchronize(s_run));
    times.kernel_ms += elapsed(ev_k0, ev_k1);

    auto rows_of = [&](uint64_t k) { return std::min(piece, n_rows - k * piece); };
    auto upload = [&](uint64_t k) {  // piece k into device buffer k & 1, which piece k - 2 has left
        const int b = (int)(k & 1);
        const uint64_t* h = wait(k);
        KGWAS_HIP(hipEventRecord(ev_c0[b], s_copy));
        KGWAS_HIP(hipMemcpyAsync(d_rows[b].p, h, rows_of(k) * lay.stride * 8, hipMemcpyHostToDevice, s_copy));
        KGWAS_HIP(hipEventRecord(ev_c1[b], s_copy));
    };
    if (n_pieces) upload(0);
    for (uint64_t k = 0; k < n_pieces; k++) {
        const int b = (int)(k & 1);
        const uint64_t R = rows_of(k);
        const uint32_t n_blocks = (uint32_t)((R + 255) / 256);
        const LdView B = opsB.view(R, (R + 127) / 128 * 128);
        KGWAS_HIP(hipStreamWaitEvent(s_run, ev_c1[b], 0));
        KGWAS_HIP(hipEventRecord(ev_k0, s_run));
        prepare(d_rows[b].p, d_sqB.p, B);
        KGWAS_HIP(launch_ld_rect(A, B, (uint32_t)n, d_bits.p, pitch_q, popcount, s_run));
        KGWAS_HIP(launch_ld_proxy_count(d_bits.p, pitch_q, R, d_bcnt.p, d_boff.p, s_run));
        KGWAS_HIP(hipEventRecord(ev_k1, s_run));
        KGWAS_HIP(hipMemcpyAsync(h_boff.p, d_boff.p, (n_blocks + 1) * 4, hipMemcpyDeviceToHost, s_run));
        KGWAS_HIP(hipEventSynchronize(ev_c1[b]));
        release(k);                          // the rows are on the device: the host buffer goes back to its reader
        if (k + 1 < n_pieces) upload(k + 1);  // ... and the next piece's copy runs beside this piece's kernels
        KGWAS_HIP(hipStreamSynchronize(s_run));
        times.kernel_ms += elapsed(ev_k0, ev_k1);
        times.copy_ms += elapsed(ev_c0[b], ev_c1[b]);
        for (const Round& r : drain_rounds(h_boff.p, n_blocks, cap)) {
            KGWAS_HIP(hipEventRecord(ev_k0, s_run));
            KGWAS_HIP(launch_ld_proxy_write(d_bits.p, pitch_q, d_boff.p, r.blk0, r.blk1, r.lo, cap, A, B, lay.kmers ? d_rows[b].p : nullptr, lay.stride,
                                            k * piece, d_rec.p, s_run));
            KGWAS_HIP(hipEventRecord(ev_k1, s_run));
            KGWAS_HIP(hipMemcpyAsync(h_rec.p, d_rec.p, (size_t)(r.hi - r.lo) * sizeof(ProxyRecord), hipMemcpyDeviceToHost, s_run));
            KGWAS_HIP(hipStreamSynchronize(s_run));
            times.kernel_ms += elapsed(ev_k0, ev_k1);
            times.rounds++;
            consume(h_rec.p, r.hi - r.lo);
        }
    }
}

void kmers_ld_proxies(const uint64_t* lead_bits, uint64_t L, const uint64_t* bits, uint64_t n_rows, uint64_t W, uint64_t n_acc, uint32_t tm,
                      int32_t device, kgwas_proxy_record* out, uint64_t cap, uint64_t* n_out) {
    const char* who = "kgwas_kmers_ld_proxies";
    if (!lead_bits || !n_out || (!bits && n_rows) || (!out && cap)) throw Error(KGWAS_ERR_ARG, std::string(who) + ": null argument");
    check_proxy_shape(who, L, n_acc, tm);
    if (W < (n_acc + 63) / 64) throw Error(KGWAS_ERR_ARG, std::string(who) + ": words_per_row is too small for n_acc");
    *n_out = 0;
    if (!n_rows) return;
    use_device(device);
    RowLayout lay;
    lay.stride = lay.W = W;
    const uint64_t piece = piece_rows(n_rows, W, 64ull << 20, PROXY_MAX_PIECE, PROXY_MAX_PIECE, "KGWAS_PROXY_PIECE_ROWS");
    uint64_t total = 0;
    SearchTimes times;
    search(lay, lead_bits, L, n_acc, tm, n_rows, piece, nullptr, [&](uint64_t k) { return bits + k * piece * W; }, [](uint64_t) {},
           [&](const kgwas_proxy_record* rec, uint64_t count) {
               if (total < cap) memcpy(out + total, rec, std::min(count, cap - total) * sizeof(kgwas_proxy_record));
               total += count;
           },
           times);
    *n_out = total;
    if (opt_set("KGWAS_LD_TIMING"))
        fprintf(stderr, "[kgwas] kmers_ld_proxies: leads=%llu rows=%llu accessions=%llu kernels_ms=%.3f copy_ms=%.3f rounds=%llu\n", (unsigned long long)L,
                (unsigned long long)n_rows, (unsigned long long)n_acc, times.kernel_ms, times.copy_ms, (unsigned long long)times.rounds);
}

void run(const char* table_base, uint32_t kmer_len, const char* pheno_path, const char* leads_path, uint32_t tm, uint64_t max_per_lead, int32_t device,
         const char* out_path, kgwas_proxy_stats* st) {
    const char* who = "kgwas_proxy_kmers_run";
    if (!table_base || !leads_path || !out_path) throw Error(KGWAS_ERR_ARG, std::string(who) + ": null argument");
    if (tm == 0 || tm > 1000000) throw Error(KGWAS_ERR_ARG, std::string(who) + ": r2_millionths must be within 1..1000000");
    if (kmer_len < 1 || kmer_len > 32) throw Error(KGWAS_ERR_ARG, std::string(who) + ": k-mers of 1 to 32 bases are supported");
    const double t_start = now_ms();
    // the leads, before the table is looked for
    const std::vector<Lead> leads = read_leads(leads_path, kmer_len, kgwas_kmer_encode);
    const uint64_t L = leads.size();
    check_proxy_shape("proxy_kmers", L, 1, tm);  // (the leads' number before the table is looked for; the accessions below)
    TableSession ts;
    if (pheno_path) ts.load_pheno(pheno_path);
    ts.open_table(table_base, kmer_len);
    ts.refuse_duplicate_accessions();
    ts.check_squeeze_fits("proxy_kmers");
    const uint64_t n = ts.S, n_rows = ts.n_rows, stride = ts.stride();
    check_proxy_shape("proxy_kmers", L, n, tm);

    kgwas_proxy_stats s{};
    s.accessions = n;
    s.leads = L;
    // the leads' rows, by the table's own search
    double t = now_ms();
    std::vector<uint64_t> codes(L);
    for (uint64_t i = 0; i < L; i++) codes[i] = leads[i].code;
    const PlacedRows placed = ts.rows_of_codes(codes, device);
    if (placed.missing != PlacedRows::NONE)
        throw Error(KGWAS_ERR_FORMAT, "the k-mer " + leads[placed.missing].text + " of " + leads_path + " is not in the table " + table_base);
    s.search_ms = now_ms() - t;

    // one pass over the table
    use_device(device);
    RowLayout lay;
    lay.stride = stride, lay.bit_off = 1, lay.W = ts.W_f, lay.kmers = true;
    lay.col = pheno_path ? ts.col.data() : nullptr;
    const uint64_t piece = piece_rows(n_rows, stride, 64ull << 20, PROXY_MAX_PIECE, PROXY_MAX_PIECE, "KGWAS_PROXY_PIECE_ROWS");
    std::vector<uint32_t> n1_leads(L, 0);
    Buckets buckets(L, max_per_lead);
    SearchTimes times;
    if (n_rows) {
        PieceReader reader(ts.t, n_rows, piece, stride);
        search(lay, placed.rows.data(), L, n, tm, n_rows, piece, n1_leads.data(), [&](uint64_t k) { return reader.wait(k); },
               [&](uint64_t k) { reader.release(k); }, [&](const kgwas_proxy_record* rec, uint64_t count) { buckets.add(rec, count); }, times);
    }
    s.rows_read = n_rows;
    s.pairs_tested = n_rows * L;
    s.proxies_found = buckets.total;
    s.drain_rounds = times.rounds;
    s.kernel_ms = times.kernel_ms;
    s.copy_ms = times.copy_ms;

    std::string text = header_line(), per_lead;
    for (uint64_t i = 0; i < L; i++) {
        for (const kgwas_proxy_record& r : buckets.kept[i]) append_line(text, leads[i].text, kmer_len, n, n1_leads[i], r);
        s.proxies_kept += buckets.kept[i].size();
        per_lead += "lead\t" + leads[i].text + "\t" + std::to_string(buckets.kept[i].size()) + "\t" + std::to_string(buckets.found[i]) + "\n";
    }
    write_text(out_path, text);
    s.total_ms = now_ms() - t_start;
    char log[4096];
    int ll = snprintf(log, sizeof(log),
                      "proxy_kmers: the k-mers of the table in LD with a lead (a proxy iff r2 >= the threshold)\nkmers_table\t%s\nkmers_len\t%u\n"
                      "phenotypes\t%s\nleads_file\t%s\nr2\t%s\nmax_per_lead\t%llu\naccessions\t%llu\nleads\t%llu\n",
                      table_base, kmer_len, pheno_path ? pheno_path : "(none: every accession of the table)", leads_path, r2_text(tm).c_str(),
                      (unsigned long long)max_per_lead, (unsigned long long)s.accessions, (unsigned long long)s.leads);
    if (ll < 0) throw Error(KGWAS_ERR_IO, std::string("can't write ") + out_path + ".log.txt");
    std::string log_text(log, std::min((size_t)ll, sizeof(log) - 1));
    log_text += per_lead;
    ll = snprintf(log, sizeof(log), "rows_read\t%llu\npairs_tested\t%llu\nproxies_found\t%llu\nproxies_kept\t%llu\ndrain_rounds\t%llu\n"
                                    "ms: search=%.3f kernels=%.3f copy=%.3f total=%.3f\n",
                  (unsigned long long)s.rows_read, (unsigned long long)s.pairs_tested, (unsigned long long)s.proxies_found,
                  (unsigned long long)s.proxies_kept, (unsigned long long)s.drain_rounds, s.search_ms, s.kernel_ms, s.copy_ms, s.total_ms);
    if (ll < 0) throw Error(KGWAS_ERR_IO, std::string("can't write ") + out_path + ".log.txt");
    log_text.append(log, std::min((size_t)ll, sizeof(log) - 1));
    write_text(std::string(out_path) + ".log.txt", log_text);
    if (st) *st = s;
}

}  // namespace

extern "C" {

int kgwas_kmers_ld_proxies(const uint64_t* lead_bits, uint64_t n_leads, const uint64_t* bits, uint64_t n_rows, uint64_t words_per_row, uint64_t n_acc,
                           uint32_t r2_millionths, int32_t device, kgwas_proxy_record* records_out, uint64_t cap, uint64_t* n_out) {
    return guarded([&] { kmers_ld_proxies(lead_bits, n_leads, bits, n_rows, words_per_row, n_acc, r2_millionths, device, records_out, cap, n_out); });
}

int kgwas_proxy_kmers_run(const char* table_base, uint32_t kmer_len, const char* pheno_path, const char* leads_path, uint32_t r2_millionths,
                          uint64_t max_per_lead, int32_t device, const char* out_path, kgwas_proxy_stats* st) {
    return guarded([&] { run(table_base, kmer_len, pheno_path, leads_path, r2_millionths, max_per_lead, device, out_path, st); });
}

}  // extern "C"
