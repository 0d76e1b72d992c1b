// proxy.cpp — kgwas_kmers_ld_proxies and kgwas_proxy_kmers_run: every k-mer of the table in LD with a lead k-mer.
// A tool of this project's own: clump_kmers ends with one lead per signal, this finds the k-mers that travel with each lead.
//
// search   few leads against many rows in one streaming pass. The leads' operands are prepared once and stay on the device; the rows
//          come in pieces through two device buffers that take turns: piece k + 1 is copied on a stream of its own while piece k is
//          squeezed, prepared, linked (ld_rect_kernel: one bit per pair) and compacted into records, which come back in rounds of at
//          most the record buffer's size. What leaves the device is the records alone, in (row, lead) order, the same in every run.
// run      leads file -> their rows from the table (kgwas_filter_kmers' search) -> search over the whole table (PieceReader) ->
//          the records bucketed per lead (proxy_host.h) -> the output and its log.
#include <chrono>
#include <cstring>
#include <functional>

#include "device.h"
#include "kernels.h"
#include "piece_reader.h"
#include "proxy_host.h"

using namespace kgwas;
using namespace kgwas::proxy;

namespace {

static_assert(sizeof(ProxyRecord) == sizeof(kgwas_proxy_record) && sizeof(ProxyRecord) == 32, "the device's record is the header's");

constexpr uint64_t PROXY_MAX_PIECE = 1ull << 18, PROXY_RECORDS = 1ull << 20;

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// rows per piece for rows of `stride` words: about 64 MiB of rows, at most 2^18 (KGWAS_PROXY_PIECE_ROWS: the tests' hook)
uint64_t piece_rows(uint64_t n_rows, uint64_t stride) {
    uint64_t piece = std::max<uint64_t>(1024, std::min<uint64_t>(PROXY_MAX_PIECE, (64ull << 20) / (8 * stride)));
    const long long forced = opt_int("KGWAS_PROXY_PIECE_ROWS", 0);
    if (forced > 0) piece = (uint64_t)std::min<long long>(forced, (long long)PROXY_MAX_PIECE);
    return std::min(piece, std::max<uint64_t>(n_rows, 1));
}
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
    const uint32_t n_chunks = (uint32_t)((n + 511) / 512 * 4), W_m = (uint32_t)(2 * ((n + 127) / 128));
    const uint64_t n_pieces = (n_rows + piece - 1) / piece;

    DevBuf<uint64_t> d_leads, d_rows[2], d_tqA, d_tqB, d_bits;
    DevBuf<uint32_t> d_colmap, d_sqA, d_sqB, d_n1A, d_pqA, d_n1B, d_pqB, d_bcnt, d_boff;
    DevBuf<uint4> d_PA, d_PB;
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
    d_PA.alloc((size_t)n_chunks * L_pad), d_n1A.alloc(L_pad), d_pqA.alloc(L_pad), d_tqA.alloc(L_pad);
    d_PB.alloc((size_t)n_chunks * P_pad), d_n1B.alloc(P_pad), d_pqB.alloc(P_pad), d_tqB.alloc(P_pad);
    d_bits.alloc(P_pad * pitch_q);
    d_bcnt.alloc(max_blocks), d_boff.alloc(max_blocks + 1), h_boff.alloc(max_blocks + 1);
    d_rec.alloc(cap), h_rec.alloc(cap);
    ev_k0.create(), ev_k1.create();
    if (lay.col) {
        std::vector<uint32_t> colmap(64ull * W_m, 0xFFFFFFFFu);
        for (uint64_t i = 0; i < n; i++) colmap[i] = (uint32_t)lay.col[i];
        d_colmap.alloc(colmap.size());
        KGWAS_HIP(hipMemcpy(d_colmap.p, colmap.data(), colmap.size() * 4, hipMemcpyHostToDevice));
        d_sqA.alloc(L * 2 * W_m), d_sqB.alloc(piece * 2 * W_m);
    }
    Stream s_run, s_copy;  // (declared after the buffers their work uses: they go first, idle)
    s_run.create(hipStreamNonBlocking);
    s_copy.create(hipStreamNonBlocking);

    // the operands of `count` rows at d (the layout's) -> P, n1, pq, tq with `pad` rows, on s_run
    auto prepare = [&](const uint64_t* d, uint64_t count, uint64_t pad, uint32_t* sq, uint4* P, uint32_t* n1, uint32_t* pq, uint64_t* tq) {
        const uint64_t* bits = d + lay.bit_off;
        uint64_t stride = lay.stride, W = lay.W;
        if (lay.col) {
            KGWAS_HIP(launch_squeeze(d, lay.stride, count, d_colmap.p, W_m, (uint32_t)lay.W, sq, s_run));
            bits = reinterpret_cast<const uint64_t*>(sq);
            stride = W = W_m;
        }
        KGWAS_HIP(launch_ld_prep(bits, stride, W, count, (uint32_t)n, n_chunks, pad, tm, P, n1, pq, tq, s_run));
    };
    auto elapsed = [](hipEvent_t a, hipEvent_t b) {
        float ms = 0;
        KGWAS_HIP(hipEventElapsedTime(&ms, a, b));
        return (double)ms;
    };

    // the leads, once
    KGWAS_HIP(hipMemcpyAsync(d_leads.p, lead_rows, L * lay.stride * 8, hipMemcpyHostToDevice, s_run));
    KGWAS_HIP(hipEventRecord(ev_k0, s_run));
    prepare(d_leads.p, L, L_pad, d_sqA.p, d_PA.p, d_n1A.p, d_pqA.p, d_tqA.p);
    KGWAS_HIP(hipEventRecord(ev_k1, s_run));
    if (n1_leads) KGWAS_HIP(hipMemcpyAsync(n1_leads, d_n1A.p, L * 4, hipMemcpyDeviceToHost, s_run));
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
        const uint64_t R = rows_of(k), R_pad = (R + 127) / 128 * 128;
        const uint32_t n_blocks = (uint32_t)((R + 255) / 256);
        KGWAS_HIP(hipStreamWaitEvent(s_run, ev_c1[b], 0));
        KGWAS_HIP(hipEventRecord(ev_k0, s_run));
        prepare(d_rows[b].p, R, R_pad, d_sqB.p, d_PB.p, d_n1B.p, d_pqB.p, d_tqB.p);
        KGWAS_HIP(launch_ld_rect(d_PA.p, d_n1A.p, d_pqA.p, L, L_pad, d_PB.p, d_n1B.p, d_tqB.p, R, R_pad, (uint32_t)n, n_chunks, d_bits.p, pitch_q, popcount,
                                 s_run));
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
            KGWAS_HIP(launch_ld_proxy_write(d_bits.p, pitch_q, R, d_boff.p, r.blk0, r.blk1, r.lo, cap, d_PA.p, L_pad, d_PB.p, R_pad, n_chunks, d_n1B.p,
                                            lay.kmers ? d_rows[b].p : nullptr, lay.stride, k * piece, d_rec.p, s_run));
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
    const uint64_t piece = piece_rows(n_rows, W);
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
    std::vector<uint64_t> col;
    if (pheno_path) {
        col.resize(S);
        std::vector<uint64_t> mask(W_f, 0);
        ck(kgwas_table_column_map(own.t, acc.data(), S, col.data()));
        for (uint64_t i = 0; i < S; i++) {
            if (mask[col[i] / 64] >> (col[i] % 64) & 1) throw Error(KGWAS_ERR_FORMAT, std::string(pheno_path) + " lists the accession " + acc[i] + " twice");
            mask[col[i] / 64] |= 1ull << (col[i] % 64);
        }
        check_squeeze_fits("proxy_kmers", S_f, S);
    } else {
        S = S_f;
    }
    const uint64_t n = S, stride = 1 + W_f;
    check_proxy_shape("proxy_kmers", L, n, tm);

    kgwas_proxy_stats s{};
    s.accessions = n;
    s.leads = L;
    // the leads' rows, by the table's own search
    double t = now_ms();
    std::vector<uint64_t> codes(L), found(L * stride), lead_rows(L * stride);
    for (uint64_t i = 0; i < L; i++) codes[i] = leads[i].code;
    uint64_t n_found = 0;
    ck(kgwas_filter_kmers(own.t, codes.data(), L, device, nullptr, found.data(), &n_found));
    std::unordered_map<uint64_t, uint64_t> at;  // code -> place among the leads
    for (uint64_t i = 0; i < L; i++) at.emplace(codes[i], i);
    std::vector<uint8_t> have(L, 0);
    for (uint64_t i = 0; i < n_found; i++) {
        const auto it = at.find(found[i * stride]);
        if (it == at.end() || have[it->second]) continue;  // (a key the table holds twice: its first row)
        have[it->second] = 1;
        memcpy(&lead_rows[it->second * stride], &found[i * stride], stride * 8);
    }
    for (uint64_t i = 0; i < L; i++)
        if (!have[i]) throw Error(KGWAS_ERR_FORMAT, "the k-mer " + leads[i].text + " of " + leads_path + " is not in the table " + table_base);
    s.search_ms = now_ms() - t;

    // one pass over the table
    use_device(device);
    RowLayout lay;
    lay.stride = stride, lay.bit_off = 1, lay.W = W_f, lay.kmers = true;
    lay.col = pheno_path ? col.data() : nullptr;
    const uint64_t piece = piece_rows(n_rows, stride);
    std::vector<uint32_t> n1_leads(L, 0);
    Buckets buckets(L, max_per_lead);
    SearchTimes times;
    if (n_rows) {
        PieceReader reader(own.t, n_rows, piece, stride);
        search(lay, lead_rows.data(), L, n, tm, n_rows, piece, n1_leads.data(), [&](uint64_t k) { return reader.wait(k); },
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
    auto write_text = [](const std::string& path, const std::string& body) {
        FILE* fo = fopen(path.c_str(), "wb");
        const bool ok = fo && fwrite(body.data(), 1, body.size(), fo) == body.size();
        if ((fo && fclose(fo) != 0) || !ok) throw Error(KGWAS_ERR_IO, "can't write " + path);
    };
    write_text(out_path, text);
    s.total_ms = now_ms() - t_start;
    char r2_text[16], log[4096];
    snprintf(r2_text, sizeof(r2_text), "%u.%06u", tm / 1000000u, tm % 1000000u);
    int ll = snprintf(log, sizeof(log),
                      "proxy_kmers: the k-mers of the table in LD with a lead (a proxy iff r2 >= the threshold)\nkmers_table\t%s\nkmers_len\t%u\n"
                      "phenotypes\t%s\nleads_file\t%s\nr2\t%s\nmax_per_lead\t%llu\naccessions\t%llu\nleads\t%llu\n",
                      table_base, kmer_len, pheno_path ? pheno_path : "(none: every accession of the table)", leads_path, r2_text,
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
