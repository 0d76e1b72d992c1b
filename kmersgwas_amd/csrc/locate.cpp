// locate.cpp — kgwas_locate_kmers_bases and kgwas_locate_kmers_run: the genome positions of k-mers, exact or with one mismatch
// (DESIGN.md 4.15). A tool of this project's own: proxy_kmers ends with the k-mers one maps, this maps them.
//
// search   many windows against few patterns in one streaming pass. The queries' sorted pattern lists are built once (locate_host.h)
//          and stay on the device; the base stream comes in pieces of P window positions plus k - 1 bytes of overlap, so a window
//          that straddles a piece boundary belongs to the piece it starts in and is reported once. Two device buffers take turns:
//          piece j + 1 is copied on a stream of its own while piece j is counted (locate_kernels.hip: records per tile, scan) and
//          its records are written and brought back in rounds of at most the record buffer's size. What leaves the device is the
//          records alone, in (pos, kmer, strand) order, the same in every run.
// run      k-mers file -> the reference's stream from a reader thread (FASTA lines into pinned pieces) -> search -> the records
//          bucketed per k-mer with the reference's letter at the mismatch -> the output and its log.
#include <condition_variable>
#include <cstring>
#include <functional>
#include <mutex>

#include "device.h"
#include "kernels.h"
#include "locate_host.h"

using namespace kgwas;
using namespace kgwas::locate;

namespace {

static_assert(sizeof(LocateRecord) == sizeof(kgwas_locate_record) && sizeof(LocateRecord) == 16, "the device's record is the header's");
static_assert(MAX_SPLITTERS == LOCATE_SPLITTERS, "locate_host.h sizes the splitters for the kernels' LDS");

constexpr uint64_t LOCATE_RECORDS = 1ull << 20;  // records of the device buffer (KGWAS_LOCATE_RECORDS: the tests' hook)
uint32_t record_cap() {
    const long long forced = opt_int("KGWAS_LOCATE_RECORDS", 0);
    return (uint32_t)(forced > 0 ? std::min<long long>(forced, 1ll << 26) : (long long)LOCATE_RECORDS);
}
// window positions per piece (KGWAS_LOCATE_PIECE_BYTES: the tests' hook)
uint64_t piece_bytes() {
    const long long forced = opt_int("KGWAS_LOCATE_PIECE_BYTES", 0);
    return forced > 0 ? std::min<uint64_t>((uint64_t)forced, LOCATE_MAX_PIECE) : LOCATE_MAX_PIECE;
}

// Piece j: the stream's bytes [base, base + bytes), base = j P, bytes <= P + k - 1; its windows start in the first P of them.
struct Piece {
    const uint8_t* p = nullptr;  // host memory, or device memory when the stream is resident
    uint64_t bytes = 0, base = 0;
    bool last = true;
};
struct SearchTimes {
    double kernel_ms = 0, copy_ms = 0;
    uint64_t rounds = 0, windows = 0;
};

// wait(j) -> piece j, release(j): its records are consumed, the host's bytes may go. consume(records, count, piece): valid until it
// returns.
typedef std::function<Piece(uint64_t)> WaitPiece;
typedef std::function<void(uint64_t)> ReleasePiece;
typedef std::function<void(const kgwas_locate_record*, uint64_t, const Piece&)> ConsumeRecords;

struct DeviceList {
    DevBuf<uint64_t> spl, keys, codes;
    DevBuf<uint32_t> ids;
    LocateList view{};
    void upload(const List& l, bool codes_are_keys) {
        const size_t n = l.keys.size();
        view = LocateList{nullptr, nullptr, nullptr, nullptr, n, l.B, (uint32_t)l.spl.size()};
        if (!n) return;
        spl.alloc(l.spl.size()), keys.alloc(n), ids.alloc(n);
        KGWAS_HIP(hipMemcpy(spl.p, l.spl.data(), l.spl.size() * 8, hipMemcpyHostToDevice));
        KGWAS_HIP(hipMemcpy(keys.p, l.keys.data(), n * 8, hipMemcpyHostToDevice));
        KGWAS_HIP(hipMemcpy(ids.p, l.ids.data(), n * 4, hipMemcpyHostToDevice));
        if (!codes_are_keys) {
            codes.alloc(n);
            KGWAS_HIP(hipMemcpy(codes.p, l.codes.data(), n * 8, hipMemcpyHostToDevice));
        }
        view.spl = spl.p, view.keys = keys.p, view.codes = codes_are_keys ? keys.p : codes.p, view.ids = ids.p;
    }
};

void search(uint32_t k, uint32_t d, const Lists& lists, uint64_t P, bool resident, const WaitPiece& wait, const ReleasePiece& release,
            const ConsumeRecords& consume, SearchTimes& times) {
    const uint32_t cap = record_cap();
    const uint32_t max_tiles = locate_tiles(P);
    DeviceList H, L;
    DevBuf<uint8_t> d_bases[2];
    DevBuf<uint32_t> d_bcnt, d_boff;
    DevBuf<unsigned long long> d_windows;
    DevBuf<LocateRecord> d_rec;
    PinBuf<kgwas_locate_record> h_rec;
    PinBuf<uint32_t> h_boff;
    PinBuf<unsigned long long> h_windows;
    Event ev_c0[2], ev_c1[2], ev_k0, ev_k1;
    H.upload(lists.H, d == 0), L.upload(lists.L, false);
    for (int i = 0; i < 2; i++) {
        if (!resident) d_bases[i].alloc(P + k - 1);
        ev_c0[i].create(), ev_c1[i].create();
    }
    d_bcnt.alloc(max_tiles), d_boff.alloc(max_tiles + 1), h_boff.alloc(max_tiles + 1);
    d_windows.alloc(1), h_windows.alloc(1);
    KGWAS_HIP(hipMemset(d_windows.p, 0, sizeof(unsigned long long)));
    d_rec.alloc(cap), h_rec.alloc(cap);
    ev_k0.create(), ev_k1.create();
    Stream s_run, s_copy;  // (declared after the buffers their work uses: they go first, idle)
    s_run.create(hipStreamNonBlocking);
    s_copy.create(hipStreamNonBlocking);

    auto elapsed = [](hipEvent_t a, hipEvent_t b) {
        float ms = 0;
        KGWAS_HIP(hipEventElapsedTime(&ms, a, b));
        return (double)ms;
    };
    auto upload = [&](uint64_t j, const Piece& pc) {  // piece j into device buffer j & 1, which piece j - 2 has left
        if (resident) return;
        const int b = (int)(j & 1);
        if (pc.bytes > d_bases[b].n) throw Error(KGWAS_ERR_STATE, "locate: a piece larger than its buffer");
        KGWAS_HIP(hipEventRecord(ev_c0[b], s_copy));
        if (pc.bytes) KGWAS_HIP(hipMemcpyAsync(d_bases[b].p, pc.p, pc.bytes, hipMemcpyHostToDevice, s_copy));
        KGWAS_HIP(hipEventRecord(ev_c1[b], s_copy));
    };
    Piece cur = wait(0);
    upload(0, cur);
    for (uint64_t j = 0;; j++) {
        const int b = (int)(j & 1);
        const uint8_t* d_p = resident ? cur.p : d_bases[b].p;
        const uint64_t n_win = std::min(P, cur.bytes);
        const uint32_t tiles = locate_tiles(n_win);
        if (!resident) KGWAS_HIP(hipStreamWaitEvent(s_run, ev_c1[b], 0));
        KGWAS_HIP(hipEventRecord(ev_k0, s_run));
        KGWAS_HIP(launch_locate_count(d_p, cur.bytes, n_win, k, d, H.view, L.view, d_bcnt.p, d_boff.p, d_windows.p, s_run));
        KGWAS_HIP(hipEventRecord(ev_k1, s_run));
        if (tiles) KGWAS_HIP(hipMemcpyAsync(h_boff.p, d_boff.p, (tiles + 1) * 4, hipMemcpyDeviceToHost, s_run));
        Piece next;
        if (!cur.last) {  // the next piece's copy runs beside this piece's kernels
            next = wait(j + 1);
            upload(j + 1, next);
        }
        KGWAS_HIP(hipStreamSynchronize(s_run));
        times.kernel_ms += elapsed(ev_k0, ev_k1);
        if (!resident) times.copy_ms += elapsed(ev_c0[b], ev_c1[b]);
        if (tiles)
            for (const Round& r : drain_rounds(h_boff.p, tiles, cap)) {
                KGWAS_HIP(hipEventRecord(ev_k0, s_run));
                KGWAS_HIP(launch_locate_write(d_p, cur.bytes, n_win, k, d, H.view, L.view, d_boff.p, r.blk0, r.blk1, r.lo, cap, cur.base, d_rec.p, s_run));
                KGWAS_HIP(hipEventRecord(ev_k1, s_run));
                KGWAS_HIP(hipMemcpyAsync(h_rec.p, d_rec.p, (size_t)(r.hi - r.lo) * sizeof(LocateRecord), hipMemcpyDeviceToHost, s_run));
                KGWAS_HIP(hipStreamSynchronize(s_run));
                times.kernel_ms += elapsed(ev_k0, ev_k1);
                times.rounds++;
                consume(h_rec.p, r.hi - r.lo, cur);
            }
        release(j);
        if (cur.last) break;
        cur = next;
    }
    KGWAS_HIP(hipMemcpy(h_windows.p, d_windows.p, sizeof(unsigned long long), hipMemcpyDeviceToHost));
    times.windows = *h_windows.p;
}

void locate_bases(const void* bases, uint64_t n_bytes, int on_device, const uint64_t* codes, uint64_t n_kmers, uint32_t k, uint32_t d, int32_t device,
                  kgwas_locate_record* out, uint64_t cap, uint64_t* n_out) {
    const char* who = "kgwas_locate_kmers_bases";
    if (!codes || !n_out || (!bases && n_bytes) || (!out && cap)) throw Error(KGWAS_ERR_ARG, std::string(who) + ": null argument");
    const Lists lists = build_lists(who, codes, n_kmers, k, d);
    *n_out = 0;
    use_device(device);
    if (!n_bytes) return;
    const uint64_t P = std::min(piece_bytes(), n_bytes);
    const uint8_t* p = static_cast<const uint8_t*>(bases);
    uint64_t total = 0;
    SearchTimes times;
    search(k, d, lists, P, on_device != 0,
           [&](uint64_t j) {
               Piece pc;
               pc.base = j * P, pc.p = p + pc.base;
               pc.bytes = std::min(n_bytes - pc.base, P + k - 1);
               pc.last = pc.base + P >= n_bytes;
               return pc;
           },
           [](uint64_t) {},
           [&](const kgwas_locate_record* rec, uint64_t count, const Piece&) {
               if (total < cap) memcpy(out + total, rec, std::min(count, cap - total) * sizeof(kgwas_locate_record));
               total += count;
           },
           times);
    *n_out = total;
    if (opt_set("KGWAS_LOCATE_TIMING"))
        fprintf(stderr, "[kgwas] locate_kmers_bases: bytes=%llu kmers=%llu mismatches=%u windows=%llu hits=%llu kernels_ms=%.3f copy_ms=%.3f rounds=%llu\n",
                (unsigned long long)n_bytes, (unsigned long long)n_kmers, d, (unsigned long long)times.windows, (unsigned long long)total, times.kernel_ms,
                times.copy_ms, (unsigned long long)times.rounds);
}

// The reference's stream in pinned pieces, filled by a thread of its own: two blocks take turns; piece j lies in block j & 1 and
// starts with the k - 1 bytes piece j - 1 ended with.
class ReferenceFeed {
   public:
    FastaParser parser;
    double parse_ms = 0;
    // opens the file and looks at its first byte: before any device call
    ReferenceFeed(const std::string& path, uint64_t P, uint32_t k)
        : parser(path, [this](const char* p, size_t n) { put(p, n); }), path_(path), P_(P), k_(k) {
        f_ = fopen(path.c_str(), "rb");
        if (!f_) throw Error(KGWAS_ERR_IO, "can't open file: " + path);
        const int c = fgetc(f_);
        if (c != '>') {
            fclose(f_);
            throw Error(KGWAS_ERR_FORMAT, path + (c == EOF ? ": not FASTA (the file is empty)" : ": not FASTA"));
        }
        rewind(f_);
    }
    void start() {  // (pinned memory: a device is current)
        for (int i = 0; i < 2; i++) block_[i].alloc(P_ + k_ - 1);
        th_ = std::thread([this] { run(); });
    }
    Piece wait(uint64_t j) {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return published_ > j || err_; });
        if (published_ <= j) std::rethrow_exception(err_);
        return pieces_[j & 1];
    }
    void release(uint64_t j) {
        std::lock_guard<std::mutex> lk(mu_);
        released_ = j + 1;
        cv_.notify_all();
    }
    ~ReferenceFeed() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
            cv_.notify_all();
        }
        if (th_.joinable()) th_.join();
        if (f_) fclose(f_);
    }

   private:
    struct Stopped {};
    void run() {
        kgwas_name_this_thread("kgwas-fasta");
        const double t0 = now_ms();
        try {
            std::vector<char> block(4u << 20);
            for (size_t n; (n = fread(block.data(), 1, block.size(), f_)) > 0;) parser.feed(block.data(), n);
            if (ferror(f_)) throw Error(KGWAS_ERR_IO, "can't read file: " + path_);
            parser.finish();
            acquire();
            publish(true);
        } catch (const Stopped&) {
        } catch (...) {
            std::lock_guard<std::mutex> lk(mu_);
            err_ = std::current_exception();
            cv_.notify_all();
        }
        parse_ms = now_ms() - t0 - waited_ms_;
    }
    // block filling_ & 1 is this thread's once piece filling_ - 2 is released
    void acquire() {
        if (have_) return;
        const double t0 = now_ms();
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return stop_ || filling_ < released_ + 2; });
        if (stop_) throw Stopped();
        waited_ms_ += now_ms() - t0;
        have_ = true;
        fill_ = 0;
        if (filling_ && k_ > 1) memcpy(block_[filling_ & 1].p, carry_, fill_ = k_ - 1);
    }
    void put(const char* p, size_t n) {
        while (n) {
            acquire();
            uint8_t* dst = block_[filling_ & 1].p;
            const size_t m = std::min<uint64_t>(n, P_ + k_ - 1 - fill_);
            memcpy(dst + fill_, p, m);
            fill_ += m, p += m, n -= m;
            if (fill_ == P_ + k_ - 1) publish(false);
        }
    }
    void publish(bool last) {
        const uint8_t* src = block_[filling_ & 1].p;
        if (!last && k_ > 1) memcpy(carry_, src + fill_ - (k_ - 1), k_ - 1);
        Piece pc;
        pc.p = src, pc.bytes = fill_, pc.base = filling_ * P_, pc.last = last;
        std::lock_guard<std::mutex> lk(mu_);
        pieces_[filling_ & 1] = pc;
        published_ = ++filling_;
        have_ = false;
        cv_.notify_all();
    }
    std::string path_;
    uint64_t P_;
    uint32_t k_;
    FILE* f_ = nullptr;
    PinBuf<uint8_t> block_[2];
    Piece pieces_[2];
    uint8_t carry_[32];
    uint64_t filling_ = 0, fill_ = 0, published_ = 0, released_ = 0;
    double waited_ms_ = 0;
    bool have_ = false, stop_ = false;
    std::exception_ptr err_;
    std::mutex mu_;
    std::condition_variable cv_;
    std::thread th_;
};

void run(const char* reference_path, const char* kmers_path, uint32_t k, uint32_t d, uint64_t max_per_kmer, int32_t device, const char* out_path,
         kgwas_locate_stats* st) {
    const char* who = "kgwas_locate_kmers_run";
    if (!reference_path || !kmers_path || !out_path) throw Error(KGWAS_ERR_ARG, std::string(who) + ": null argument");
    check_locate_shape(who, k, d, 1);
    const double t_start = now_ms();
    // the k-mers, before the reference is looked for
    const Queries queries = read_queries(kmers_path, k);
    const uint64_t n = queries.q.size();
    std::vector<uint64_t> codes(n);
    for (uint64_t i = 0; i < n; i++) codes[i] = queries.q[i].f;
    const Lists lists = build_lists("locate_kmers", codes.data(), n, k, d);
    const uint64_t P = piece_bytes();
    ReferenceFeed feed(reference_path, P, k);
    use_device(device);
    feed.start();

    Buckets buckets(n, max_per_kmer, k);
    SearchTimes times;
    search(k, d, lists, P, false, [&](uint64_t j) { return feed.wait(j); }, [&](uint64_t j) { feed.release(j); },
           [&](const kgwas_locate_record* rec, uint64_t count, const Piece& pc) {
               buckets.add(rec, count, [&](uint64_t pos) {
                   if (pos < pc.base || pos - pc.base >= pc.bytes) throw Error(KGWAS_ERR_STATE, "locate: a hit outside its piece");
                   return pc.p[pos - pc.base];
               });
           },
           times);

    kgwas_locate_stats s{};
    s.contigs = feed.parser.contigs.size();
    s.bases = feed.parser.sequence_bytes();
    s.windows_tested = times.windows;
    s.kmers = n;
    s.hits_found = buckets.total;
    s.drain_rounds = times.rounds;
    s.kernel_ms = times.kernel_ms, s.copy_ms = times.copy_ms, s.parse_ms = feed.parse_ms;
    std::string text = header_line(queries.has_p), per_kmer;
    for (uint64_t i = 0; i < n; i++) {
        for (const Hit& h : buckets.kept[i]) append_line(text, queries.q[i], feed.parser.contigs, h, queries.has_p);
        s.hits_kept += buckets.kept[i].size();
        s.kmers_without_hit += buckets.found[i] == 0, s.kmers_with_one_hit += buckets.found[i] == 1;
        per_kmer += "kmer\t" + queries.q[i].text + "\t" + std::to_string(buckets.kept[i].size()) + "\t" + std::to_string(buckets.found[i]) + "\n";
    }
    write_text(out_path, text);
    s.total_ms = now_ms() - t_start;
    char log[4096];
    int ll = snprintf(log, sizeof(log),
                      "locate_kmers: the windows of the reference that spell a k-mer or its reverse complement\nreference\t%s\nkmers_file\t%s\n"
                      "kmers_len\t%u\nmismatches\t%u\nmax_per_kmer\t%llu\n",
                      reference_path, kmers_path, k, d, (unsigned long long)max_per_kmer);
    if (ll < 0) throw Error(KGWAS_ERR_IO, std::string("can't write ") + out_path + ".log.txt");
    std::string log_text(log, std::min((size_t)ll, sizeof(log) - 1));
    log_text += per_kmer;
    ll = snprintf(log, sizeof(log),
                  "contigs\t%llu\nbases\t%llu\nwindows_tested\t%llu\nkmers\t%llu\nhits_found\t%llu\nhits_kept\t%llu\nkmers_without_hit\t%llu\n"
                  "kmers_with_one_hit\t%llu\ndrain_rounds\t%llu\nms: parse=%.3f copy=%.3f kernels=%.3f total=%.3f\n",
                  (unsigned long long)s.contigs, (unsigned long long)s.bases, (unsigned long long)s.windows_tested, (unsigned long long)s.kmers,
                  (unsigned long long)s.hits_found, (unsigned long long)s.hits_kept, (unsigned long long)s.kmers_without_hit,
                  (unsigned long long)s.kmers_with_one_hit, (unsigned long long)s.drain_rounds, s.parse_ms, s.copy_ms, s.kernel_ms, s.total_ms);
    if (ll < 0) throw Error(KGWAS_ERR_IO, std::string("can't write ") + out_path + ".log.txt");
    log_text.append(log, std::min((size_t)ll, sizeof(log) - 1));
    write_text(std::string(out_path) + ".log.txt", log_text);
    if (st) *st = s;
}

}  // namespace

extern "C" {

int kgwas_locate_kmers_bases(const void* bases, uint64_t n_bytes, int on_device, const uint64_t* codes, uint64_t n_kmers, uint32_t kmer_len,
                             uint32_t mismatches, int32_t device, kgwas_locate_record* records_out, uint64_t cap, uint64_t* n_out) {
    return guarded([&] { locate_bases(bases, n_bytes, on_device, codes, n_kmers, kmer_len, mismatches, device, records_out, cap, n_out); });
}

int kgwas_locate_kmers_run(const char* reference_path, const char* kmers_path, uint32_t kmer_len, uint32_t mismatches, uint64_t max_per_kmer,
                           int32_t device, const char* out_path, kgwas_locate_stats* st) {
    return guarded([&] { run(reference_path, kmers_path, kmer_len, mismatches, max_per_kmer, device, out_path, st); });
}

}  // extern "C"
