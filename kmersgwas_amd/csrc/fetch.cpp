// fetch.cpp — kgwas_fetch_reads_bases and kgwas_fetch_reads_run: the reads of an accession that contain listed k-mers (DESIGN.md
// 4.16). A tool of this project's own: proxy_kmers ends with the k-mers one assembles or maps; locate_kmers maps them, this pulls
// the reads to assemble.
//
// search   many windows against few k-mers in one streaming pass, reduced per read on the device. The queries' sorted list of
//          canonical codes is built once (fetch_host.h) and stays on the device. The read stream comes in pieces of at most P bytes
//          that end behind a newline, which the host finds. Two device buffers take turns: piece j + 1 is copied on a stream of its
//          own while piece j is marked and its reads are reduced (fetch_kernels.hip), and the kept reads' records are written and
//          brought back in rounds of at most the record buffer's size. What leaves the device is the records alone, in read order,
//          the same in every run, and at the end the k-mers' window counts.
// run      k-mers file -> the reads' stream from a reader thread (records into pinned pieces, their bytes kept beside) -> search
//          -> the kept reads' bytes as the input has them, the table of kept reads and the log.
#include <condition_variable>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>

#include "device.h"
#include "fetch_host.h"
#include "kernels.h"

using namespace kgwas;
using namespace kgwas::fetch;

namespace {

static_assert(sizeof(FetchRecord) == sizeof(kgwas_fetch_record) && sizeof(FetchRecord) == 24, "the device's record is the header's");
static_assert(locate::MAX_SPLITTERS == LOCATE_SPLITTERS, "locate_host.h sizes the splitters for the kernels' LDS");

constexpr uint64_t FETCH_RECORDS = 1ull << 20;  // records of the device buffer (KGWAS_FETCH_RECORDS: the tests' hook)
constexpr int FETCH_PREFILTER = 1;              // the presence bitmap ahead of the search: on, by measurement (KGWAS_FETCH_PREFILTER: the tests' hook)
uint32_t record_cap() {
    const long long forced = opt_int("KGWAS_FETCH_RECORDS", 0);
    return (uint32_t)(forced > 0 ? std::min<long long>(forced, 1ll << 26) : (long long)FETCH_RECORDS);
}
// bytes per piece (KGWAS_FETCH_PIECE_BYTES: the tests' hook)
uint64_t piece_bytes() {
    const long long forced = opt_int("KGWAS_FETCH_PIECE_BYTES", 0);
    return forced > 0 ? std::min<uint64_t>((uint64_t)forced, LOCATE_MAX_PIECE) : LOCATE_MAX_PIECE;
}

// Piece j: `bytes` bytes of pinned host memory, whole reads that each end with '\n'; `reads` of them, the first is read `read0`.
struct Piece {
    const uint8_t* p = nullptr;
    uint64_t bytes = 0, reads = 0, read0 = 0;
    bool last = true;
};
struct SearchTimes {
    double kernel_ms = 0, copy_ms = 0;
    uint64_t rounds = 0, windows = 0;
};

// wait(j) -> piece j, release(j): its records are consumed, the host's bytes may go. consume(records, count): valid until it returns.
typedef std::function<Piece(uint64_t)> WaitPiece;
typedef std::function<void(uint64_t)> ReleasePiece;
typedef std::function<void(const kgwas_fetch_record*, uint64_t)> ConsumeRecords;

void search(uint32_t k, uint32_t min_hits, const List& list, uint64_t n_kmers, uint64_t P, const WaitPiece& wait, const ReleasePiece& release,
            const ConsumeRecords& consume, uint64_t* kmer_windows, SearchTimes& times) {
    const uint32_t cap = record_cap();
    const uint32_t max_tiles = locate_tiles(P), max_blocks = fetch_read_blocks((uint32_t)P);
    const bool prefilter = opt_int("KGWAS_FETCH_PREFILTER", FETCH_PREFILTER) != 0;
    const size_t n = list.keys.size();
    DevBuf<uint64_t> d_spl, d_keys;
    DevBuf<uint32_t> d_ids, d_filter, d_nlcnt, d_nloff, d_starts, d_bcnt, d_boff;
    DevBuf<uint16_t> d_marks;
    DevBuf<uint8_t> d_bases[2];
    DevBuf<unsigned long long> d_counts;  // [n_kmers] the k-mers' hit windows, then the windows of k bases
    DevBuf<FetchRecord> d_rec;
    PinBuf<kgwas_fetch_record> h_rec;
    PinBuf<uint32_t> h_boff, h_reads;
    PinBuf<unsigned long long> h_counts;
    Event ev_c0[2], ev_c1[2], ev_k0, ev_k1;
    d_spl.alloc(list.spl.size()), d_keys.alloc(n), d_ids.alloc(n);
    KGWAS_HIP(hipMemcpy(d_spl.p, list.spl.data(), list.spl.size() * 8, hipMemcpyHostToDevice));
    KGWAS_HIP(hipMemcpy(d_keys.p, list.keys.data(), n * 8, hipMemcpyHostToDevice));
    KGWAS_HIP(hipMemcpy(d_ids.p, list.ids.data(), n * 4, hipMemcpyHostToDevice));
    const LocateList Q{d_spl.p, d_keys.p, d_keys.p, d_ids.p, n, list.B, (uint32_t)list.spl.size()};
    for (int i = 0; i < 2; i++) {
        d_bases[i].alloc(P);
        ev_c0[i].create(), ev_c1[i].create();
    }
    d_marks.alloc((size_t)max_tiles * 256  /* a 16-bit word per lane of a tile */);
    d_nlcnt.alloc(max_tiles), d_nloff.alloc(max_tiles + 1), d_starts.alloc(P + 1);
    d_bcnt.alloc(max_blocks), d_boff.alloc(max_blocks + 1), h_boff.alloc(max_blocks + 1), h_reads.alloc(1);
    d_counts.alloc(n_kmers + 1), h_counts.alloc(n_kmers + 1);
    KGWAS_HIP(hipMemset(d_counts.p, 0, (n_kmers + 1) * sizeof(unsigned long long)));
    d_rec.alloc(cap), h_rec.alloc(cap);
    ev_k0.create(), ev_k1.create();
    Stream s_run, s_copy;  // (declared after the buffers their work uses: they go first, idle)
    s_run.create(hipStreamNonBlocking);
    s_copy.create(hipStreamNonBlocking);
    if (prefilter) {
        d_filter.alloc(FETCH_FILTER_WORDS);
        KGWAS_HIP(launch_fetch_filter(Q, d_filter.p, s_run));
    }

    auto elapsed = [](hipEvent_t a, hipEvent_t b) {
        float ms = 0;
        KGWAS_HIP(hipEventElapsedTime(&ms, a, b));
        return (double)ms;
    };
    auto upload = [&](uint64_t j, const Piece& pc) {  // piece j into device buffer j & 1, which piece j - 2 has left
        const int b = (int)(j & 1);
        if (pc.bytes > d_bases[b].n || pc.reads > pc.bytes) throw Error(KGWAS_ERR_STATE, "fetch: a piece larger than its buffer");
        KGWAS_HIP(hipEventRecord(ev_c0[b], s_copy));
        if (pc.bytes) KGWAS_HIP(hipMemcpyAsync(d_bases[b].p, pc.p, pc.bytes, hipMemcpyHostToDevice, s_copy));
        KGWAS_HIP(hipEventRecord(ev_c1[b], s_copy));
    };
    Piece cur = wait(0);
    upload(0, cur);
    for (uint64_t j = 0;; j++) {
        const int b = (int)(j & 1);
        const uint8_t* d_p = d_bases[b].p;
        const uint32_t tiles = locate_tiles(cur.bytes), n_reads = (uint32_t)cur.reads, blocks = fetch_read_blocks(n_reads);
        KGWAS_HIP(hipStreamWaitEvent(s_run, ev_c1[b], 0));
        if (tiles) {
            KGWAS_HIP(hipEventRecord(ev_k0, s_run));
            KGWAS_HIP(launch_fetch_mark(d_p, cur.bytes, k, Q, prefilter ? d_filter.p : nullptr, d_marks.p, d_nlcnt.p, d_nloff.p, d_counts.p, d_counts.p + n_kmers,
                                        s_run));
            KGWAS_HIP(launch_fetch_count(d_p, cur.bytes, k, min_hits, d_marks.p, d_nloff.p, n_reads, d_starts.p, d_bcnt.p, d_boff.p, s_run));
            KGWAS_HIP(hipEventRecord(ev_k1, s_run));
            KGWAS_HIP(hipMemcpyAsync(h_boff.p, d_boff.p, (blocks + 1) * 4, hipMemcpyDeviceToHost, s_run));
            KGWAS_HIP(hipMemcpyAsync(h_reads.p, d_nloff.p + tiles, 4, hipMemcpyDeviceToHost, s_run));
        }
        Piece next;
        if (!cur.last) {  // the next piece's copy runs beside this piece's kernels
            next = wait(j + 1);
            upload(j + 1, next);
        }
        KGWAS_HIP(hipStreamSynchronize(s_run));
        times.copy_ms += elapsed(ev_c0[b], ev_c1[b]);
        if (tiles) {
            times.kernel_ms += elapsed(ev_k0, ev_k1);
            if (*h_reads.p != n_reads) throw Error(KGWAS_ERR_STATE, "fetch: the device counts other newlines in a piece than the host");
            for (const Round& r : drain_rounds(h_boff.p, blocks, cap)) {
                KGWAS_HIP(hipEventRecord(ev_k0, s_run));
                KGWAS_HIP(launch_fetch_write(d_p, cur.bytes, k, min_hits, Q, d_marks.p, d_starts.p, n_reads, d_boff.p, r.blk0, r.blk1, r.lo, cap, cur.read0,
                                             d_rec.p, s_run));
                KGWAS_HIP(hipEventRecord(ev_k1, s_run));
                KGWAS_HIP(hipMemcpyAsync(h_rec.p, d_rec.p, (size_t)(r.hi - r.lo) * sizeof(FetchRecord), hipMemcpyDeviceToHost, s_run));
                KGWAS_HIP(hipStreamSynchronize(s_run));
                times.kernel_ms += elapsed(ev_k0, ev_k1);
                times.rounds++;
                consume(h_rec.p, r.hi - r.lo);
            }
        }
        release(j);
        if (cur.last) break;
        cur = next;
    }
    KGWAS_HIP(hipMemcpy(h_counts.p, d_counts.p, (n_kmers + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    times.windows = h_counts.p[n_kmers];
    if (kmer_windows)
        for (uint64_t i = 0; i < n_kmers; i++) kmer_windows[i] = h_counts.p[i];
}

void fetch_bases(const void* bases, uint64_t n_bytes, const uint64_t* codes, uint64_t n_kmers, uint32_t k, uint32_t min_hits, int32_t device,
                 kgwas_fetch_record* out, uint64_t cap, uint64_t* n_out, uint64_t* kmer_windows) {
    const char* who = "kgwas_fetch_reads_bases";
    if (!codes || !n_out || (!bases && n_bytes) || (!out && cap)) throw Error(KGWAS_ERR_ARG, std::string(who) + ": null argument");
    const List list = build_list(who, codes, n_kmers, k, min_hits);
    *n_out = 0;
    use_device(device);
    if (kmer_windows) std::fill(kmer_windows, kmer_windows + n_kmers, 0);
    if (!n_bytes) return;
    const uint64_t P = std::min(piece_bytes(), n_bytes + 1);
    const uint8_t* p = static_cast<const uint8_t*>(bases);
    PinBuf<uint8_t> block[2];  // the pieces' pinned copies
    for (int i = 0; i < 2; i++) block[i].alloc(P);
    uint64_t total = 0, at = 0, read0 = 0;
    SearchTimes times;
    search(k, min_hits, list, n_kmers, P,
           [&](uint64_t j) {
               const Cut c = cut_piece(who, p + at, n_bytes - at, P);
               uint8_t* dst = block[j & 1].p;
               memcpy(dst, p + at, c.take);
               if (c.add_newline) dst[c.take] = '\n';
               Piece pc;
               pc.p = dst, pc.bytes = c.bytes, pc.reads = c.reads, pc.read0 = read0, pc.last = c.last;
               at += c.take, read0 += c.reads;
               return pc;
           },
           [](uint64_t) {},
           [&](const kgwas_fetch_record* rec, uint64_t count) {
               if (total < cap) memcpy(out + total, rec, std::min(count, cap - total) * sizeof(kgwas_fetch_record));
               total += count;
           },
           kmer_windows, times);
    *n_out = total;
    if (opt_set("KGWAS_FETCH_TIMING"))
        fprintf(stderr, "[kgwas] fetch_reads_bases: bytes=%llu kmers=%llu min_hits=%u windows=%llu reads_kept=%llu kernels_ms=%.3f copy_ms=%.3f rounds=%llu\n",
                (unsigned long long)n_bytes, (unsigned long long)n_kmers, min_hits, (unsigned long long)times.windows, (unsigned long long)total, times.kernel_ms,
                times.copy_ms, (unsigned long long)times.rounds);
}

// The reads' stream in pinned pieces, filled by a thread of its own: two blocks take turns; piece j lies in block j & 1 with the
// bytes of its records (PieceMeta) beside it. A unit - a read, or with mates a pair - lies in one piece.
class ReadsFeed {
   public:
    double parse_ms = 0;
    uint64_t reads = 0, bases = 0;
    // opens the files and looks at their first bytes: before any device call
    ReadsFeed(const char* reads_path, const char* mates_path, uint64_t P) : P_(P), files_(mates_path ? 2 : 1) {
        open_source(src_[0], reads_path);
        if (mates_path) {
            open_source(src_[1], mates_path);
            if (src_[0].fmt && src_[1].fmt && src_[0].fmt != src_[1].fmt)
                throw Error(KGWAS_ERR_FORMAT, src_[1].path + ": the mates are " + (src_[1].fmt == '>' ? "FASTA" : "FASTQ") + ", the reads are not");
        }
    }
    char fmt() const { return src_[0].fmt ? src_[0].fmt : src_[1].fmt; }
    void start() {  // (pinned memory: a device is current)
        for (int i = 0; i < 2; i++) block_[i].alloc(P_);
        th_ = std::thread([this] { run(); });
    }
    Piece wait(uint64_t j) {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return published_ > j || err_; });
        if (published_ <= j) std::rethrow_exception(err_);
        return pieces_[j & 1];
    }
    const PieceMeta& meta(uint64_t j) const { return meta_[j & 1]; }
    void release(uint64_t j) {
        std::lock_guard<std::mutex> lk(mu_);
        released_ = j + 1;
        cv_.notify_all();
    }
    ~ReadsFeed() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
            cv_.notify_all();
        }
        if (th_.joinable()) th_.join();
    }

   private:
    struct Stopped {};
    void run() {
        kgwas_name_this_thread("kgwas-reads");
        const double t0 = now_ms();
        try {
            std::unique_ptr<RecordReader> rd[2];
            for (uint32_t f = 0; f < files_; f++) {
                const Source* s = &src_[f];
                rd[f].reset(new RecordReader(s->path, s->fmt, [s](char* dst, size_t n) { return read_some(s->fd.fd, dst, n, s->path); }));
            }
            Record rec[2];
            for (;;) {
                bool has[2] = {false, false};
                for (uint32_t f = 0; f < files_; f++) has[f] = rd[f]->next(rec[f]);
                if (files_ == 2 && has[0] != has[1]) {
                    const int more = has[0] ? 0 : 1;
                    throw Error(KGWAS_ERR_FORMAT, src_[more].path + " has more records than " + src_[1 - more].path + " (" + std::to_string(reads / 2) + ")");
                }
                if (!has[0]) break;
                uint64_t need = 0;
                for (uint32_t f = 0; f < files_; f++) need += rec[f].seq_len + 1;
                if (need > P_)
                    throw Error(KGWAS_ERR_ARG, "fetch_reads: a read of " + std::to_string(rec[0].seq_len) + " bytes" +
                                                   (files_ == 2 ? " and its mate of " + std::to_string(rec[1].seq_len) : std::string()) + " do not fit a piece of " +
                                                   std::to_string(P_) + " bytes");
                if (have_ && fill_ + need > P_) publish(false);
                acquire();
                uint8_t* dst = block_[filling_ & 1].p;
                for (uint32_t f = 0; f < files_; f++) {
                    memcpy(dst + fill_, rec[f].seq, rec[f].seq_len);
                    dst[fill_ + rec[f].seq_len] = '\n';
                    fill_ += rec[f].seq_len + 1, bases += rec[f].seq_len;
                    meta_[filling_ & 1].add((int)f, rec[f]);
                }
                in_piece_ += files_, reads += files_;
            }
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
        fill_ = 0, in_piece_ = 0;
        meta_[filling_ & 1].clear(reads, files_);
    }
    void publish(bool last) {
        Piece pc;
        pc.p = block_[filling_ & 1].p, pc.bytes = fill_, pc.reads = in_piece_, pc.read0 = reads - in_piece_, pc.last = last;
        std::lock_guard<std::mutex> lk(mu_);
        pieces_[filling_ & 1] = pc;
        published_ = ++filling_;
        have_ = false;
        cv_.notify_all();
    }
    uint64_t P_;
    uint32_t files_;
    Source src_[2];
    PinBuf<uint8_t> block_[2];
    PieceMeta meta_[2];
    Piece pieces_[2];
    uint64_t filling_ = 0, fill_ = 0, in_piece_ = 0, published_ = 0, released_ = 0;
    double waited_ms_ = 0;
    bool have_ = false, stop_ = false;
    std::exception_ptr err_;
    std::mutex mu_;
    std::condition_variable cv_;
    std::thread th_;
};

void run(const char* reads_path, const char* mates_path, const char* kmers_path, uint32_t k, uint32_t min_hits, uint64_t max_reads_per_kmer, int32_t device,
         const char* out_prefix, kgwas_fetch_stats* st) {
    const char* who = "kgwas_fetch_reads_run";
    if (!reads_path || !kmers_path || !out_prefix) throw Error(KGWAS_ERR_ARG, std::string(who) + ": null argument");
    check_fetch_shape(who, k, min_hits, 1);
    const double t_start = now_ms();
    // the k-mers, before the reads are looked for
    const Queries queries = locate::read_queries(kmers_path, k);
    const uint64_t n = queries.q.size();
    std::vector<uint64_t> codes(n);
    for (uint64_t i = 0; i < n; i++) codes[i] = queries.q[i].f;
    const List list = build_list("fetch_reads", codes.data(), n, k, min_hits);
    const uint64_t P = piece_bytes();
    ReadsFeed feed(reads_path, mates_path, P);
    use_device(device);
    Outputs outputs(out_prefix, feed.fmt(), mates_path != nullptr, queries, max_reads_per_kmer);
    feed.start();

    std::vector<kgwas_fetch_record> piece_records;  // a piece's records, over its rounds
    std::vector<uint64_t> kmer_windows(n, 0);
    SearchTimes times;
    search(k, min_hits, list, n, P, [&](uint64_t j) { return feed.wait(j); },
           [&](uint64_t j) {
               outputs.add(feed.meta(j), piece_records.data(), piece_records.size());
               piece_records.clear();
               feed.release(j);
           },
           [&](const kgwas_fetch_record* rec, uint64_t count) { piece_records.insert(piece_records.end(), rec, rec + count); }, kmer_windows.data(), times);

    kgwas_fetch_stats s{};
    s.reads = feed.reads, s.bases = feed.bases;
    s.windows_tested = times.windows;
    s.kmers = n;
    s.reads_kept = outputs.reads_kept, s.reads_written = outputs.reads_written, s.pairs_written = outputs.pairs_written;
    s.drain_rounds = times.rounds;
    s.kernel_ms = times.kernel_ms, s.copy_ms = times.copy_ms, s.parse_ms = feed.parse_ms;
    std::string per_kmer;
    for (uint64_t i = 0; i < n; i++) {
        s.windows_hit += kmer_windows[i], s.kmers_without_read += outputs.written[i] == 0;
        per_kmer += "kmer\t" + queries.q[i].text + "\t" + std::to_string(outputs.written[i]) + "\t" + std::to_string(kmer_windows[i]) + "\n";
    }
    s.total_ms = now_ms() - t_start;
    std::string log_text = std::string("fetch_reads: the reads that hold a window spelling a k-mer or its reverse complement\nreads_file\t") + reads_path + "\nmates_file\t" +
                           (mates_path ? mates_path : "-") + "\nkmers_file\t" + kmers_path + "\nkmers_len\t" + std::to_string(k) + "\nmin_hits\t" +
                           std::to_string(min_hits) + "\nmax_reads_per_kmer\t" + std::to_string(max_reads_per_kmer) + "\n" + per_kmer;
    char log[2048];
    const int ll = snprintf(log, sizeof(log),
                            "reads\t%llu\nbases\t%llu\nwindows_tested\t%llu\nkmers\t%llu\nwindows_hit\t%llu\nreads_kept\t%llu\nreads_written\t%llu\n"
                            "pairs_written\t%llu\nkmers_without_read\t%llu\ndrain_rounds\t%llu\nms: parse=%.3f copy=%.3f kernels=%.3f total=%.3f\n",
                            (unsigned long long)s.reads, (unsigned long long)s.bases, (unsigned long long)s.windows_tested, (unsigned long long)s.kmers,
                            (unsigned long long)s.windows_hit, (unsigned long long)s.reads_kept, (unsigned long long)s.reads_written,
                            (unsigned long long)s.pairs_written, (unsigned long long)s.kmers_without_read, (unsigned long long)s.drain_rounds, s.parse_ms,
                            s.copy_ms, s.kernel_ms, s.total_ms);
    if (ll < 0) throw Error(KGWAS_ERR_IO, std::string("can't write ") + out_prefix + ".log.txt");
    log_text.append(log, std::min((size_t)ll, sizeof(log) - 1));
    outputs.commit(log_text);
    if (st) *st = s;
}

}  // namespace

extern "C" {

int kgwas_fetch_reads_bases(const void* bases, uint64_t n_bytes, const uint64_t* codes, uint64_t n_kmers, uint32_t kmer_len, uint32_t min_hits,
                            int32_t device, kgwas_fetch_record* records_out, uint64_t cap, uint64_t* n_out, uint64_t* kmer_windows_out) {
    return guarded([&] { fetch_bases(bases, n_bytes, codes, n_kmers, kmer_len, min_hits, device, records_out, cap, n_out, kmer_windows_out); });
}

int kgwas_fetch_reads_run(const char* reads_path, const char* mates_path, const char* kmers_path, uint32_t kmer_len, uint32_t min_hits,
                          uint64_t max_reads_per_kmer, int32_t device, const char* out_prefix, kgwas_fetch_stats* st) {
    return guarded([&] { run(reads_path, mates_path, kmers_path, kmer_len, min_hits, max_reads_per_kmer, device, out_prefix, st); });
}

}  // extern "C"
