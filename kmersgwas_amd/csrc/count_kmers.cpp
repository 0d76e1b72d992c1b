// count_kmers.cpp — kgwas_count_kmers_files / kgwas_count_kmers_bases: an accession's sorted k-mer file from its reads, on the GPU.
// It stands where the reference pipeline runs `kmc -ci<T>`, `kmc -ci0 -b` and kmers_add_strand_information
// (src/kmers_add_strand_information.cpp:32-38,119-145) and writes that tool's output format; the counting rules are this
// project's own and are stated in include/kgwas.h and DESIGN.md §4.11.
//
// Host side. Parser threads turn the FASTA / FASTQ files into the BASE STREAM: the reads' bytes as they stand, one separator
// byte behind each read. A file is read in blocks by the thread that took it, cut at record boundaries that are certain - in
// FASTQ behind a line whose number, counted from the file's start, is a multiple of four; in FASTA in front of a line that
// begins with '>' - and the cut-off chunks are converted by whichever thread is free. A thread collects its reads in a pinned
// piece and uploads a full piece to room it claims in a device SEGMENT; a read longer than a piece claims its room at once and
// goes through the pieces in parts. Reads land in any order: counting does not depend on it. The whole stream stays resident.
//
// Counting runs in key-range PASSES of at most C sort words (count_kernels.hip): encode the windows of the range, sort, reduce
// the runs, append the kept words to the output. A single pass covers everything when the stream has no more than C bytes;
// otherwise the boundaries are quantiles of a sorted sample of canonical keys. A pass whose words exceed C is cut at the middle
// of its key range and redone; a single key with more than C words is decided from the encode kernel's two counters.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <deque>
#include <mutex>
#include <string>
#include <vector>

#include "common.h"
#include "device.h"
#include "kernels.h"
#include "reads_source.h"
#include "sorted_file_io.h"

using namespace kgwas;

namespace {

constexpr uint8_t SEP = '\n';
constexpr uint64_t FLAG_CANON = 0x4000000000000000ull, FLAG_NON = 0x8000000000000000ull;

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// ---- the resident base stream ---------------------------------------------------------------------------------------------------------
struct Segment {
    DevBuf<uint8_t> own;   // the segment's memory, unless it is the caller's
    uint8_t* p = nullptr;  // own.p, or the caller's memory
    uint64_t cap = 0, used = 0;
};

struct BaseStream {
    std::mutex mu;
    std::vector<Segment> segs;
    uint64_t seg_bytes = 256ull << 20;  // room of a new segment (more for a single claim above it)
    uint64_t min_pass_bytes = 0;        // what one pass of the smallest size needs beside the stream

    uint64_t bytes() const {
        uint64_t b = 0;
        for (auto& s : segs) b += s.used;
        return b;
    }
    // room for n bytes in one piece of device memory
    uint8_t* claim(uint64_t n) {
        std::lock_guard<std::mutex> lk(mu);
        if (segs.empty() || !segs.back().own.p || segs.back().used + n > segs.back().cap) {
            const uint64_t cap = (std::max(seg_bytes, n) + 255) / 256 * 256;
            size_t free_b = 0, total_b = 0;
            KGWAS_HIP(hipMemGetInfo(&free_b, &total_b));
            if (free_b < cap + min_pass_bytes) {
                uint64_t have = cap;
                for (auto& s : segs) have += s.cap;
                throw Error(KGWAS_ERR_ARG, "the bases of the input do not fit on the device: " + std::to_string(have) +
                                               " bytes of bases and at least " + std::to_string(min_pass_bytes) + " bytes of one pass's buffers, " +
                                               std::to_string(free_b) + " bytes of device memory free beside the bases so far");
            }
            Segment s;
            s.own.alloc(cap);
            s.p = s.own.p;
            s.cap = cap;
            segs.push_back(std::move(s));
        }
        Segment& s = segs.back();
        uint8_t* at = s.p + s.used;
        s.used += n;
        return at;
    }
};

// One parser thread's way to the device: an upload lane of two pinned pieces.
struct Uploader {
    BaseStream& out;
    uint64_t P;
    uint32_t k;
    UploadLane<uint8_t> lane;
    uint8_t* piece = nullptr;  // the piece in hand
    uint64_t fill = 0;

    Uploader(BaseStream& o, uint64_t piece_size, uint32_t kmer_len) : out(o), P(piece_size), k(kmer_len) {
        lane.create(P);
        piece = lane.take();
    }
    // the piece in hand goes to `dst`; the other one is in hand once its last copy is through
    void send(uint8_t* dst, uint64_t n) {
        KGWAS_HIP(hipMemcpyAsync(dst, piece, n, hipMemcpyHostToDevice, lane.st));
        lane.sent();
        piece = lane.take();
        fill = 0;
    }
    void flush() {
        if (fill) send(out.claim(fill), fill);
    }
    // n bytes that lie next to each other on the device, and a separator behind them if `sep`
    void put(const uint8_t* p, uint64_t n, bool sep) {
        const uint64_t len = n + (sep ? 1 : 0);
        if (fill + len > P) flush();
        if (len <= P) {
            memcpy(piece + fill, p, n);
            if (sep) piece[fill + n] = SEP;
            fill += len;
            return;
        }
        uint8_t* dst = out.claim(len);
        for (uint64_t o = 0; o < len; o += P) {
            const uint64_t part = std::min(P, len - o), from_p = std::min(part, n - std::min(n, o));
            memcpy(piece, p + o, from_p);
            if (from_p < part) piece[from_p] = SEP;
            send(dst + o, part);
        }
    }
    void read(const char* p, uint64_t n) {
        if (n >= k) put(reinterpret_cast<const uint8_t*>(p), n, true);  // (a shorter read has no window)
    }
    void finish() {
        flush();
        KGWAS_HIP(hipStreamSynchronize(lane.st));
    }
};

// ---- the files --------------------------------------------------------------------------------------------------------------------
struct Chunk {
    std::vector<char> data;  // whole records
    const Source* src = nullptr;
    bool last = false;  // the file ends with it
};

void convert(Chunk& c, Uploader& up) {
    char* d = c.data.data();
    const size_t n = c.data.size();
    if (c.src->fmt == '@') {
        for (size_t p = 0; p < n;) {
            size_t b[4], e[4];  // the record's four lines, without '\n'
            int lines = 0;
            for (; lines < 4 && p < n; lines++) {
                b[lines] = p;
                e[lines] = line_end(d, p, n);
                p = e[lines] + 1;
            }
            if (lines < 4) throw Error(KGWAS_ERR_FORMAT, c.src->path + ": the last FASTQ record has fewer than four lines");
            if (d[b[0]] != '@' || b[2] == e[2] || d[b[2]] != '+')
                throw Error(KGWAS_ERR_FORMAT, c.src->path + ": a FASTQ record does not have '@' and '+' at the head of its first and third line");
            size_t len = e[1] - b[1];
            if (len && d[b[1] + len - 1] == '\r') len--;
            up.read(d + b[1], len);
        }
    } else {
        // a record's sequence lines are moved together in place, then handed over as one read
        size_t rd = 0, len = 0;
        bool open_rec = false;
        for (size_t p = 0; p < n;) {
            const size_t e = line_end(d, p, n);
            size_t l = e - p;
            if (l && d[p + l - 1] == '\r') l--;
            if (d[p] == '>' ) {
                if (open_rec) up.read(d + rd, len);
                open_rec = true;
                rd = p, len = 0;
            } else {
                memmove(d + rd + len, d + p, l);
                len += l;
            }
            p = e + 1;
        }
        if (open_rec) up.read(d + rd, len);
    }
}

struct Parser {
    std::vector<Source>& src;
    BaseStream& out;
    uint64_t piece, block;
    uint32_t k;
    int dev;
    unsigned n_threads;
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Chunk> q;
    size_t next_file = 0;
    unsigned splitters = 0;
    bool failed = false;

    // reads the file block by block and hands whole records on
    void split(const Source& s, Uploader& up) {
        std::vector<char> buf;
        buf.push_back(s.fmt);  // (open_source took the first byte)
        size_t scanned = 0;    // FASTQ: buf[0, scanned) holds `lines` whole lines
        uint64_t lines = 0;
        for (bool eof = false; !eof;) {
            const size_t old = buf.size();
            buf.resize(old + block);
            size_t got = 0;
            while (got < block) {
                const size_t r = read_some(s.fd.fd, buf.data() + old + got, block - got, s.path);
                if (r == 0) {
                    eof = true;
                    break;
                }
                got += r;
            }
            buf.resize(old + got);
            size_t cut = 0;
            if (eof)
                cut = buf.size();
            else if (s.fmt == '@') {
                size_t last4 = 0;
                for (size_t p = scanned; p < buf.size();) {
                    const size_t e = line_end(buf.data(), p, buf.size());
                    if (e == buf.size()) break;
                    p = scanned = e + 1;
                    if (++lines % 4 == 0) last4 = scanned;
                }
                cut = last4;
            } else {
                const size_t from = std::max<size_t>(old, 1);  // (what was here before holds no cut)
                for (size_t p = buf.size(); p > from;) {
                    const void* g = memrchr(buf.data() + from, '>', p - from);
                    if (!g) break;
                    p = (size_t)(static_cast<const char*>(g) - buf.data());
                    if (buf[p - 1] == '\n') {
                        cut = p;
                        break;
                    }
                }
            }
            if (!cut) continue;  // (a record longer than what is here: read on)
            Chunk c;
            c.src = &s;
            c.last = eof;
            c.data.assign(buf.begin(), buf.begin() + cut);
            buf.erase(buf.begin(), buf.begin() + cut);
            scanned -= std::min(scanned, cut);
            bool mine = false;
            {
                std::unique_lock<std::mutex> lk(mu);
                if (failed) return;
                if (q.size() >= 2 * (size_t)n_threads)
                    mine = true;  // (the others are behind: no more memory is taken)
                else
                    q.push_back(std::move(c));
            }
            if (mine)
                convert(c, up);
            else
                cv.notify_one();
        }
    }

    void work() {
        KGWAS_HIP(hipSetDevice(dev));
        try {
            Uploader up(out, piece, k);
            for (;;) {
                Chunk c;
                size_t f = ~(size_t)0;
                {
                    std::unique_lock<std::mutex> lk(mu);
                    cv.wait(lk, [&] { return failed || !q.empty() || next_file < src.size() || splitters == 0; });
                    if (failed) break;
                    if (!q.empty()) {
                        c = std::move(q.front());
                        q.pop_front();
                    } else if (next_file < src.size()) {
                        f = next_file++;
                        splitters++;
                    } else
                        break;
                }
                if (f != ~(size_t)0) {
                    struct Done {
                        Parser& p;
                        ~Done() {
                            {
                                std::lock_guard<std::mutex> lk(p.mu);
                                p.splitters--;
                            }
                            p.cv.notify_all();
                        }
                    } done{*this};
                    if (src[f].fmt) split(src[f], up);
                } else
                    convert(c, up);
            }
            up.finish();
        } catch (...) {
            {
                std::lock_guard<std::mutex> lk(mu);
                failed = true;
            }
            cv.notify_all();
            throw;
        }
    }
};

// ---- the passes -----------------------------------------------------------------------------------------------------------------------
struct Counter {
    BaseStream& in;
    uint32_t k;
    uint64_t ci, cx;
    int out_fd;
    const std::string& out_path;
    uint64_t C = 0;
    DevBuf<uint64_t> d_a, d_b;  // a: the pass's words, then the runs' results; b: the sorted words, then the kept words
    DevBuf<uint32_t> d_heads, d_blk, d_off;
    DevBuf<unsigned long long> d_ctr, d_counts;
    DevBuf<char> d_temp;
    PinBuf<uint64_t> h_out[2];
    PinBuf<unsigned long long> h_ctr;
    Stream st;  // (after the buffers its work reads and writes: it goes first)
    size_t temp_bytes = 0;
    uint64_t host_counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t passes = 0, splits = 0, big_keys = 0;
    std::vector<uint64_t> sample_;  // the sampled canonical keys, sorted

    static uint64_t pass_bytes(uint64_t c, size_t temp) { return c * 20 + 2 * 4 * (uint64_t)ck_blocks(c) + temp + (1 << 20); }

    void setup(uint32_t max_sample) {
        const uint64_t total = in.bytes();
        uint64_t c = std::min<uint64_t>(CK_MAX_PASS_WORDS, std::max<uint64_t>(total, 1));
        const long long hook = opt_int("KGWAS_COUNT_PASS_WORDS", 0);
        if (hook > 0)
            c = std::min<uint64_t>((uint64_t)hook, CK_MAX_PASS_WORDS);
        else {
            size_t free_b = 0, total_b = 0;
            KGWAS_HIP(hipMemGetInfo(&free_b, &total_b));
            const uint64_t budget = free_b / 10 * 8;
            while (c > 1024 && pass_bytes(c, ck_temp_bytes(c, max_sample, k)) > budget) c = c / 4 * 3;
        }
        C = c;
        temp_bytes = ck_temp_bytes(C, max_sample, k);
        if (!temp_bytes) throw Error(KGWAS_ERR_DEVICE, "kgwas_count_kmers: hipcub temporary-storage query failed");
        st.create(hipStreamNonBlocking);
        d_a.alloc(C);
        d_b.alloc(C);
        d_heads.alloc(C);
        d_blk.alloc(ck_blocks(C));
        d_off.alloc(ck_blocks(C));
        d_ctr.alloc(2);
        d_counts.alloc(8);
        d_temp.alloc(temp_bytes);
        h_ctr.alloc(4);
        for (auto& h : h_out) h.alloc(std::min<uint64_t>(C, 4u << 20));
        KGWAS_HIP(hipMemsetAsync(d_counts.p, 0, 64, st));
    }

    void keep_on_host(uint64_t key, uint64_t count, bool has0, bool has1) {
        host_counts[1] += has0 + has1;
        if (count < ci || count > cx) return;
        host_counts[0]++;
        host_counts[2] += has0 + has1;
        host_counts[3 + (has0 ? 1 : 0) + (has1 ? 2 : 0)]++;
        const uint64_t w = key | (has0 ? FLAG_CANON : 0) | (has1 ? FLAG_NON : 0);
        write_all(out_fd, &w, 8, out_path);
    }

    // the windows with keys in [lo, hi): false when they are more than C and the range can be cut
    bool pass(uint64_t lo, uint64_t hi) {
        KGWAS_HIP(hipMemsetAsync(d_ctr.p, 0, 16, st));
        for (auto& s : in.segs) KGWAS_HIP(launch_ck_encode(s.p, s.used, k, lo, hi, d_a.p, C, d_ctr.p, st));
        KGWAS_HIP(hipMemcpyAsync(h_ctr.p, d_ctr.p, 16, hipMemcpyDeviceToHost, st));
        KGWAS_HIP(hipStreamSynchronize(st));
        const uint64_t n = h_ctr.p[0], n1 = h_ctr.p[1];
        if (n > C) {
            if (hi - lo > 1) return false;
            big_keys++;
            host_counts[7] += n;
            keep_on_host(lo, n, n1 < n, n1 > 0);
            return true;
        }
        passes++;
        host_counts[7] += n;
        if (!n) return true;
        KGWAS_HIP(launch_ck_sort(d_a.p, d_b.p, n, k, d_temp.p, temp_bytes, st));
        KGWAS_HIP(launch_ck_heads(d_b.p, n, d_blk.p, d_off.p, d_heads.p, d_temp.p, temp_bytes, st));
        KGWAS_HIP(hipMemcpyAsync(h_ctr.p + 2, d_off.p + (n + 2047) / 2048, 4, hipMemcpyDeviceToHost, st));
        KGWAS_HIP(hipStreamSynchronize(st));
        const uint32_t n_runs = *reinterpret_cast<const uint32_t*>(h_ctr.p + 2);
        KGWAS_HIP(launch_ck_reduce(d_b.p, n, d_heads.p, n_runs, ci, cx, d_a.p, d_blk.p, d_off.p, d_b.p, d_counts.p, d_temp.p, temp_bytes, st));
        KGWAS_HIP(hipMemcpyAsync(h_ctr.p + 3, d_off.p + ((uint64_t)n_runs + 2047) / 2048, 4, hipMemcpyDeviceToHost, st));
        KGWAS_HIP(hipStreamSynchronize(st));
        const uint64_t n_kept = *reinterpret_cast<const uint32_t*>(h_ctr.p + 3);
        // out in parts through the two pinned buffers: one is written to the file while the next is copied
        const uint64_t part = h_out[0].n;
        uint64_t prev_cnt = 0;
        int i = 0;
        for (uint64_t o = 0; o < n_kept || prev_cnt; o += part, i ^= 1) {
            const uint64_t cnt = o < n_kept ? std::min(part, n_kept - o) : 0;
            if (cnt) KGWAS_HIP(hipMemcpyAsync(h_out[i].p, d_b.p + o, cnt * 8, hipMemcpyDeviceToHost, st));
            if (prev_cnt) write_all(out_fd, h_out[i ^ 1].p, prev_cnt * 8, out_path);
            KGWAS_HIP(hipStreamSynchronize(st));
            prev_cnt = cnt;
        }
        return true;
    }

    // the boundaries between `ranges` key ranges: quantiles of a sample of the canonical keys
    std::vector<uint64_t> boundaries(uint64_t ranges, uint32_t max_sample) {
        const uint64_t total = in.bytes();
        const uint32_t want = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(max_sample, C), total);
        std::vector<uint32_t> per_seg;
        uint32_t m = 0;
        for (auto& s : in.segs) {
            const uint32_t ms = s.used ? (uint32_t)std::min<uint64_t>(s.used, std::max<uint64_t>(1, (uint64_t)want * s.used / total)) : 0;
            per_seg.push_back(m + ms <= want ? ms : want - m);
            m += per_seg.back();
        }
        // (d_a: the raw sample, d_b: the sorted one; both hold C >= m words)
        uint32_t at = 0;
        for (size_t i = 0; i < in.segs.size(); at += per_seg[i], i++)
            if (per_seg[i]) KGWAS_HIP(launch_ck_sample(in.segs[i].p, in.segs[i].used, k, per_seg[i], d_a.p + at, st));
        std::vector<uint64_t> sample(m), cuts;
        if (m) {
            KGWAS_HIP(launch_ck_sort_sample(d_a.p, d_b.p, m, d_temp.p, temp_bytes, st));
            KGWAS_HIP(hipMemcpyAsync(sample.data(), d_b.p, (size_t)m * 8, hipMemcpyDeviceToHost, st));
            KGWAS_HIP(hipStreamSynchronize(st));
        }
        const uint64_t v = (uint64_t)(std::lower_bound(sample.begin(), sample.end(), ~0ull) - sample.begin());  // the counted windows among them
        sample_.assign(sample.begin(), sample.begin() + v);
        for (uint64_t r = 1; r < ranges && v; r++) {
            const uint64_t key = sample[r * v / ranges];
            if (key > (cuts.empty() ? 0 : cuts.back())) cuts.push_back(key);
        }
        return cuts;
    }

    void run() {
        const uint32_t max_sample = 1u << 18;
        setup(max_sample);
        const uint64_t total = in.bytes(), top = 1ull << (2 * k);
        std::deque<std::pair<uint64_t, uint64_t>> todo;
        if (total <= C)
            todo.emplace_back(0, top);
        else {
            // (every window has a byte of its own: aim at passes that are half full)
            uint64_t lo = 0;
            for (uint64_t cut : boundaries((total + C / 2 - 1) / std::max<uint64_t>(C / 2, 1), max_sample)) {
                todo.emplace_back(lo, cut);
                lo = cut;
            }
            todo.emplace_back(lo, top);
        }
        while (!todo.empty()) {
            const auto r = todo.front();
            todo.pop_front();
            if (pass(r.first, r.second)) continue;
            // cut at the median of the sampled keys inside the range, or, where the sample does not tell, in the middle of the range
            uint64_t mid = r.first + (r.second - r.first) / 2;
            const auto i0 = std::lower_bound(sample_.begin(), sample_.end(), r.first), i1 = std::lower_bound(i0, sample_.end(), r.second);
            if (i1 - i0 >= 2 && *(i0 + (i1 - i0) / 2) > r.first) mid = *(i0 + (i1 - i0) / 2);
            todo.emplace_front(mid, r.second);
            todo.emplace_front(r.first, mid);
            splits++;
        }
        unsigned long long dev_counts[8];
        KGWAS_HIP(hipMemcpyAsync(dev_counts, d_counts.p, 64, hipMemcpyDeviceToHost, st));
        KGWAS_HIP(hipStreamSynchronize(st));
        for (int i = 0; i < 7; i++) host_counts[i] += dev_counts[i];
    }
};

void check_args(const char* who, uint32_t kmer_len, uint64_t ci, uint64_t cx, const char* out_path) {
    if (!out_path) throw Error(KGWAS_ERR_ARG, std::string(who) + ": null argument");
    if (kmer_len < 1 || kmer_len > 31) throw Error(KGWAS_ERR_ARG, std::string(who) + ": k-mer lengths of 1 to 31 are supported");
    if (ci > cx) throw Error(KGWAS_ERR_ARG, std::string(who) + ": the minimum count " + std::to_string(ci) + " is above the maximum count " + std::to_string(cx));
}

uint64_t piece_bytes() { return (uint64_t)std::max<long long>(16, std::min<long long>(opt_int("KGWAS_COUNT_PIECE_BYTES", 8 << 20), 1 << 28)); }

void count_stream(BaseStream& in, uint32_t kmer_len, uint64_t ci, uint64_t cx, const char* out_path, uint64_t counts[8], double t0, double t_in) {
    const std::string out(out_path);
    Fd f;
    open_output(f, out);
    Counter c{in, kmer_len, ci, cx, f.fd, out};
    c.run();
    close_output(f, out);
    if (counts)
        for (int i = 0; i < 8; i++) counts[i] = c.host_counts[i];
    if (opt_set("KGWAS_TRACE"))
        fprintf(stderr, "[kgwas] count: passes=%llu splits=%llu big_keys=%llu pass_words=%llu bases=%llu segments=%llu windows=%llu input_s=%.4f count_s=%.4f\n",
                (unsigned long long)c.passes, (unsigned long long)c.splits, (unsigned long long)c.big_keys, (unsigned long long)c.C,
                (unsigned long long)in.bytes(), (unsigned long long)in.segs.size(), (unsigned long long)c.host_counts[7], t_in - t0, now_s() - t_in);
}

uint64_t min_pass_bytes(uint32_t kmer_len) { return Counter::pass_bytes(1 << 20, ck_temp_bytes(1 << 20, 1u << 18, kmer_len)); }

void files_run(const char* const* paths, uint64_t n, uint32_t kmer_len, uint64_t ci, uint64_t cx, int32_t device, const char* out_path,
               uint64_t counts[8]) {
    const double t0 = now_s();
    check_args("kgwas_count_kmers_files", kmer_len, ci, cx, out_path);
    if (!paths && n) throw Error(KGWAS_ERR_ARG, "kgwas_count_kmers_files: null argument");
    for (uint64_t i = 0; i < n; i++)
        if (!paths[i]) throw Error(KGWAS_ERR_ARG, "kgwas_count_kmers_files: null argument");
    std::vector<Source> src(n);
    uint64_t known = 0;
    bool all_known = true;
    for (uint64_t i = 0; i < n; i++) {
        open_source(src[i], paths[i]);
        struct stat sb;
        if (fstat(src[i].fd.fd, &sb) == 0 && S_ISREG(sb.st_mode))
            known += (uint64_t)sb.st_size;
        else
            all_known = false;
    }
    use_device(device);
    BaseStream in;
    const bool hooked = opt_set("KGWAS_COUNT_PIECE_BYTES");
    const uint64_t piece = piece_bytes();
    // (a read takes no more room in the stream than its record in the file)
    in.seg_bytes = hooked ? 64 * piece : all_known ? std::min<uint64_t>(std::max<uint64_t>(known, 4096), 1ull << 30) : 256ull << 20;
    in.min_pass_bytes = min_pass_bytes(kmer_len);
    unsigned nt = std::max(1u, std::min(8u, kgwas_host_cpu_quota()));
    if (hooked) nt = std::min(nt, 3u);
    Parser p{src, in, piece, hooked ? 8 * piece : 4ull << 20, kmer_len, device, nt};
    kgwas_run_on_threads(nt, "kgwas-count", [&] { p.work(); });
    if (opt_set("KGWAS_COUNT_PARSE_ONLY")) {  // (timing mode of the tool: the host parse and the upload alone)
        if (counts) std::fill(counts, counts + 8, 0);
        fprintf(stderr, "[kgwas] count: parse only, bases=%llu input_s=%.4f\n", (unsigned long long)in.bytes(), now_s() - t0);
        return;
    }
    count_stream(in, kmer_len, ci, cx, out_path, counts, t0, now_s());
}

void bases_run(const void* bases, uint64_t n_bytes, int on_device, uint32_t kmer_len, uint64_t ci, uint64_t cx, int32_t device,
               const char* out_path, uint64_t counts[8]) {
    const double t0 = now_s();
    check_args("kgwas_count_kmers_bases", kmer_len, ci, cx, out_path);
    if (!bases && n_bytes) throw Error(KGWAS_ERR_ARG, "kgwas_count_kmers_bases: null argument");
    use_device(device);
    BaseStream in;
    in.min_pass_bytes = min_pass_bytes(kmer_len);
    if (on_device) {
        Segment s;
        s.p = const_cast<uint8_t*>(static_cast<const uint8_t*>(bases));
        s.cap = s.used = n_bytes;
        if (n_bytes) in.segs.push_back(std::move(s));
    } else if (n_bytes) {
        in.seg_bytes = n_bytes;
        Uploader up(in, std::min<uint64_t>(piece_bytes(), std::max<uint64_t>(n_bytes, 16)), kmer_len);
        up.put(static_cast<const uint8_t*>(bases), n_bytes, false);
        up.finish();
    }
    count_stream(in, kmer_len, ci, cx, out_path, counts, t0, now_s());
}

}  // namespace

extern "C" {

int kgwas_count_kmers_files(const char* const* paths, uint64_t n, uint32_t kmer_len, uint64_t ci, uint64_t cx, int32_t device,
                            const char* out_path, uint64_t counts[8]) {
    return guarded([&] { files_run(paths, n, kmer_len, ci, cx, device, out_path, counts); });
}

int kgwas_count_kmers_bases(const void* bases, uint64_t n_bytes, int on_device, uint32_t kmer_len, uint64_t ci, uint64_t cx, int32_t device,
                            const char* out_path, uint64_t counts[8]) {
    return guarded([&] { bases_run(bases, n_bytes, on_device, kmer_len, ci, cx, device, out_path, counts); });
}

}  // extern "C"
