// list_kmers.cpp — kgwas_list_kmers: the reference's list_kmers_found_in_multiple_samples
// (src/list_kmers_found_in_multiple_samples.cpp, KmersSingleDataBaseSortedFile in src/kmers_single_database.cpp:90-177) on the GPU.
//
// The reference walks 5001 key windows (threshold step * i); in each, every file hands over the words it has not handed over
// yet, up to the first one above the threshold, and one hash map counts the window's words per key and strand flag. Here the
// windows run in PIECES, each a run of whole windows i..j, and every file's slice of a piece is read by the same rule with the
// threshold step * j, block by block, into one device buffer. Every word that is read is used: it is at or below step * j <=
// step * 5001. The word that ended a file's previous slice is above every word before it, so a descent never straddles two
// pieces, and in a piece where no slice descends a word's window is decided by its key alone: the window's hash map is a count
// per key and the reference's output order is key order, which list_kernels.hip computes without sorting the words. A piece in
// which a slice descends, a single window larger than the piece budget and a piece one of whose buckets overflows its table
// go through host_piece below: the reference's loop itself, from the same slices. Pieces are planned from the file sizes; one
// that does not fit the budget is cut in half and read again. A piece's outputs are written by a thread of their own while
// the next piece is counted. No CPU fallback: without a device the call fails with KGWAS_ERR_DEVICE.
#include <algorithm>
#include <atomic>
#include <charconv>
#include <cmath>
#include <cstdio>
#include <future>
#include <string>
#include <unordered_map>
#include <vector>

#include "common.h"
#include "device.h"
#include "kernels.h"
#include "sorted_file_io.h"

using namespace kgwas;

namespace {

constexpr uint64_t KEY_MASK = SORTED_KEY_MASK;
constexpr uint64_t STEPS = 5000;  // src/list_kmers_found_in_multiple_samples.cpp:144; windows 1 .. STEPS + 1 are run
constexpr uint32_t SAMPLES_PER_BUCKET = 16;

// bits2kmer31 (src/kmer_general.cpp:77-87)
std::string kmer_text(uint64_t w, uint32_t k) {
    std::string res(k, 'X');
    for (uint32_t i = 0; i < k; i++, w >>= 2) res[k - 1 - i] = "ACGT"[w & 3];
    return res;
}

void append_num(std::string& s, uint64_t v) {
    char buf[24];
    s.append(buf, std::to_chars(buf, buf + sizeof buf, v).ptr);
}

void append_no_pass(std::string& text, uint64_t key, uint32_t k, uint64_t all, uint64_t canon, uint64_t non) {
    text += kmer_text(key, k);
    for (uint64_t v : {all, canon, non, all - canon - non}) {
        text += '\t';
        append_num(text, v);
    }
    text += '\n';
}

struct Counts {
    uint64_t all = 0, canon = 0, non = 0;
};

struct Lister {
    std::vector<std::string> paths;
    uint64_t N = 0, N1 = 1, NN = 1, step = 0, mac = 0;
    uint32_t k = 0;
    std::vector<uint64_t> words, pos, head;  // per file: words in it, words handed over, the key of the next word (while pos < words)
    std::vector<uint32_t> need;              // [N + 1]: the smallest count of a strand side with (double)count >= ceil(p * all), or none
    std::vector<uint64_t> stats;             // as ListArgs::stats without the shards: what host_piece counted, at the end everything
    uint64_t cnt_pass = 0, cnt_no_pass = 0, cnt_low = 0;
    uint64_t block_words = 0;
    unsigned n_threads = 1;
    int dev = 0;

    uint64_t window_of(uint64_t x) const { return kgwas::window_of(x, step); }
    bool file_has(uint64_t c, uint64_t thr) const { return pos[c] < words[c] && head[c] <= thr; }
    void ended(uint64_t c, const SliceEnd& r) {  // file c's slice of a piece has been walked
        pos[c] = r.pos;
        if (r.above) head[c] = r.head;
    }

    [[noreturn]] void flag_zero(uint64_t c) const {
        throw Error(KGWAS_ERR_FORMAT, "a k-mer word without strand flags (flag 0) in: " + paths[c]);
    }
    [[noreturn]] void above_n(uint64_t key) const {
        throw Error(KGWAS_ERR_FORMAT, "k-mer " + kmer_text(key, k) + " is counted more often than there are files (" + std::to_string(N) +
                                          "): a file repeats it");
    }

    // The decision and the statistics of one distinct key (:173-199); true: it passes.
    bool decide(uint64_t key, const Counts& c, std::string& no_pass) {
        if (c.all > N) above_n(key);
        const uint64_t both = c.all - c.canon - c.non;
        stats[c.all * N1 + c.canon]++;
        stats[NN + c.all * N1 + c.non]++;
        stats[2 * NN + c.all * N1 + both]++;
        if (c.all < mac) {
            cnt_low++;
            return false;
        }
        const uint32_t nd = need[c.all];
        if (nd != LL_NEED_NONE && c.canon + both >= nd && c.non + both >= nd) {
            cnt_pass++;
            stats[3 * NN + c.all]++;
            return true;
        }
        append_no_pass(no_pass, key, k, c.all, c.canon, c.non);
        cnt_no_pass++;
        return false;
    }

    // The reference's loop over windows w0..w1 on the host: every file's slice read from pos[c] by the reference's rule with
    // threshold thr, a word's window from the running maximum of its slice, one hash map per window.
    void host_piece(uint64_t w0, uint64_t w1, uint64_t thr, std::vector<uint64_t>& pass, std::string& no_pass) {
        std::vector<std::unordered_map<uint64_t, Counts>> maps(w1 - w0 + 1);
        std::vector<uint64_t> buf(block_words);
        uint64_t zero_window = ~0ull, zero_file = 0;  // the flag-0 word the reference meets first: lowest window, then first file
        for (uint64_t c = 0; c < N; c++) {
            if (!file_has(c, thr)) continue;
            uint64_t m = 0;
            ended(c, walk_slice(paths[c], pos[c], words[c], block_words, thr, [&] { return buf.data(); }, [&](const uint64_t* h, uint64_t e) {
                for (uint64_t i = 0; i < e; i++) {
                    const uint64_t x = h[i] & KEY_MASK, flag = h[i] >> 62;
                    m = std::max(m, x);
                    const uint64_t w = std::min(std::max(window_of(m), w0), w1);
                    if (flag == 0) {
                        if (w < zero_window) zero_window = w, zero_file = c;
                        continue;
                    }
                    Counts& n = maps[w - w0][x];
                    n.all++;
                    n.canon += flag == 1;
                    n.non += flag == 2;
                }
                return true;
            }));
        }
        std::vector<uint64_t> keys;
        for (auto& map : maps) {
            if (w0 + (uint64_t)(&map - maps.data()) == zero_window) flag_zero(zero_file);  // (the windows before it are written first)
            keys.clear();
            for (auto& kv : map) keys.push_back(kv.first);
            std::sort(keys.begin(), keys.end());
            for (uint64_t key : keys)
                if (decide(key, map[key], no_pass)) pass.push_back(key);
        }
    }
};

void write_text_file(const std::string& path, const std::string& text) {
    Fd f;
    open_output(f, path);
    write_all(f.fd, text.data(), text.size(), path);
    close_output(f, path);
}

void list_run(const char* const* kmer_paths, uint64_t n_files, uint32_t kmer_len, uint64_t mac, double min_strand_percent, int32_t device,
              const char* out_path, uint64_t counts[3]) {
    if (!out_path || (!kmer_paths && n_files)) throw Error(KGWAS_ERR_ARG, "kgwas_list_kmers: null argument");
    if (kmer_len < 1 || kmer_len > 31) throw Error(KGWAS_ERR_ARG, "kgwas_list_kmers: k-mer lengths of 1 to 31 are supported");
    for (uint64_t i = 0; i < n_files; i++)
        if (!kmer_paths[i]) throw Error(KGWAS_ERR_ARG, "kgwas_list_kmers: null argument");
    if (n_files >= (1ull << 20))  // (the reference's three 20-bit counters in one word overflow)
        throw Error(KGWAS_ERR_FORMAT, "too many k-mer files: " + std::to_string(n_files) + " (at most 1048575)");

    Lister b;
    b.dev = device;
    b.N = n_files;
    b.N1 = n_files + 1;
    b.NN = b.N1 * b.N1;
    b.k = kmer_len;
    b.mac = mac;
    b.step = kmers_step_to_threshold(STEPS, kmer_len);
    b.paths.assign(kmer_paths, kmer_paths + n_files);
    b.words.resize(n_files);
    b.pos.assign(n_files, 0);
    b.head.resize(n_files);
    for (uint64_t c = 0; c < n_files; c++) {
        b.words[c] = words_in_file(b.paths[c], &b.head[c]);
        b.head[c] &= KEY_MASK;
    }
    // (every guard of the reference is through: only now is the device touched)
    use_device(device);

    // need[all]: ceil(p * all) is an integer, an infinity or NaN, so (double)m >= it is m >= it in integers
    b.need.resize(b.N1);
    for (uint64_t all = 0; all <= b.N; all++) {
        const double t = std::ceil(min_strand_percent * static_cast<double>(all));
        b.need[all] = std::isnan(t) || t > 4194304.0 ? LL_NEED_NONE : t <= 0.0 ? 0u : (uint32_t)t;
    }
    const uint64_t n_stats = 3 * b.NN + b.N1;
    b.stats.assign(n_stats, 0);
    b.n_threads = std::max(2u, std::min(8u, kgwas_host_cpu_quota() / 2));
    b.block_words = (uint64_t)std::max<long long>(1, std::min<long long>(opt_int("KGWAS_LIST_BLOCK_WORDS", 1 << 16), 1 << 24));
    const uint64_t cap = (uint64_t)std::max<long long>(1, std::min<long long>(opt_int("KGWAS_LIST_PIECE_WORDS", 1 << 25), 1 << 30));
    const uint64_t bucket_words = (uint64_t)std::max<long long>(1, std::min<long long>(opt_int("KGWAS_LIST_BUCKET_WORDS", 2048), 1 << 30));
    uint32_t slots = 64;  // a table of twice the bucket's words, within 64 .. LL_MAX_SLOTS
    while (slots < LL_MAX_SLOTS && slots < 2 * bucket_words) slots *= 2;
    const uint32_t max_nb = (uint32_t)std::min<uint64_t>((cap + bucket_words - 1) / bucket_words, 1u << 22);
    const uint32_t max_m = (uint32_t)std::min<uint64_t>(cap, (uint64_t)max_nb * SAMPLES_PER_BUCKET);

    const std::string out(out_path), np_path = out + ".no_pass_kmers";
    Fd f_out, f_np;
    open_output(f_out, out);
    open_output(f_np, np_path);
    {
        const std::string h = "kmer\tcount_all\tcanonical\tnon-canonical\tboth\n";
        write_all(f_np.fd, h.data(), h.size(), np_path);
    }

    DevBuf<uint64_t> d_words, d_stage[3], d_out[3], d_sample_raw, d_sample;
    DevBuf<uint32_t> d_seg_off, d_seg_len, d_bk, d_off, d_need, d_flags;
    DevBuf<unsigned long long> d_piece_stats, d_total_stats, d_err_key;
    DevBuf<char> d_temp;
    PinBuf<uint64_t> h_out[2][3];
    PinBuf<uint32_t> h_seg, h_flags;
    PinBuf<unsigned long long> h_err_key;
    const size_t temp_bytes = ll_temp_bytes(max_m, max_nb);
    if (!temp_bytes) throw Error(KGWAS_ERR_DEVICE, "kgwas_list_kmers: hipcub temporary-storage query failed");
    const uint64_t n_dev_stats = n_stats + TESTED_SHARDS;
    if (b.N) {
        d_words.alloc(cap);
        for (auto& d : d_stage) d.alloc(cap);
        for (auto& d : d_out) d.alloc(cap);
        d_sample_raw.alloc(max_m);
        d_sample.alloc(max_m);
        d_bk.alloc(3 * ((size_t)max_nb + 1));
        d_off.alloc(2 * ((size_t)max_nb + 1));
        d_need.alloc(b.N1);
        d_flags.alloc(4);
        d_err_key.alloc(1);
        d_piece_stats.alloc(n_dev_stats);
        d_total_stats.alloc(n_dev_stats);
        d_temp.alloc(temp_bytes);
        h_flags.alloc(8);
        h_err_key.alloc(2);
        KGWAS_HIP(hipMemcpy(d_need.p, b.need.data(), b.N1 * 4, hipMemcpyHostToDevice));
        KGWAS_HIP(hipMemset(d_piece_stats.p, 0, n_dev_stats * 8));
        KGWAS_HIP(hipMemset(d_total_stats.p, 0, n_dev_stats * 8));
    }
    Stream st;
    st.create(hipStreamNonBlocking);
    // one lane of the slice readers: its upload lane and what it put into the piece
    struct Lane {
        UploadLane<uint64_t> up;
        std::vector<uint32_t> segs;  // (offset, length) of the blocks it put into the piece
    };
    std::vector<Lane> lanes(b.N ? b.n_threads : 0);
    for (auto& l : lanes) l.up.create(b.block_words);
    std::future<void> pending;  // the outputs of the last device piece being written (after h_out: its destructor waits for the writer)

    // windows per piece, from the file sizes: three quarters of the budget if every window held the same number of words
    uint64_t all_words = 0;
    for (uint64_t c = 0; c < b.N; c++) all_words += b.words[c];
    uint64_t wpp = std::max<uint64_t>(1, std::min<uint64_t>(STEPS + 1, cap / 4 * 3 / std::max<uint64_t>(1, all_words / (STEPS + 1))));
    uint64_t handed = 0, host_pieces = 0, reread = 0, words_used = 0;
    std::vector<uint64_t> host_pass;
    std::string host_text;
    for (uint64_t w_next = 1; w_next <= STEPS + 1;) {
        // ---- the next piece: windows w_next .. j; windows in which no file has a word are passed over ---------------------------
        uint64_t lowest = ~0ull;
        for (uint64_t c = 0; c < b.N; c++)
            if (b.pos[c] < b.words[c]) lowest = std::min(lowest, b.head[c]);
        if (lowest == ~0ull) break;
        w_next = std::max(w_next, b.window_of(lowest));
        if (w_next > STEPS + 1) break;  // the words that are left are never used
        const uint64_t j = std::min(STEPS + 1, w_next + wpp - 1), thr = b.step * j;
        const std::vector<uint64_t> start_pos = b.pos, start_head = b.head;

        // ---- its slices into the device buffer ---------------------------------------------------------------------------------
        const uint32_t init[4] = {0u, 0xFFFFFFFFu, 0u, 0u};
        memcpy(h_flags.p, init, 16);
        h_err_key.p[0] = ~0ull;
        KGWAS_HIP(hipMemcpyAsync(d_flags.p, h_flags.p, 16, hipMemcpyHostToDevice, st));
        KGWAS_HIP(hipMemcpyAsync(d_err_key.p, h_err_key.p, 8, hipMemcpyHostToDevice, st));
        KGWAS_HIP(hipStreamSynchronize(st));
        std::atomic<uint64_t> next(0), total(0);
        std::atomic<unsigned> next_lane(0);
        std::atomic<bool> no_fit(false);
        for (auto& l : lanes) l.segs.clear();
        kgwas_run_on_threads((unsigned)std::min<uint64_t>(b.n_threads, b.N), "kgwas-list", [&] {
            KGWAS_HIP(hipSetDevice(b.dev));
            Lane& l = lanes[next_lane.fetch_add(1)];
            for (uint64_t c; !no_fit.load() && (c = next.fetch_add(1)) < b.N;) {
                if (!b.file_has(c, thr)) continue;
                uint64_t carry = 0;
                bool has_prev = false;
                // (a piece that does not fit stops every walk: its files are rewound below, whatever the walks leave behind)
                b.ended(c, walk_slice(b.paths[c], b.pos[c], b.words[c], b.block_words, thr, [&] { return l.up.take(); }, [&](const uint64_t* h, uint64_t e) {
                    if (no_fit.load()) return false;
                    if (e) {
                        const uint64_t off = total.fetch_add(e);
                        if (off + e > cap) {
                            no_fit.store(true);
                            return false;
                        }
                        KGWAS_HIP(hipMemcpyAsync(d_words.p + off, h, e * 8, hipMemcpyHostToDevice, l.up.st));
                        KGWAS_HIP(launch_ll_check(d_words.p + off, (uint32_t)e, carry, has_prev, (uint32_t)c, d_flags.p, l.up.st));
                        l.up.sent();
                        l.segs.push_back((uint32_t)off);
                        l.segs.push_back((uint32_t)e);
                        carry = h[e - 1] & KEY_MASK;
                        has_prev = true;
                    }
                    return true;
                }));
            }
            KGWAS_HIP(hipStreamSynchronize(l.up.st));
        });
        const auto rewind = [&] { b.pos = start_pos, b.head = start_head; };
        if (no_fit.load()) {
            rewind();
            if (j > w_next) {  // fewer windows, read again
                wpp = (j - w_next + 1) / 2;
                reread++;
                continue;
            }
        }
        const uint64_t n = total.load();
        bool on_host = no_fit.load();  // a single window above the budget
        uint32_t n_pass = 0, n_np = 0;
        if (!on_host) {
            KGWAS_HIP(hipMemcpyAsync(h_flags.p, d_flags.p, 16, hipMemcpyDeviceToHost, st));
            KGWAS_HIP(hipStreamSynchronize(st));
            // a slice descends, or a word has flag 0: the host's loop finds the one the reference meets first
            on_host = h_flags.p[0] != 0 || h_flags.p[1] != 0xFFFFFFFFu;
        }
        if (!on_host && n) {
            // ---- the device's count ------------------------------------------------------------------------------------------------
            uint32_t n_seg = 0;
            for (auto& l : lanes) n_seg += (uint32_t)(l.segs.size() / 2);
            if (h_seg.n < 2 * (size_t)n_seg) h_seg.alloc(2 * (size_t)n_seg + 1024);
            if (d_seg_off.n < n_seg) d_seg_off.alloc(n_seg + 512), d_seg_len.alloc(n_seg + 512);
            uint32_t s = 0;
            for (auto& l : lanes)
                for (size_t i = 0; i < l.segs.size(); i += 2, s++) h_seg.p[s] = l.segs[i], h_seg.p[n_seg + s] = l.segs[i + 1];
            ListArgs a{};
            a.words = d_words.p;
            a.seg_off = d_seg_off.p;
            a.seg_len = d_seg_len.p;
            a.n_seg = n_seg;
            a.sample = d_sample.p;
            a.nb = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(max_nb, n), (n + bucket_words - 1) / bucket_words));
            a.m = (uint32_t)std::min<uint64_t>(n, (uint64_t)a.nb * SAMPLES_PER_BUCKET);
            a.slots = slots;
            a.N = b.N;
            a.mac = b.mac;
            a.need = d_need.p;
            a.stage_pass = d_stage[0].p;
            a.stage_np_key = d_stage[1].p;
            a.stage_np_cnt = d_stage[2].p;
            a.bk_base = d_bk.p;
            a.bk_pass = d_bk.p + (a.nb + 1);
            a.bk_np = d_bk.p + 2 * ((size_t)a.nb + 1);
            a.stats = d_piece_stats.p;
            a.flags = d_flags.p;
            a.err_key = d_err_key.p;
            KGWAS_HIP(hipMemcpyAsync(d_seg_off.p, h_seg.p, (size_t)n_seg * 4, hipMemcpyHostToDevice, st));
            KGWAS_HIP(hipMemcpyAsync(d_seg_len.p, h_seg.p + n_seg, (size_t)n_seg * 4, hipMemcpyHostToDevice, st));
            KGWAS_HIP(hipMemsetAsync(d_bk.p, 0, 3 * ((size_t)a.nb + 1) * 4, st));
            KGWAS_HIP(launch_ll_splitters(d_words.p, n, a.m, d_sample_raw.p, d_sample.p, d_temp.p, temp_bytes, st));
            KGWAS_HIP(launch_ll_count(a, st));
            KGWAS_HIP(hipMemcpyAsync(h_flags.p, d_flags.p, 16, hipMemcpyDeviceToHost, st));
            KGWAS_HIP(hipMemcpyAsync(h_err_key.p + 1, d_err_key.p, 8, hipMemcpyDeviceToHost, st));
            KGWAS_HIP(hipStreamSynchronize(st));
            if (h_flags.p[2]) {  // a bucket's table filled: the host's loop counts this piece from the same slices
                on_host = true;
                KGWAS_HIP(hipMemsetAsync(d_piece_stats.p, 0, n_dev_stats * 8, st));
                KGWAS_HIP(hipStreamSynchronize(st));
            } else {
                if (h_flags.p[3]) b.above_n(h_err_key.p[1]);
                uint32_t* off_pass = d_off.p;
                uint32_t* off_np = d_off.p + (a.nb + 1);
                KGWAS_HIP(launch_ll_gather(a, off_pass, off_np, d_out[0].p, d_out[1].p, d_out[2].p, d_temp.p, temp_bytes, st));
                KGWAS_HIP(launch_ll_commit(d_total_stats.p, d_piece_stats.p, n_dev_stats, st));
                KGWAS_HIP(hipMemcpyAsync(h_flags.p + 4, off_pass + a.nb, 4, hipMemcpyDeviceToHost, st));
                KGWAS_HIP(hipMemcpyAsync(h_flags.p + 5, off_np + a.nb, 4, hipMemcpyDeviceToHost, st));
                KGWAS_HIP(hipStreamSynchronize(st));
                n_pass = h_flags.p[4];
                n_np = h_flags.p[5];
                auto& ho = h_out[handed & 1];  // (its last writer, two pieces ago, is through: see below)
                if (ho[0].n < n_pass) ho[0].alloc(n_pass + n_pass / 4 + 1024);
                if (ho[1].n < n_np) ho[1].alloc(n_np + n_np / 4 + 1024), ho[2].alloc(n_np + n_np / 4 + 1024);
                if (n_pass) KGWAS_HIP(hipMemcpyAsync(ho[0].p, d_out[0].p, (size_t)n_pass * 8, hipMemcpyDeviceToHost, st));
                if (n_np) {
                    KGWAS_HIP(hipMemcpyAsync(ho[1].p, d_out[1].p, (size_t)n_np * 8, hipMemcpyDeviceToHost, st));
                    KGWAS_HIP(hipMemcpyAsync(ho[2].p, d_out[2].p, (size_t)n_np * 8, hipMemcpyDeviceToHost, st));
                }
                KGWAS_HIP(hipStreamSynchronize(st));
            }
        }
        if (on_host) {
            rewind();
            host_pieces++;
            host_pass.clear();
            host_text.clear();
            b.host_piece(w_next, j, thr, host_pass, host_text);
            if (pending.valid()) pending.get();
            write_all(f_out.fd, host_pass.data(), host_pass.size() * 8, out);
            write_all(f_np.fd, host_text.data(), host_text.size(), np_path);
        } else if (n) {
            b.cnt_pass += n_pass;
            b.cnt_no_pass += n_np;
            if (pending.valid()) pending.get();  // (the piece before this one: its buffers are the other ones)
            const uint64_t* hp = h_out[handed & 1][0].p;
            const uint64_t* hk = h_out[handed & 1][1].p;
            const uint64_t* hc = h_out[handed & 1][2].p;
            const int fd_out = f_out.fd, fd_np = f_np.fd;
            const uint32_t k = b.k;
            pending = std::async(std::launch::async, [=, &out, &np_path] {
                write_all(fd_out, hp, (size_t)n_pass * 8, out);
                std::string text;
                for (uint32_t i = 0; i < n_np; i++)
                    append_no_pass(text, hk[i], k, hc[i] & 0x1FFFFF, (hc[i] >> 21) & 0x1FFFFF, (hc[i] >> 42) & 0x1FFFFF);
                write_all(fd_np, text.data(), text.size(), np_path);
            });
            handed++;
        }
        if (!no_fit.load()) words_used += n;
        if (n < cap / 4) wpp = std::min<uint64_t>(STEPS + 1, wpp * 2);
        w_next = j + 1;
    }
    if (pending.valid()) pending.get();
    if (opt_set("KGWAS_TRACE"))
        fprintf(stderr, "[kgwas] list: device_pieces=%llu host_pieces=%llu reread=%llu device_words=%llu\n", (unsigned long long)handed,
                (unsigned long long)host_pieces, (unsigned long long)reread, (unsigned long long)words_used);
    close_output(f_out, out);
    close_output(f_np, np_path);
    if (b.N) {  // the device's statistics to the host's
        std::vector<unsigned long long> dev_stats(n_dev_stats);
        KGWAS_HIP(hipMemcpy(dev_stats.data(), d_total_stats.p, n_dev_stats * 8, hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < n_stats; i++) b.stats[i] += dev_stats[i];
        for (uint64_t i = n_stats; i < n_dev_stats; i++) b.cnt_low += dev_stats[i];
    }

    // ---- the closing files (:209-218) ---------------------------------------------------------------------------------------------
    std::string text = "kmer appearance\tcount\n";
    for (uint64_t i = 0; i <= b.N; i++) {
        append_num(text, i);
        text += '\t';
        append_num(text, b.stats[3 * b.NN + i]);
        text += '\n';
    }
    write_text_file(out + ".shareness", text);
    const char* const ext[3] = {".stats.only_canonical", ".stats.only_non_canonical", ".stats.both"};
    for (int mth = 0; mth < 3; mth++) {
        text.clear();
        for (uint64_t i = 0; i <= b.N; i++)
            for (uint64_t c = 0; c <= b.N; c++) {
                append_num(text, b.stats[mth * b.NN + i * b.N1 + c]);
                text += c < b.N ? '\t' : '\n';
            }
        write_text_file(out + ext[mth], text);
    }
    if (counts) counts[0] = b.cnt_pass, counts[1] = b.cnt_no_pass, counts[2] = b.cnt_low;
}

}  // namespace

extern "C" {

int kgwas_list_kmers(const char* const* kmer_paths, uint64_t n, uint32_t kmer_len, uint64_t mac, double min_strand_percent, int32_t device,
                     const char* out_path, uint64_t counts[3]) {
    return guarded([&] { list_run(kmer_paths, n, kmer_len, mac, min_strand_percent, device, out_path, counts); });
}

}  // extern "C"
