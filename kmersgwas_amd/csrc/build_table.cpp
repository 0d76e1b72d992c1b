// build_table.cpp — kgwas_build_table: the reference's build_kmers_table (src/build_kmers_table.cpp,
// src/kmers_merge_multiple_databaes.cpp, KmersSingleDataBaseSortedFile in src/kmers_single_database.cpp:90-177) on the GPU.
//
// The reference walks 5001 key windows (threshold step * i); in each, every file hands over the words it has not handed over
// yet, up to the first one above the threshold, and a hash map of the window's all-k-mers words (first insert wins) finds the
// row of each accession word. Here the all-k-mers file streams in PIECES, each a run of whole windows i..j, and every
// accession's slice of a piece is read by the same rule with the threshold step * j. The word that ended a file's previous
// slice is above every word before it, so a descent never straddles two pieces, and in a piece where no file descends a
// word's window is decided by its key alone: the window's hash map is then plain membership, first of equal keys, which
// bt_match (build_kernels.hip) computes with a lower bound. A piece in which the all-k-mers words or any slice descend, and a
// single window larger than the piece budget, go through host_piece below: the reference's loop itself, from the same
// slices. The finished rows of a piece are written by a thread of their own while the next piece is matched. No CPU
// fallback: without a device the call fails with KGWAS_ERR_DEVICE.
#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstring>
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
constexpr uint64_t TOTAL_ITER = 5000;                 // src/build_kmers_table.cpp:98; windows 1 .. TOTAL_ITER + 1 are run

struct Builder {
    std::string all_path;
    std::vector<std::string> paths;
    uint64_t S = 0, W = 0, stride = 0, step = 0;
    uint64_t a_words = 0, a_pos = 0;
    std::vector<uint64_t> words, pos;  // per accession: words in the file, words handed over
    uint64_t block_words = 0;
    unsigned n_threads = 1;
    int dev = 0;

    uint64_t window_of(uint64_t x) const { return kgwas::window_of(x, step); }

    // The reference's loop over the windows of one piece on the host: A[0, n) masked all-k-mers words (windows from their
    // running maximum), every accession's slice read from pos[c] by the reference's rule with threshold thr. rows: n x stride,
    // keys and zeroes on entry. One hash map per window, first insert wins; threads take whole words of 64 accessions.
    void host_piece(const uint64_t* A, uint64_t n, uint64_t thr, uint64_t* rows) {
        std::vector<uint32_t> wa(n);
        uint64_t pm = 0;
        for (uint64_t r = 0; r < n; r++) {
            pm = std::max(pm, A[r]);
            wa[r] = (uint32_t)window_of(pm);
        }
        const uint32_t w0 = n ? wa[0] : 0, w1 = n ? wa[n - 1] : 0;
        std::vector<std::unordered_map<uint64_t, uint64_t>> maps(n ? w1 - w0 + 1 : 0);
        for (uint64_t r = 0; r < n; r++) maps[wa[r] - w0].emplace(A[r], r);
        std::atomic<uint64_t> next(0);
        kgwas_run_on_threads(n_threads, "kgwas-build", [&] {
            std::vector<uint64_t> buf(block_words);
            for (uint64_t wd; (wd = next.fetch_add(1)) < W;) {
                for (uint64_t c = wd * 64; c < std::min(S, wd * 64 + 64); c++) {
                    const uint64_t bit = 1ull << (c % 64);
                    uint64_t m = 0;
                    pos[c] = walk_slice(paths[c], pos[c], words[c], block_words, thr, [&] { return buf.data(); }, [&](const uint64_t* h, uint64_t e) {
                        for (uint64_t i = 0; i < e; i++) {
                            const uint64_t x = h[i] & KEY_MASK;
                            m = std::max(m, x);
                            const uint64_t w = window_of(m);
                            if (w < w0 || w > w1) continue;
                            auto it = maps[w - w0].find(x);
                            if (it != maps[w - w0].end()) rows[it->second * stride + 1 + wd] |= bit;
                        }
                        return true;
                    }).pos;
                }
            }
        });
    }
};

void build_run(const char* all_kmers_path, const char* const* kmer_paths, const char* const* names, uint64_t n_acc, uint32_t kmer_len,
               int32_t device, const char* out_base, uint64_t* n_rows_out) {
    if (!all_kmers_path || !out_base || (!kmer_paths && n_acc)) throw Error(KGWAS_ERR_ARG, "kgwas_build_table: null argument");
    if (kmer_len < 1 || kmer_len > 31) throw Error(KGWAS_ERR_ARG, "kgwas_build_table: k-mer lengths of 1 to 31 are supported");
    for (uint64_t i = 0; i < n_acc; i++)
        if (!kmer_paths[i] || (names && !names[i])) throw Error(KGWAS_ERR_ARG, "kgwas_build_table: null argument");

    const std::string base(out_base), table_path = base + ".table";
    if (names) {  // (src/build_kmers_table.cpp:80-91)
        const std::string np = base + ".names";
        Fd f;
        open_output(f, np);
        std::string text;
        for (uint64_t i = 0; i < n_acc; i++) text += std::string(names[i]) + "\n";
        write_all(f.fd, text.data(), text.size(), np);
    }

    Builder b;
    b.dev = device;
    b.all_path = all_kmers_path;
    b.S = n_acc;
    b.W = (n_acc + 63) / 64;
    b.stride = 1 + b.W;
    b.step = kmers_step_to_threshold(TOTAL_ITER, kmer_len);
    const uint64_t last_thr = b.step * (TOTAL_ITER + 1);
    // the member initialiser opens the all-k-mers file first, the constructor's body the accessions' in order
    b.a_words = words_in_file(b.all_path);
    b.paths.assign(kmer_paths, kmer_paths + n_acc);
    b.words.resize(n_acc);
    b.pos.assign(n_acc, 0);
    for (uint64_t c = 0; c < n_acc; c++) b.words[c] = words_in_file(b.paths[c]);
    // (every guard of the reference is through: only now is the device touched)
    use_device(device);
    b.n_threads = std::max(2u, std::min(8u, kgwas_host_cpu_quota() / 2));
    b.block_words = (uint64_t)std::max<long long>(1, std::min<long long>(opt_int("KGWAS_BUILD_BLOCK_WORDS", 1 << 16), 1 << 24));
    // rows of a piece: 256 MiB of rows on the device (pieces small enough that writing one overlaps matching the next)
    uint64_t budget = std::max<uint64_t>(128, std::min<uint64_t>((256ull << 20) / (8 * b.stride), 1ull << 26));
    if (const long long e = opt_int("KGWAS_BUILD_PIECE_ROWS", 0))
        if (e > 0) budget = std::min<uint64_t>((uint64_t)e, 1ull << 26);

    Fd out;
    open_output(out, table_path);
    {
        char head[16] = {(char)0xAA, (char)0xBB, (char)0xCC, (char)0xDD};
        const uint64_t acc = n_acc;
        memcpy(head + 4, &acc, 8);
        memcpy(head + 12, &kmer_len, 4);
        write_all(out.fd, head, 16, table_path);
    }

    Fd a_fd;
    open_input(a_fd, b.all_path);
    const uint64_t cap = budget + 1;  // (a piece that ends the file may have one word more than the budget)
    const uint64_t B = (cap + FK_SPLITTERS - 1) / FK_SPLITTERS;
    DevBuf<uint64_t> d_A, d_spl, d_rows;
    DevBuf<uint32_t> d_flag;
    PinBuf<uint64_t> h_A, h_spl, h_out[2];
    PinBuf<uint32_t> h_flag;
    d_A.alloc(cap);
    d_spl.alloc(FK_SPLITTERS);
    d_rows.alloc(cap * b.stride);
    d_flag.alloc(1);
    h_A.alloc(cap);
    h_spl.alloc(FK_SPLITTERS);
    h_flag.alloc(1);
    Stream st;
    st.create(hipStreamNonBlocking);
    // one lane of the slice readers: its upload lane and a device block for each of the lane's two
    struct Lane {
        DevBuf<uint64_t> d[2];
        UploadLane<uint64_t> up;
    };
    std::vector<Lane> lanes(b.n_threads);
    for (auto& l : lanes) {
        l.up.create(b.block_words);
        for (auto& d : l.d) d.alloc(b.block_words);
    }
    std::future<void> pending;  // the rows of the last piece being written (after h_out: its destructor waits for the writer)

    std::vector<uint64_t> big_A, host_rows;  // a window above the budget; rows made on the host
    uint64_t total_rows = 0, handed = 0;
    bool last = false;
    while (!last && b.a_pos < b.a_words) {
        // ---- the next piece: as many whole windows as fit the budget ----------------------------------------------------------
        const uint64_t cnt = std::min(cap, b.a_words - b.a_pos);
        const bool more = b.a_pos + cnt < b.a_words;
        read_words(a_fd.fd, h_A.p, b.a_pos, cnt, b.all_path);
        uint64_t pm = 0, prev = 0, cur_w = 0, first_of_w = 0, n = cnt;
        bool desc = false, desc_before_w = false, cut_last = false;
        for (uint64_t j = 0; j < cnt; j++) {
            const uint64_t x = h_A.p[j] & KEY_MASK;
            if (x > pm || j == 0) {
                pm = std::max(pm, x);
                if (pm > last_thr) {  // this word and all after it are never used
                    n = j;
                    cut_last = true;
                    break;
                }
                const uint64_t w = b.window_of(pm);
                if (w != cur_w) cur_w = w, first_of_w = j, desc_before_w = desc;
            }
            if (j && x < prev) desc = true;
            prev = x;
        }
        const uint64_t* A = h_A.p;
        uint64_t thr;
        bool host_only = false;
        if (cut_last || !more) {  // the rest of the file: no row lies in a window above its last word's
            last = true;
            thr = b.step * cur_w;
        } else if (first_of_w > 0) {  // windows below the buffer's last one are whole
            n = first_of_w;
            desc = desc_before_w;
            thr = b.step * (cur_w - 1);
        } else {  // one window fills the buffer: read it whole, it goes to the host's loop
            host_only = true;
            thr = b.step * cur_w;
            big_A.assign(h_A.p, h_A.p + cnt);
            uint64_t p = b.a_pos + cnt;
            bool end = false;
            while (!end && p < b.a_words) {
                const uint64_t c2 = std::min<uint64_t>(1 << 20, b.a_words - p), o = big_A.size();
                big_A.resize(o + c2);
                read_words(a_fd.fd, big_A.data() + o, p, c2, b.all_path);
                const uint64_t e = first_above(big_A.data() + o, c2, thr);
                end = e < c2;
                big_A.resize(o + e);
                p += e;
            }
            n = big_A.size();
            A = big_A.data();
            if (p >= b.a_words) last = true;
        }
        b.a_pos += n;
        if (n == 0) break;  // (the file's next word is above the last threshold)

        const std::vector<uint64_t> start = b.pos;
        bool on_host = host_only || desc || b.S == 0;
        uint64_t* out_rows = nullptr;
        if (!on_host) {
            // ---- the device's match ----------------------------------------------------------------------------------------------
            const uint64_t ns = (n + B - 1) / B;
            for (uint64_t j = 0; j < ns; j++) h_spl.p[j] = h_A.p[j * B] & KEY_MASK;
            if (h_out[handed & 1].n < n * b.stride) {
                if (pending.valid()) pending.get();
                h_out[handed & 1].alloc(cap * b.stride);
            }
            KGWAS_HIP(hipMemcpyAsync(d_A.p, h_A.p, n * 8, hipMemcpyHostToDevice, st));
            KGWAS_HIP(hipMemcpyAsync(d_spl.p, h_spl.p, ns * 8, hipMemcpyHostToDevice, st));
            KGWAS_HIP(hipMemsetAsync(d_flag.p, 0, 4, st));
            KGWAS_HIP(launch_bt_init(d_A.p, n, b.stride, d_rows.p, st));
            KGWAS_HIP(hipStreamSynchronize(st));
            std::atomic<uint64_t> next(0);
            std::atomic<unsigned> next_lane(0);
            kgwas_run_on_threads((unsigned)std::min<uint64_t>(b.n_threads, std::max<uint64_t>(1, b.S)), "kgwas-build", [&] {
                KGWAS_HIP(hipSetDevice(b.dev));
                Lane& l = lanes[next_lane.fetch_add(1)];
                for (uint64_t c; (c = next.fetch_add(1)) < b.S;) {
                    uint64_t carry = 0;
                    bool has_prev = false;
                    b.pos[c] = walk_slice(b.paths[c], b.pos[c], b.words[c], b.block_words, thr, [&] { return l.up.take(); }, [&](const uint64_t* h, uint64_t e) {
                        if (e) {
                            uint64_t* d = l.d[l.up.cur].p;
                            KGWAS_HIP(hipMemcpyAsync(d, h, e * 8, hipMemcpyHostToDevice, l.up.st));
                            KGWAS_HIP(launch_bt_match(d_A.p, n, d_spl.p, (uint32_t)ns, B, d, (uint32_t)e, carry, has_prev, d_rows.p, b.stride, c,
                                                      d_flag.p, l.up.st));
                            l.up.sent();
                            carry = h[e - 1] & KEY_MASK;
                            has_prev = true;
                        }
                        return true;
                    }).pos;
                }
                KGWAS_HIP(hipStreamSynchronize(l.up.st));
            });
            KGWAS_HIP(hipMemcpyAsync(h_flag.p, d_flag.p, 4, hipMemcpyDeviceToHost, st));
            KGWAS_HIP(hipStreamSynchronize(st));
            if (*h_flag.p)
                on_host = true;  // a slice descends: the host's loop makes this piece's rows from the same slices
            else {
                out_rows = h_out[handed & 1].p;
                KGWAS_HIP(hipMemcpyAsync(out_rows, d_rows.p, n * b.stride * 8, hipMemcpyDeviceToHost, st));
                KGWAS_HIP(hipStreamSynchronize(st));
            }
        }
        if (on_host) {
            b.pos = start;
            host_rows.assign(n * b.stride, 0);
            std::vector<uint64_t> masked(n);
            for (uint64_t r = 0; r < n; r++) host_rows[r * b.stride] = masked[r] = A[r] & KEY_MASK;
            b.host_piece(masked.data(), n, thr, host_rows.data());
            if (pending.valid()) pending.get();
            write_all(out.fd, host_rows.data(), host_rows.size() * 8, table_path);
        } else {
            if (pending.valid()) pending.get();  // (the piece before this one: its buffer is the other one)
            const int fd = out.fd;
            const size_t bytes = n * b.stride * 8;
            pending = std::async(std::launch::async, [fd, out_rows, bytes, &table_path] { write_all(fd, out_rows, bytes, table_path); });
            handed++;
        }
        total_rows += n;
    }
    if (pending.valid()) pending.get();
    close_output(out, table_path);
    if (n_rows_out) *n_rows_out = total_rows;
}

}  // namespace

extern "C" {

int kgwas_build_table(const char* all_kmers_path, const char* const* kmer_paths, const char* const* names, uint64_t n,
                      uint32_t kmer_len, int32_t device, const char* out_base, uint64_t* n_rows) {
    return guarded([&] { build_run(all_kmers_path, kmer_paths, names, n, kmer_len, device, out_base, n_rows); });
}

}  // extern "C"
