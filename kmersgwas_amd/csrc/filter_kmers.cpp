// filter_kmers.cpp — kgwas_filter_kmers / kgwas_filter_kmers_write: the reference's filter_kmers (src/filter_kmers.cpp) on the
// GPU, and kgwas_kmer_encode (kmer2bits, src/kmer_general.cpp:260-283).
//
// The table streams through Ingest (ingest.h). On every device piece fk_match / fk_select (filter_kernels.hip) apply the
// merge-join's parallel form up to the first descent of the table's keys; from that row on the host runs the merge-join
// itself over the piece's keys (8 B a row, copied back compacted) from the state the parallel rule left, and uploads the
// offsets it emits. The emitted rows of a piece are then formatted into text lines on the device (fk_format) - written by
// a thread of their own while the next piece is on the device - or gathered whole (fk_gather) for the library call that
// returns rows. No CPU fallback: without a device the calls fail with KGWAS_ERR_DEVICE.
#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstring>
#include <future>
#include <string>
#include <vector>

#include "common.h"
#include "device.h"
#include "ingest.h"
#include "kernels.h"
#include "sorted_file_io.h"

using namespace kgwas;

namespace {

// Text output budget of a piece: pieces are cut so that their emitted lines fit (every row of a piece may be emitted).
constexpr uint64_t TEXT_BUDGET = 256ull << 20;

void filter_run(kgwas_table* t, const uint64_t* codes, uint64_t n, int32_t device, const char* out_path, uint64_t* file_rows,
                uint64_t* rows_out, uint64_t* n_found) {
    if (!t || (!codes && n)) throw Error(KGWAS_ERR_ARG, "kgwas_filter_kmers: null argument");
    use_device(device);
    uint64_t S_f = 0, n_rows = 0, W_f = 0;
    uint32_t klen = 0;
    if (kgwas_table_info(t, &S_f, &n_rows, &W_f, &klen) != KGWAS_OK) throw Error(KGWAS_ERR_ARG, kgwas_last_error());
    if (out_path && (klen == 0 || klen > 32))
        throw Error(KGWAS_ERR_ARG, "kgwas_filter_kmers_write: the table's k-mer length " + std::to_string(klen) + " is not within 1..32");
    const uint64_t stride = 1 + W_f, width = (uint64_t)klen + 2 * S_f + 1;

    std::vector<uint64_t> L(codes, codes + n);
    std::sort(L.begin(), L.end());

    Fd f;
    const std::string path = out_path ? out_path : "";
    if (out_path) {
        open_output(f, path);
        std::string head = "kmer";  // src/filter_kmers.cpp:144-147
        for (uint64_t i = 0; i < S_f; i++) {
            const char* nm = nullptr;
            if (kgwas_table_name(t, i, &nm) != KGWAS_OK) throw Error(KGWAS_ERR_ARG, kgwas_last_error());
            head += '\t';
            head += nm;
        }
        head += '\n';
        write_all(f.fd, head.data(), head.size(), path);
    }
    uint64_t found = 0;
    if (n > 0 && n_rows > 0) {
        // splitters: every B-th list entry, at most FK_SPLITTERS of them
        const uint64_t B = (n + FK_SPLITTERS - 1) / FK_SPLITTERS, ns = (n + B - 1) / B;
        std::vector<uint64_t> spl(ns);
        for (uint64_t j = 0; j < ns; j++) spl[j] = L[j * B];
        DevBuf<uint64_t> d_L, d_spl, d_lb, d_cnt, d_out, d_small;
        DevBuf<uint32_t> d_head, d_start, d_sel;
        DevBuf<uint8_t> d_emit, d_temp;
        DevBuf<char> d_text;
        d_L.alloc(n);
        d_spl.alloc(ns);
        d_small.alloc(5);  // info[0..3], then u32 first descent | u32 selected
        KGWAS_HIP(hipMemcpy(d_L.p, L.data(), n * 8, hipMemcpyHostToDevice));
        KGWAS_HIP(hipMemcpy(d_spl.p, spl.data(), ns * 8, hipMemcpyHostToDevice));
        PinBuf<uint64_t> h_small, h_keys;
        PinBuf<char> h_text[2];
        h_small.alloc(5);
        std::vector<uint32_t> h_sel;
        Stream st;
        st.create(hipStreamNonBlocking);

        uint64_t max_piece = ~0ull;  // (the rows-only call: Ingest's own piece size)
        if (out_path) {
            const uint64_t budget_rows = std::max<uint64_t>(128, TEXT_BUDGET / width);
            if (n > budget_rows) max_piece = budget_rows;
        }
        uint64_t cap = 0, text_bytes = 0, out_lines = 0;
        size_t temp_bytes = 0;
        // merge-join state: parallel rule (carry of the last piece's last run) until the first descent, then the host's p
        bool has_prev = false, host_mode = false, done = false;
        uint64_t carry_key = 0, carry_run = 0, p = 0, handed = 0;
        std::future<void> pending;  // the text of the last piece being written (after h_text: its destructor waits for the writer)

        Ingest ingest;
        ingest.file_feed_ = true;
        ingest.run(
            stride, n_rows, max_piece, st,
            [&](uint64_t* dst, uint64_t row_off, uint64_t c) {
                if (kgwas_table_read_rows(t, row_off, c, dst) != KGWAS_OK) throw Error(KGWAS_ERR_IO, kgwas_last_error());
            },
            [&](const uint64_t* d_rows, uint64_t row_off, uint64_t c) {
                if (done) return;  // the list is used up: nothing more is emitted (src/filter_kmers.cpp:152)
                if (c > cap) {  // (the first piece is the largest)
                    cap = c;
                    out_lines = std::min<uint64_t>(n, cap);
                    d_lb.alloc(cap);
                    d_cnt.alloc(cap);
                    d_head.alloc(cap);
                    d_start.alloc(cap);
                    d_sel.alloc(cap);
                    d_emit.alloc(cap);
                    temp_bytes = fk_scan_temp_bytes((uint32_t)cap);
                    if (!temp_bytes) throw Error(KGWAS_ERR_DEVICE, "kgwas_filter_kmers: hipcub temp storage query failed");
                    d_temp.alloc(temp_bytes);
                    h_keys.alloc(cap);
                    h_sel.resize(cap);
                    if (out_path) {
                        text_bytes = (out_lines * width + 15) / 16 * 16;
                        d_text.alloc(text_bytes);
                        h_text[0].alloc(text_bytes);
                        h_text[1].alloc(text_bytes);
                    } else if (rows_out)
                        d_out.alloc(out_lines * stride);
                }
                const uint32_t cnt = (uint32_t)c;
                uint32_t m = 0, r_host = 0;
                if (!host_mode) {
                    KGWAS_HIP(hipMemsetAsync(d_small.p + 4, 0xFF, 4, st));
                    uint32_t* first_desc = reinterpret_cast<uint32_t*>(d_small.p + 4);
                    KGWAS_HIP(launch_fk_match(d_rows, stride, cnt, d_L.p, n, d_spl.p, (uint32_t)ns, B, carry_key, has_prev, d_lb.p,
                                              d_cnt.p, d_head.p, first_desc, st));
                    KGWAS_HIP(launch_fk_select(d_rows, stride, cnt, d_cnt.p, d_head.p, d_start.p, carry_run, first_desc, d_emit.p,
                                               d_sel.p, first_desc + 1, d_small.p, d_temp.p, temp_bytes, st));
                    KGWAS_HIP(hipMemcpyAsync(h_small.p, d_small.p, 5 * 8, hipMemcpyDeviceToHost, st));
                    KGWAS_HIP(hipStreamSynchronize(st));
                    uint32_t d;
                    memcpy(&d, h_small.p + 4, 4);
                    memcpy(&m, reinterpret_cast<const char*>(h_small.p + 4) + 4, 4);
                    if (d >= cnt) {
                        carry_run = h_small.p[0];
                        carry_key = h_small.p[1];
                        has_prev = true;
                    } else {  // the first descent of the table: the state after row d - 1
                        const uint64_t x = d ? h_small.p[3] : carry_key, run = d ? h_small.p[2] : carry_run;
                        const uint64_t lb = std::lower_bound(L.begin(), L.end(), x) - L.begin();
                        const uint64_t ub = std::upper_bound(L.begin(), L.end(), x) - L.begin();
                        p = lb + std::min(run, ub - lb);
                        host_mode = true;
                        r_host = d;
                    }
                }
                if (host_mode) {  // the reference's loop (src/filter_kmers.cpp:152-177) over rows [r_host, cnt)
                    uint32_t mh = 0;
                    if (p < n) {  // (d_lb, free once the match is through, holds the keys)
                        KGWAS_HIP(launch_fk_keys(d_rows, stride, r_host, cnt, d_lb.p, st));
                        KGWAS_HIP(hipMemcpyAsync(h_keys.p, d_lb.p, (size_t)(cnt - r_host) * 8, hipMemcpyDeviceToHost, st));
                        KGWAS_HIP(hipStreamSynchronize(st));
                        for (uint32_t r = r_host; r < cnt && p < n; r++) {
                            const uint64_t x = h_keys.p[r - r_host];
                            const uint64_t q = std::lower_bound(L.begin() + p, L.end(), x) - L.begin();
                            if (q == n) {
                                p = n;
                                break;
                            }
                            if (L[q] == x) {
                                h_sel[mh++] = r;
                                p = q + 1;
                            } else
                                p = q;
                        }
                        if (mh) KGWAS_HIP(hipMemcpyAsync(d_sel.p + m, h_sel.data(), (size_t)mh * 4, hipMemcpyHostToDevice, st));
                    }
                    m += mh;
                    if (p >= n) done = true;
                }
                if (m == 0) return;
                if (found + m > std::min<uint64_t>(n, n_rows) || m > out_lines)
                    throw Error(KGWAS_ERR_STATE, "kgwas_filter_kmers: more rows emitted than the list allows");
                if (out_path) {
                    char* h = h_text[handed & 1].p;
                    const uint64_t bytes = (uint64_t)m * width;
                    KGWAS_HIP(launch_fk_format(d_rows, stride, d_sel.p, m, klen, (uint32_t)S_f, d_text.p, st));
                    KGWAS_HIP(hipMemcpyAsync(h, d_text.p, bytes, hipMemcpyDeviceToHost, st));
                    KGWAS_HIP(hipStreamSynchronize(st));
                    if (pending.valid()) pending.get();  // (the piece before this one: its buffer is the other one)
                    pending = std::async(std::launch::async, [&f, &path, h, bytes] { write_all(f.fd, h, bytes, path); });
                    handed++;
                } else {
                    if (rows_out) {
                        KGWAS_HIP(launch_fk_gather(d_rows, stride, d_sel.p, m, d_out.p, st));
                        KGWAS_HIP(hipMemcpyAsync(rows_out + found * stride, d_out.p, (size_t)m * stride * 8, hipMemcpyDeviceToHost, st));
                    }
                    if (file_rows) KGWAS_HIP(hipMemcpyAsync(h_sel.data(), d_sel.p, (size_t)m * 4, hipMemcpyDeviceToHost, st));
                    KGWAS_HIP(hipStreamSynchronize(st));
                    if (file_rows)
                        for (uint32_t i = 0; i < m; i++) file_rows[found + i] = row_off + h_sel[i];
                }
                found += m;
            });
        if (pending.valid()) pending.get();
    }
    if (f.fd >= 0) close_output(f, path);
    if (n_found) *n_found = found;
}

}  // namespace

extern "C" {

int kgwas_kmer_encode(const char* word, uint64_t len, uint64_t* code) {
    return guarded([&] {
        if (!word || !code) throw Error(KGWAS_ERR_ARG, "kgwas_kmer_encode: null argument");
        if (len < 1 || len > 32) throw Error(KGWAS_ERR_ARG, "kgwas_kmer_encode: k-mers of 1 to 32 bases are supported");
        uint64_t b = 0;
        for (uint64_t i = 0; i < len; i++) {
            uint64_t d;
            switch (word[len - i - 1]) {
                case 'A': d = 0; break;
                case 'C': d = 1; break;
                case 'G': d = 2; break;
                case 'T': d = 3; break;
                default: throw Error(KGWAS_ERR_FORMAT, "Ilegal kmer");
            }
            b |= d << (i * 2);
        }
        uint64_t x = b;  // kmer_reverse_complement (src/kmer_general.h:102-109)
        x = ((x & 0xFFFFFFFF00000000ull) >> 32) | ((x & 0x00000000FFFFFFFFull) << 32);
        x = ((x & 0xFFFF0000FFFF0000ull) >> 16) | ((x & 0x0000FFFF0000FFFFull) << 16);
        x = ((x & 0xFF00FF00FF00FF00ull) >> 8) | ((x & 0x00FF00FF00FF00FFull) << 8);
        x = ((x & 0xF0F0F0F0F0F0F0F0ull) >> 4) | ((x & 0x0F0F0F0F0F0F0F0Full) << 4);
        x = ((x & 0xCCCCCCCCCCCCCCCCull) >> 2) | ((x & 0x3333333333333333ull) << 2);
        const uint64_t bt = (~x) >> (64 - len - len);
        *code = bt < b ? bt : b;
    });
}

int kgwas_filter_kmers(kgwas_table* t, const uint64_t* codes, uint64_t n, int32_t device, uint64_t* file_rows, uint64_t* rows,
                       uint64_t* n_found) {
    return guarded([&] { filter_run(t, codes, n, device, nullptr, file_rows, rows, n_found); });
}

int kgwas_filter_kmers_write(kgwas_table* t, const uint64_t* codes, uint64_t n, int32_t device, const char* out_path,
                             uint64_t* n_found) {
    return guarded([&] {
        if (!out_path) throw Error(KGWAS_ERR_ARG, "kgwas_filter_kmers_write: null output path");
        filter_run(t, codes, n, device, out_path, nullptr, nullptr, n_found);
    });
}

}  // extern "C"
