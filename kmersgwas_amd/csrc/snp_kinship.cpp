// snp_kinship.cpp — kgwas_snpkin_*: emma_kinship (src/emma_kinship.cpp) on the GPU.
//
// open     : the reference's guards in its order (:77-88), all on the host, then the device session: the pair sums
//            (S x S doubles, lower triangle used), the lower-triangular tile list, two .bed chunk buffers on the device and
//            two pinned ones on the host;
// feed     : per chunk of SNPs the raw bytes go to the device on a copy stream, snpkin_prep_kernel and
//            snpkin_accumulate_kernel run on the compute stream (snpkin_kernels.hip). The chunks of a session run in SNP
//            order on one stream, so each pair's sum is the reference's sequential sum; the host fills chunk i + 1 and the
//            copy stream moves it while chunk i is accumulated;
// matrix   : the final division (:149-154) on the host, so that 0 / 0 is x86's default NaN (printed "-nan") as there.
// No CPU fallback: the accumulation needs the GPU.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "common.h"
#include "device.h"
#include "kernels.h"

using namespace kgwas;

struct kgwas_snpkin {
    std::string base;
    int device = 0;
    uint64_t S = 0, M = 0, bps = 0;
    uint32_t chunk = 0;  // SNPs per launch pair
    int rows_per_wave = 4;
    uint32_t n_tiles = 0;
    bool copied_pending[2] = {false, false}, used_pending[2] = {false, false};
    int slot = 0;
    DevBuf<uint8_t> d_bed[2];
    PinBuf<uint8_t> h_bed[2];
    DevBuf<uint8_t> d_params, d_vals;
    DevBuf<uint2> d_tiles;
    DevBuf<double> d_sums;
    DevBuf<unsigned long long> d_n;
    Stream stream, copy;  // (behind the buffers their work reads and writes: they go first)
    Event ev_copied[2], ev_used[2];
    bool on_device = false;
    ~kgwas_snpkin() {
        if (on_device) (void)hipSetDevice(device);  // (before any member is released)
    }
};

namespace {

// is_not_true (:27-31): the reference's message, "error:\t" + text
[[noreturn]] void fail(int code, const char* msg) { throw Error(code, std::string("error:\t") + msg); }

// count_samples_in_fam_file (:33-43): the lines getline() returns - a last line without '\n' counts, and so does a blank
// line before the end
uint64_t count_fam_lines(const std::string& path) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) fail(KGWAS_ERR_IO, "couldn't open fam file");
    uint64_t lines = 0;
    int last = '\n';
    char buf[1 << 16];
    for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;) {
        for (size_t i = 0; i < n; i++) lines += buf[i] == '\n';
        last = (unsigned char)buf[n - 1];
    }
    const bool err = ferror(f);
    fclose(f);
    if (err) fail(KGWAS_ERR_IO, "couldn't open fam file");
    return lines + (last != '\n' ? 1 : 0);
}

// Lower-triangular tiles of rw rows x 64 columns that hold at least one pair r > c, rows of the triangle first.
std::vector<uint2> make_tiles(uint32_t S, uint32_t rw) {
    std::vector<uint2> t;
    for (uint32_t r0 = 0; r0 < S; r0 += rw) {
        const uint32_t rmax = std::min(r0 + rw, S) - 1;  // the tile's last row: pairs need c < rmax
        for (uint32_t c0 = 0; c0 < rmax; c0 += 64) t.push_back(make_uint2(r0, c0));
    }
    return t;
}

void device_init(kgwas_snpkin* h) {
    use_device(h->device);
    h->on_device = true;
    const uint32_t S = (uint32_t)h->S;
    // 8 rows per wave where that still puts 2 waves on each of the MI355X's 1024 SIMDs, else 4 (S = 1135: 2 664 waves)
    std::vector<uint2> tiles = make_tiles(S, 8);
    h->rows_per_wave = 8;
    if (tiles.size() < 2048) {
        tiles = make_tiles(S, 4);
        h->rows_per_wave = 4;
    }
    h->n_tiles = (uint32_t)tiles.size();
    // chunks: the per-sample values of a chunk take 32 (S + 8) bytes per SNP; about 128 MiB of them (S = 1135: 3 648 SNPs)
    uint64_t chunk = (128ull << 20) / (32ull * snpkin_vals_stride(S));
    chunk = std::max<uint64_t>(64, std::min<uint64_t>(16384, chunk) / 64 * 64);
    const long long forced = opt_int("KGWAS_SNPKIN_CHUNK_SNPS", 0);
    if (forced > 0) chunk = (uint64_t)std::min<long long>(forced, 1 << 20);
    h->chunk = (uint32_t)chunk;
    h->stream.create(hipStreamNonBlocking);
    h->copy.create(hipStreamNonBlocking);
    for (int b = 0; b < 2; b++) {
        h->ev_copied[b].create(hipEventDisableTiming);
        h->ev_used[b].create(hipEventDisableTiming);
        h->d_bed[b].alloc(chunk * h->bps);
        h->h_bed[b].alloc(chunk * h->bps);
    }
    h->d_params.alloc(snpkin_params_bytes(h->chunk));
    h->d_vals.alloc(snpkin_vals_bytes(S, h->chunk));
    h->d_tiles.alloc(std::max<size_t>(tiles.size(), 1));
    if (!tiles.empty()) KGWAS_HIP(hipMemcpy(h->d_tiles.p, tiles.data(), tiles.size() * sizeof(uint2), hipMemcpyHostToDevice));
    h->d_sums.alloc(h->S * h->S);
    KGWAS_HIP(hipMemset(h->d_sums.p, 0, h->S * h->S * sizeof(double)));
    h->d_n.alloc(TESTED_SHARDS);
    KGWAS_HIP(hipMemset(h->d_n.p, 0, TESTED_SHARDS * sizeof(unsigned long long)));
    KGWAS_HIP(hipStreamSynchronize(nullptr));  // (null-stream memsets: the non-blocking streams below do not wait for them)
}

// n_snps SNPs in chunks; fill(dst, first, count) writes SNPs [first, first + count) of this feed into pinned memory.
template <class Fill>
void feed(kgwas_snpkin* h, uint64_t n_snps, const Fill& fill) {
    KGWAS_HIP(hipSetDevice(h->device));
    const uint32_t S = (uint32_t)h->S, bps = (uint32_t)h->bps;
    for (uint64_t pos = 0; pos < n_snps; pos += h->chunk) {
        const uint32_t c = (uint32_t)std::min<uint64_t>(h->chunk, n_snps - pos);
        const int b = h->slot;
        h->slot ^= 1;
        if (h->copied_pending[b]) KGWAS_HIP(hipEventSynchronize(h->ev_copied[b]));  // pinned buffer b is free again
        fill(h->h_bed[b].p, pos, c);
        if (h->used_pending[b]) KGWAS_HIP(hipStreamWaitEvent(h->copy, h->ev_used[b], 0));  // device buffer b too
        KGWAS_HIP(hipMemcpyAsync(h->d_bed[b].p, h->h_bed[b].p, (size_t)c * bps, hipMemcpyHostToDevice, h->copy));
        KGWAS_HIP(hipEventRecord(h->ev_copied[b], h->copy));
        h->copied_pending[b] = true;
        KGWAS_HIP(hipStreamWaitEvent(h->stream, h->ev_copied[b], 0));
        KGWAS_HIP(launch_snpkin_prep(h->d_bed[b].p, c, bps, S, h->d_params.p, h->d_vals.p, h->d_n.p, h->stream));
        KGWAS_HIP(launch_snpkin_accumulate(h->rows_per_wave, h->d_bed[b].p, c, bps, S, h->d_params.p, h->d_vals.p, h->d_tiles.p,
                                           h->n_tiles, h->d_sums.p, h->stream));
        KGWAS_HIP(hipEventRecord(h->ev_used[b], h->stream));
        h->used_pending[b] = true;
    }
    KGWAS_HIP(hipStreamSynchronize(h->stream));
}

void read_sums(kgwas_snpkin* h, double* lower, uint64_t* n_used) {
    KGWAS_HIP(hipSetDevice(h->device));
    KGWAS_HIP(hipStreamSynchronize(h->stream));
    KGWAS_HIP(hipMemcpy(lower, h->d_sums.p, h->S * h->S * sizeof(double), hipMemcpyDeviceToHost));
    unsigned long long shards[TESTED_SHARDS];
    KGWAS_HIP(hipMemcpy(shards, h->d_n.p, sizeof(shards), hipMemcpyDeviceToHost));
    uint64_t n = 0;
    for (unsigned long long v : shards) n += v;
    *n_used = n;
}

}  // namespace

extern "C" {

int kgwas_snpkin_open(const char* base_bedbim, int32_t device, kgwas_snpkin** out) {
    return guarded([&] {
        if (!base_bedbim || !out) throw Error(KGWAS_ERR_ARG, "kgwas_snpkin_open: null argument");
        std::unique_ptr<kgwas_snpkin> h(new kgwas_snpkin);
        h->base = base_bedbim;
        h->device = device;
        // emma_kinship (:77-88): the .bed opens, holds the magic, the .fam opens, the size fits - in that order
        std::ifstream bed(h->base + ".bed", std::ios::binary | std::ios::ate);
        if (!bed.is_open()) fail(KGWAS_ERR_IO, "couldn't open bed file");
        const uint64_t bed_size = (uint64_t)bed.tellg();
        if (bed_size < 3) fail(KGWAS_ERR_FORMAT, "Bed file is too small");
        h->S = count_fam_lines(h->base + ".fam");
        if (h->S == 0)  // the reference divides by zero here (SIGFPE)
            throw Error(KGWAS_ERR_ARG, "error:\t" + h->base + ".fam lists no samples");
        h->bps = (h->S + 3) / 4;
        h->M = (bed_size - 3) / h->bps;
        if (bed_size != h->M * h->bps + 3) fail(KGWAS_ERR_FORMAT, "Ilegal size of bed file");
        if (h->S >= (1ull << 20)) throw Error(KGWAS_ERR_ARG, "kgwas_snpkin_open: more than 2^20 samples");
        device_init(h.get());
        *out = h.release();
    });
}

int kgwas_snpkin_info(const kgwas_snpkin* h, uint64_t* n_samples, uint64_t* n_snps, uint64_t* bytes_per_snp) {
    return guarded([&] {
        if (!h) throw Error(KGWAS_ERR_ARG, "kgwas_snpkin_info: null session");
        if (n_samples) *n_samples = h->S;
        if (n_snps) *n_snps = h->M;
        if (bytes_per_snp) *bytes_per_snp = h->bps;
    });
}

int kgwas_snpkin_feed_bed(kgwas_snpkin* h, const uint8_t* body, uint64_t n_snps) {
    return guarded([&] {
        if (!h || (!body && n_snps)) throw Error(KGWAS_ERR_ARG, "kgwas_snpkin_feed_bed: null argument");
        feed(h, n_snps, [&](uint8_t* dst, uint64_t first, uint32_t c) { memcpy(dst, body + first * h->bps, (size_t)c * h->bps); });
    });
}

int kgwas_snpkin_feed_file(kgwas_snpkin* h) {
    return guarded([&] {
        if (!h) throw Error(KGWAS_ERR_ARG, "kgwas_snpkin_feed_file: null session");
        FILE* f = fopen((h->base + ".bed").c_str(), "rb");
        if (!f) throw Error(KGWAS_ERR_IO, "error:\tcouldn't open bed file");
        std::unique_ptr<FILE, int (*)(FILE*)> closer(f, fclose);
        if (fseek(f, 3, SEEK_SET) != 0) throw Error(KGWAS_ERR_IO, "kgwas_snpkin_feed_file: cannot seek in the .bed");
        feed(h, h->M, [&](uint8_t* dst, uint64_t, uint32_t c) {
            if (fread(dst, 1, (size_t)c * h->bps, f) != (size_t)c * h->bps)
                throw Error(KGWAS_ERR_IO, "kgwas_snpkin_feed_file: short read of " + h->base + ".bed");
        });
    });
}

int kgwas_snpkin_sums(kgwas_snpkin* h, double* lower, uint64_t* n_used) {
    return guarded([&] {
        if (!h || !lower || !n_used) throw Error(KGWAS_ERR_ARG, "kgwas_snpkin_sums: null argument");
        read_sums(h, lower, n_used);
    });
}

int kgwas_snpkin_matrix(kgwas_snpkin* h, double* K, uint64_t* n_used) {
    return guarded([&] {
        if (!h || !K || !n_used) throw Error(KGWAS_ERR_ARG, "kgwas_snpkin_matrix: null argument");
        read_sums(h, K, n_used);
        const uint64_t S = h->S;
        const double den = 2. * (double)*n_used;  // (:151)
        for (uint64_t r = 0; r < S; r++) {
            K[r * S + r] = 1;
            for (uint64_t c = 0; c < r; c++) {
                K[r * S + c] /= den;
                K[c * S + r] = K[r * S + c];
            }
        }
    });
}

void kgwas_snpkin_close(kgwas_snpkin* h) { delete h; }

}  // extern "C"
