// proxy_host_check.cpp - the host side of proxy_kmers (csrc/proxy_host.h: the limits, the leads file in its two formats, the drain
// rounds, the per-lead buckets, the output lines) on fixed inputs, under the sanitizers. The drain rounds are checked against a
// literal restatement of what ld_proxy_write_kernel does with them: every record lands once, in order, inside the buffer.
// build: g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include
//        -I kmersgwas_amd/csrc tools/proxy_host_check.cpp -o tools/bin/proxy_host_check
// (a host-only program: run it on the CPU, on its own)
#include <unistd.h>

#include <cstring>
#include <random>

#include "proxy_host.h"

using namespace kgwas;
using namespace kgwas::proxy;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond);      \
            failures++;                                                    \
        }                                                                  \
    } while (0)

// two bits a base, no canonical form: all the parser needs of an encoder
static int encode(const char* w, uint64_t len, uint64_t* code) {
    uint64_t c = 0;
    for (uint64_t i = 0; i < len; i++) {
        const char* at = strchr("ACGT", w[i]);
        if (!at || !w[i]) return KGWAS_ERR_FORMAT;
        c = c << 2 | (uint64_t)(at - "ACGT");
    }
    *code = c;
    return KGWAS_OK;
}

static std::string temp_file(const std::string& text) {
    char name[] = "/tmp/proxy_host_check_XXXXXX";
    const int fd = mkstemp(name);
    if (fd < 0 || write(fd, text.data(), text.size()) != (ssize_t)text.size()) abort();
    close(fd);
    return name;
}

static std::string leads_of(const std::string& text, uint32_t k, std::string* refusal) {
    const std::string path = temp_file(text);
    std::string got;
    try {
        for (const Lead& l : read_leads(path, k, encode)) got += l.text + ",";
    } catch (const Error& e) {
        if (refusal) *refusal = e.what();
    }
    unlink(path.c_str());
    return got;
}
static bool has(const std::string& s, const char* part) { return s.find(part) != std::string::npos; }

static void check_limits() {
    for (const auto& bad : std::vector<std::vector<uint64_t>>{{0, 5, 1}, {4097, 5, 1}, {1, 0, 1}, {1, 8193, 1}, {1, 5, 0}, {1, 5, 1000001}}) {
        bool thrown = false;
        try {
            check_proxy_shape("x", bad[0], bad[1], (uint32_t)bad[2]);
        } catch (const Error& e) {
            thrown = e.code == KGWAS_ERR_ARG;
        }
        CHECK(thrown);
    }
    check_proxy_shape("x", 1, 1, 1);
    check_proxy_shape("x", 4096, 8192, 1000000);
}

static void check_leads() {
    std::string why;
    CHECK(leads_of("ACGTA\n\nCCCCC\r\nGGGGA", 5, &why) == "ACGTA,CCCCC,GGGGA," && why.empty());
    const std::string h = "rs\tp_lrt\tclump\tlead\tr2\tn1\tn11\n";
    // the file's lines are in the assoc file's order: the leads come out by clump number
    CHECK(leads_of(h + "AAAAC\t1e-3\t2\tAAAAC\t1.000000\t3\t3\nCCCCC\t1e-9\t1\tCCCCC\t1.000000\t4\t4\nAC\t1e-5\t1\tCCCCC\t0.9\t4\t3\nGGGGG\t1\t3\tGGGGG\tnan\t0\t0\n", 5, &why) ==
          "CCCCC,AAAAC,GGGGG," && why.empty());
    leads_of("ACGTA\nCCCCC\nACGTA\n", 5, &why);
    CHECK(has(why, "line 3: duplicate k-mer 'ACGTA' (the k-mer of line 1)"));
    leads_of("ACGTA\nCCCC\n", 5, &why);
    CHECK(has(why, "line 2: k-mer 'CCCC' has length 4, not 5"));
    leads_of("ACGTN\n", 5, &why);
    CHECK(has(why, "line 1: k-mer 'ACGTN' has a letter other than A, C, G, T"));
    leads_of("ACGTA 3\n", 5, &why);
    CHECK(has(why, "line 1: 2 fields: a list of leads has one k-mer per line"));
    leads_of(h + "AAAAC\t1e-3\t2\n", 5, &why);
    CHECK(has(why, "line 2: 3 fields, a clump_kmers line has 7"));
    leads_of(h + "AAAAC\t1e-3\tx\tAAAAC\t1.000000\t3\t3\n", 5, &why);
    CHECK(has(why, "line 2: clump 'x' is not a number"));
    leads_of(h, 5, &why);
    CHECK(has(why, "no lead k-mer"));
    why.clear();
    leads_of("", 5, &why);
    CHECK(has(why, "no lead k-mer"));
    bool thrown = false;
    try {
        read_leads("/nonexistent/proxy_host_check", 5, encode);
    } catch (const Error& e) {
        thrown = e.code == KGWAS_ERR_IO;
    }
    CHECK(thrown);
}

// rows with cnt[r] records each, blocks of 256 rows; what the write kernel does per round, into a buffer of exactly cap records
static void check_rounds(uint32_t R, uint32_t cap, uint32_t max_per_row, uint64_t seed) {
    std::mt19937_64 rng(seed);
    std::vector<uint32_t> cnt(R);
    for (uint32_t& c : cnt) c = (rng() % 3 == 0) ? (uint32_t)(rng() % (max_per_row + 1)) : 0;
    const uint32_t n_blocks = (R + 255) / 256;
    std::vector<uint32_t> boff(n_blocks + 1, 0);
    for (uint32_t r = 0; r < R; r++) boff[r / 256 + 1] += cnt[r];
    for (uint32_t b = 0; b < n_blocks; b++) boff[b + 1] += boff[b];
    std::vector<uint64_t> all;  // record number -> row * 2^16 + its place in the row, in order
    uint64_t expect_rounds = ((uint64_t)boff[n_blocks] + cap - 1) / cap;
    const std::vector<Round> rounds = drain_rounds(boff.data(), n_blocks, cap);
    CHECK(rounds.size() == expect_rounds);
    for (const Round& rd : rounds) {
        CHECK(rd.hi > rd.lo && rd.hi - rd.lo <= cap && rd.blk0 <= rd.blk1 && rd.blk1 <= n_blocks);
        std::vector<uint64_t> buf(cap, ~0ull);  // exactly the buffer: a store past it is a store past the allocation
        for (uint32_t blk = rd.blk0; blk < rd.blk1; blk++) {
            uint32_t at = boff[blk];
            for (uint32_t r = blk * 256; r < std::min(R, blk * 256 + 256); r++)
                for (uint32_t k = 0; k < cnt[r]; k++, at++)
                    if (at >= rd.lo && at - rd.lo < cap) buf[at - rd.lo] = (uint64_t)r << 16 | k;
        }
        for (uint32_t i = 0; i < rd.hi - rd.lo; i++) {
            CHECK(buf[i] != ~0ull);  // (a record of the window that no block of [blk0, blk1) holds)
            all.push_back(buf[i]);
        }
    }
    CHECK(all.size() == boff[n_blocks]);
    size_t i = 0;
    for (uint32_t r = 0; r < R; r++)
        for (uint32_t k = 0; k < cnt[r]; k++, i++) CHECK(i < all.size() && all[i] == ((uint64_t)r << 16 | k));
}

static void check_buckets_and_lines() {
    Buckets b(3, 2);
    const kgwas_proxy_record recs[] = {{0, 9, 0, 4, 4, 0}, {0, 9, 2, 4, 1, 0}, {3, 7, 0, 4, 0, 0}, {5, 6, 0, 3, 3, 0}, {5, 6, 1, 3, 2, 0}};
    b.add(recs, 2);
    b.add(recs + 2, 3);
    CHECK(b.total == 5 && b.found[0] == 3 && b.found[1] == 1 && b.found[2] == 1 && b.kept[0].size() == 2 && b.kept[0][1].row == 3 && b.kept[1][0].row == 5);
    for (const kgwas_proxy_record& bad : {kgwas_proxy_record{5, 6, 1, 3, 2, 0}, kgwas_proxy_record{4, 6, 2, 3, 2, 0}, kgwas_proxy_record{9, 6, 3, 3, 2, 0}}) {
        bool thrown = false;
        try {
            b.add(&bad, 1);
        } catch (const Error&) {
            thrown = true;
        }
        CHECK(thrown);
    }
    std::string text = header_line();
    append_line(text, "ACGTA", 5, 8, 4, kgwas_proxy_record{0, 0x1B, 0, 4, 4, 0});    // the lead's own row
    append_line(text, "ACGTA", 5, 8, 4, kgwas_proxy_record{3, 0x1B1, 0, 4, 0, 0});   // its complement
    append_line(text, "ACGTA", 5, 8, 4, kgwas_proxy_record{12, 0x3FF, 0, 4, 3, 0});  // r2 = 0.25
    CHECK(text == "lead\tkmer\tr2\tphase\tn1\tn11\trow\nACGTA\tAACGT\t1.000000\t+\t4\t4\t0\nACGTA\tCGTAC\t1.000000\t-\t4\t0\t3\nACGTA\tTTTTT\t0.250000\t+\t4\t3\t12\n");
    CHECK(kmer_letters(3, 31) == std::string(30, 'A') + "T");
}

int main() {
    check_limits();
    check_leads();
    check_rounds(1, 1, 1, 1);
    check_rounds(300, 7, 130, 2);
    check_rounds(1000, 1000, 130, 3);
    check_rounds(1000, 1, 3, 4);
    check_rounds(700, 100000, 4096, 5);
    check_rounds(513, 4097, 4096, 6);
    check_rounds(256, 33, 0, 7);
    check_buckets_and_lines();
    printf(failures ? "proxy_host_check: %d check(s) FAILED\n" : "proxy_host_check: all checks passed\n", failures);
    return failures ? 1 : 0;
}
