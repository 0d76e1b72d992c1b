// clump_host_check.cpp - the host side of clump_kmers (csrc/clump_host.h and what it takes from csrc/ld_host.h: the threshold's text,
// the assoc parser, the p order, the placement of the hits' rows, the streaming clump pass, the output lines) on fixed inputs, under
// the sanitizers. The link matrix the clump pass consumes is made here with a literal restatement of the predicate and handed over
// in blocks of several sizes, pitches wider than the rows included, as the device hands it over; the result is compared with a
// whole-matrix greedy pass.
// build: g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include
//        -I kmersgwas_amd/csrc tools/clump_host_check.cpp -o tools/bin/clump_host_check
// (a host-only program: run it on the CPU, on its own)
#include <unistd.h>

#include <cstring>
#include <random>

#include "clump_host.h"

using namespace kgwas;
using namespace kgwas::clump;

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
    char name[] = "/tmp/clump_host_check_XXXXXX";
    const int fd = mkstemp(name);
    if (fd < 0 || write(fd, text.data(), text.size()) != (ssize_t)text.size()) abort();
    close(fd);
    return name;
}

static std::string refusal(const std::string& text, uint32_t k) {
    const std::string path = temp_file(text);
    std::string msg;
    try {
        read_assoc(path, k, encode);
    } catch (const Error& e) {
        msg = e.what();
    }
    unlink(path.c_str());
    return msg;
}
static bool has(const std::string& s, const char* part) { return s.find(part) != std::string::npos; }

static void check_threshold() {
    CHECK(r2_millionths("0.8") == 800000 && r2_millionths("1") == 1000000 && r2_millionths("1.000000") == 1000000);
    CHECK(r2_millionths("0.000001") == 1 && r2_millionths(".25") == 250000 && r2_millionths("0.3") == 300000 && r2_millionths("1.") == 1000000);
    for (const char* bad : {"0", "1.0000001", "0.1234567", "abc", "", ".", "-0.5", "1e-1", "2", "0.0", " 0.5", "0.5 ", "1000000"}) {
        bool thrown = false;
        try {
            r2_millionths(bad);
        } catch (const Error&) {
            thrown = true;
        }
        CHECK(thrown);
    }
}

static void check_parser() {
    const std::string h9 = "chr\trs\tps\tn_miss\tallele1\tallele0\taf\tl_mle\tp_lrt\n";
    const std::string h14 = "chr\trs\tps\tn_miss\tallele1\tallele0\taf\tbeta\tse\tl_remle\tl_mle\tp_wald\tp_lrt\tp_score\n";
    {
        const std::string path = temp_file(h9 + "0\tACGTA\t0\t0\t0\t1\t0.3\t1.0\t3e-5\n\n0\tCCCCC\t0\t0\t0\t1\t0.3\t1.0\t1.000000e-09\r\n0\tGGGGG\t0\t0\t0\t1\t0.3\t1.0\t3e-5");
        const std::vector<Hit> hits = read_assoc(path, 5, encode);
        unlink(path.c_str());
        CHECK(hits.size() == 3 && hits[0].rs == "ACGTA" && hits[1].p_text == "1.000000e-09" && hits[2].p == 3e-5 && hits[2].line == 2);
        const std::vector<uint32_t> all = p_order(hits, std::numeric_limits<double>::infinity());
        CHECK(all.size() == 3 && all[0] == 1 && all[1] == 0 && all[2] == 2);  // the tie keeps the file's order
        CHECK(p_order(hits, 1e-9).size() == 1 && p_order(hits, 1e-10).empty() && p_order(hits, 3e-5).size() == 3);
    }
    {
        const std::string path = temp_file(h14 + "0\tACGTA\t0\t0\t0\t1\t0.3\t0.1\t0.2\t1.0\t1.0\t0.5\t0.25\t0.75\n");
        const std::vector<Hit> hits = read_assoc(path, 5, encode);
        unlink(path.c_str());
        CHECK(hits.size() == 1 && hits[0].p == 0.25 && hits[0].p_text == "0.25");
    }
    CHECK(has(refusal("chr\trs\tp_wald\n0\tACGTA\t0.5\n", 5), "no column 'p_lrt'"));
    CHECK(has(refusal("chr\tsnp\tp_lrt\n0\tACGTA\t0.5\n", 5), "no column 'rs'"));
    CHECK(has(refusal("", 5), "no column 'rs'"));
    CHECK(has(refusal(h9 + "0\tACGT\t0\t0\t0\t1\t0.3\t1.0\t3e-5\n", 5), "line 2: k-mer 'ACGT' has length 4, not 5"));
    CHECK(has(refusal(h9 + "0\tACGTN\t0\t0\t0\t1\t0.3\t1.0\t3e-5\n", 5), "has a letter other than A, C, G, T"));
    CHECK(has(refusal(h9 + "0\tACGTA\t0\t0\t0\t1\t0.3\t1.0\t3e-5\n0\tACGTA\t0\t0\t0\t1\t0.3\t1.0\t3e-5\n", 5), "line 3: duplicate k-mer 'ACGTA' (the k-mer of line 2)"));
    CHECK(has(refusal(h9 + "0\tACGTA\t0\t0\n", 5), "line 2: too few fields (4, the header has 9)"));
    CHECK(has(refusal(h9 + "0\tACGTA\t0\t0\t0\t1\t0.3\t1.0\tNA\n", 5), "p_lrt 'NA' is not a number"));
    CHECK(has(refusal(h9 + "0\tACGTA\t0\t0\t0\t1\t0.3\t1.0\tnan\n", 5), "p_lrt 'nan' is not a number"));
    CHECK(has(refusal(h9 + "0\tACGTA\t0\t0\t0\t1\t0.3\t1.0\t1e-5x\n", 5), "is not a number"));
    bool thrown = false;
    try {
        read_assoc("/nonexistent/clump_host_check", 5, encode);
    } catch (const Error& e) {
        thrown = e.code == KGWAS_ERR_IO;
    }
    CHECK(thrown);
}

static bool linked(uint64_t n, uint64_t ca, uint64_t cb, uint64_t n11, uint64_t tm) {
    const int64_t d = (int64_t)(n * n11) - (int64_t)(ca * cb);
    const unsigned __int128 num = (unsigned __int128)(uint64_t)(d * d) * 1000000u, den = (unsigned __int128)(ca * (n - ca) * cb * (n - cb));
    return den != 0 && num >= den * tm;
}

static void check_clumper(uint64_t N, uint64_t n, uint64_t tm, uint64_t seed) {
    const uint64_t W = (n + 63) / 64, n_dw = (N + 31) / 32;
    std::mt19937_64 rng(seed);
    std::vector<uint64_t> rows(N * W, 0), mask(W, ~0ull);
    if (n % 64) mask[W - 1] = (1ull << (n % 64)) - 1;
    for (uint64_t r = 0; r < N; r++)
        for (uint64_t w = 0; w < W; w++) {
            // families of four rows that differ in a few bits; every fifth family constant
            const uint64_t fam = r / 4, base = (fam % 5 == 4) ? 0ull : std::mt19937_64(seed * 1000 + fam * 64 + w)();
            rows[r * W + w] = (base ^ ((rng() & rng() & rng() & rng()) * (r % 4 != 0))) & mask[w];
        }
    std::vector<uint32_t> n1(N);
    for (uint64_t r = 0; r < N; r++) n1[r] = count_and(&rows[r * W], &rows[r * W], mask.data(), W);
    std::vector<uint32_t> adj(N * n_dw, 0);
    uint64_t pairs = 0;
    for (uint64_t a = 0; a < N; a++)
        for (uint64_t b = a + 1; b < N; b++)
            if (linked(n, n1[a], n1[b], count_and(&rows[a * W], &rows[b * W], mask.data(), W), tm)) adj[a * n_dw + b / 32] |= 1u << (b % 32), pairs++;
    // the whole-matrix greedy pass
    std::vector<uint32_t> want(N, Clumper::NONE), want_leads;
    for (uint64_t a = 0; a < N; a++) {
        if (want[a] != Clumper::NONE) continue;
        want[a] = (uint32_t)a;
        want_leads.push_back((uint32_t)a);
        for (uint64_t b = a + 1; b < N; b++)
            if (want[b] == Clumper::NONE && (adj[a * n_dw + b / 32] >> (b % 32) & 1)) want[b] = (uint32_t)a;
    }
    for (uint64_t tile : {(uint64_t)1, (uint64_t)7, (uint64_t)64, N}) {
        const uint64_t pitch = n_dw + (tile % 3);  // (a pitch wider than the rows: the device's is padded to 16 bytes)
        Clumper cl(N);
        for (uint64_t row0 = 0; row0 < N; row0 += tile) {
            const uint64_t nr = std::min(tile, N - row0);
            std::vector<uint32_t> blk(nr * pitch, 0xFFFFFFFFu);  // exactly the block: a read past it is a read past the allocation
            for (uint64_t r = 0; r < nr; r++) memcpy(&blk[r * pitch], &adj[(row0 + r) * n_dw], n_dw * 4);
            cl.block(row0, nr, blk.data(), pitch);
        }
        CHECK(cl.lead_of == want && cl.leads == want_leads && cl.pairs == pairs && cl.next_row == N);
    }
    bool thrown = false;
    try {
        Clumper cl(N);
        cl.block(1, 1, adj.data(), n_dw);
    } catch (const Error&) {
        thrown = true;
    }
    CHECK(thrown);
    // the output lines
    Hit a, b;
    a.rs = "AAAAA", a.p_text = "1e-9", b.rs = "CCCCC", b.p_text = "0.5";
    std::string text = header_line();
    append_line(text, a, 1, a, true, 8, 4, 4, 4);
    append_line(text, b, 1, a, false, 8, 4, 4, 3);
    append_line(text, b, 2, b, true, 8, 0, 0, 0);
    CHECK(text == "rs\tp_lrt\tclump\tlead\tr2\tn1\tn11\nAAAAA\t1e-9\t1\tAAAAA\t1.000000\t4\t4\nCCCCC\t0.5\t1\tAAAAA\t0.250000\t4\t3\nCCCCC\t0.5\t2\tCCCCC\tnan\t0\t0\n");
    CHECK(r2_of(8192, 4096, 4096, 3072) == 0.25 && std::isnan(r2_of(8, 8, 4, 4)));
}

// the rows of a list of codes from what the table's search found (ld_host.h, place_rows): the list in shuffled order, a key the
// table holds twice (its first row is taken), a code the table lacks (its place comes back)
static void check_placement() {
    const uint64_t stride = 3;
    std::vector<uint64_t> found;  // table order: keys 10, 20, 20, 30, 40, 50; words 1 and 2 of a row say which row it is
    const uint64_t keys[] = {10, 20, 20, 30, 40, 50};
    for (uint64_t i = 0; i < 6; i++) found.insert(found.end(), {keys[i], 100 + i, 200 + i});
    const std::vector<uint64_t> codes = {40, 10, 50, 20, 30};
    const PlacedRows all = place_rows(codes.data(), codes.size(), found.data(), 6, stride);
    CHECK(all.missing == PlacedRows::NONE && all.rows.size() == codes.size() * stride);
    const uint64_t from[] = {4, 0, 5, 1, 3};  // (key 20: row 1, not row 2)
    for (size_t i = 0; i < codes.size(); i++)
        CHECK(all.rows[i * stride] == codes[i] && all.rows[i * stride + 1] == 100 + from[i] && all.rows[i * stride + 2] == 200 + from[i]);
    // a list with two codes the table lacks: the first one's place; a found row of a key nobody asked for is passed over
    const std::vector<uint64_t> some = {30, 7, 10, 8};
    const PlacedRows part = place_rows(some.data(), some.size(), found.data(), 6, stride);
    CHECK(part.missing == 1 && part.rows.size() == some.size() * stride && part.rows[0] == 30 && part.rows[2 * stride + 1] == 100);
    // nothing found, nothing asked for
    CHECK(place_rows(some.data(), some.size(), nullptr, 0, stride).missing == 0);
    const PlacedRows none = place_rows(nullptr, 0, found.data(), 6, stride);
    CHECK(none.missing == PlacedRows::NONE && none.rows.empty());
    // exactly the arrays: a read past them is a read past the allocation
    const std::vector<uint64_t> one_found = {10, 1, 2}, one_code = {10};
    CHECK(place_rows(one_code.data(), 1, one_found.data(), 1, stride).rows == one_found);
}

int main() {
    check_threshold();
    check_parser();
    check_placement();
    check_clumper(1, 5, 800000, 1);
    check_clumper(33, 67, 800000, 2);
    check_clumper(130, 128, 250000, 3);
    check_clumper(300, 1135, 1000000, 4);
    check_clumper(97, 64, 1, 5);
    printf(failures ? "clump_host_check: %d check(s) FAILED\n" : "clump_host_check: all checks passed\n", failures);
    return failures ? 1 : 0;
}
