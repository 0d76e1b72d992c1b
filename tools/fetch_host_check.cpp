// fetch_host_check.cpp - the host side of fetch_reads (csrc/fetch_host.h: the limits, the sorted list of canonical codes, the
// cutting of a stream into pieces at newlines, the reads files' records, the outputs' bytes) on fixed and random inputs, under the
// sanitizers. The per-read reduction is checked with a literal restatement of what fetch_kernels.hip does - a hit mask over the
// piece's positions, the reads' starts from the newlines, the popcount of a read's bit range and its first set bit - against a
// loop over every window of every read of the whole stream, piece by piece.
// build: g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include
//        -I kmersgwas_amd/csrc -I include tools/fetch_host_check.cpp -o tools/bin/fetch_host_check
// (a host-only program: run it on the CPU, on its own)
#include <unistd.h>

#include <cstring>
#include <fstream>
#include <iterator>
#include <random>
#include <tuple>

#include "fetch_host.h"

using namespace kgwas;
using namespace kgwas::fetch;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond);      \
            failures++;                                                    \
        }                                                                  \
    } while (0)

static bool has(const std::string& s, const char* part) { return s.find(part) != std::string::npos; }
static std::string slurp(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}
static bool exists(const std::string& path) { return access(path.c_str(), F_OK) == 0; }

template <class F>
static std::string refusal(int code, F&& f) {
    try {
        f();
    } catch (const Error& e) {
        return e.code == code ? e.what() : std::string("(another code) ") + e.what();
    }
    return "(not refused)";
}

static int base_code(uint8_t c) {
    c &= 0xDF;
    return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4;
}
// the code of the k bases at p, or false where one of them is no base
static bool window_code(const uint8_t* p, uint32_t k, uint64_t& a) {
    a = 0;
    for (uint32_t i = 0; i < k; i++) {
        const int c = base_code(p[i]);
        if (c > 3) return false;
        a = a << 2 | (uint64_t)c;
    }
    return true;
}
// the list search of the kernels: splitters, then the block behind the last splitter at or before the key
static bool lookup(const List& l, uint64_t a, uint32_t k, uint32_t& kmer, uint32_t& strand) {
    const uint64_t c = std::min(a, locate::revcomp_code(a, k));
    const uint64_t j = (uint64_t)(std::lower_bound(l.spl.begin(), l.spl.end(), c) - l.spl.begin());
    uint64_t i = 0;
    if (j) {
        const uint64_t lo = (j - 1) * l.B + 1, hi = std::min<uint64_t>(j * l.B, l.keys.size());
        i = (uint64_t)(std::lower_bound(l.keys.begin() + lo, l.keys.begin() + hi, c) - l.keys.begin());
    }
    if (i >= l.keys.size() || l.keys[i] != c) return false;
    kmer = l.ids[i] >> 1, strand = (uint32_t)(a != c) ^ (l.ids[i] & 1u);
    return true;
}

typedef std::tuple<uint64_t, uint32_t, uint32_t, uint32_t, uint32_t> Rec;  // read, n_hits, first_pos, kmer, strand

// what the kernels do with one piece: marks, starts, the reduction per read
static void piece_records(const uint8_t* p, uint64_t n, uint64_t n_reads, uint64_t read0, uint32_t k, uint32_t min_hits, const List& l, std::vector<Rec>& out,
                          std::vector<uint64_t>& kmer_windows) {
    std::vector<uint32_t> words((n + 31) / 32 + 1, 0), starts(1, 0);
    for (uint64_t q = 0; q + k <= n; q++) {
        uint64_t a;
        uint32_t kmer, strand;
        if (window_code(p + q, k, a) && lookup(l, a, k, kmer, strand)) words[q >> 5] |= 1u << (q & 31), kmer_windows[kmer]++;
    }
    for (uint64_t q = 0; q < n; q++)
        if (p[q] == '\n') starts.push_back((uint32_t)q + 1);
    CHECK(starts.size() == n_reads + 1 && starts.back() == n);
    for (uint64_t r = 0; r + 1 < starts.size(); r++) {
        const uint32_t lo = starts[r], next = starts[r + 1];
        if (next < lo + k + 1) continue;
        const uint32_t hi = next - k;
        uint32_t n_hits = 0, first = 0;
        for (uint32_t w = lo >> 5; w <= (hi - 1) >> 5; w++) {
            uint32_t x = words[w];
            if (w == lo >> 5) x &= 0xFFFFFFFFu << (lo & 31);
            if (w == (hi - 1) >> 5) x &= 0xFFFFFFFFu >> (31 - ((hi - 1) & 31));
            if (x && !n_hits) first = w * 32 + (uint32_t)__builtin_ctz(x);
            n_hits += (uint32_t)__builtin_popcount(x);
        }
        if (n_hits < min_hits) continue;
        uint64_t a;
        uint32_t kmer = ~0u, strand = 0;
        CHECK(window_code(p + first, k, a) && lookup(l, a, k, kmer, strand));
        out.emplace_back(read0 + r, n_hits, first - lo, kmer, strand);
    }
}

static void check_limits_and_list() {
    const uint64_t two[] = {0x06, 0x3F};  // ACG, TTT
    CHECK(has(refusal(KGWAS_ERR_ARG, [&] { build_list("x", two, 2, 0, 1); }), "1 to 31"));
    CHECK(has(refusal(KGWAS_ERR_ARG, [&] { build_list("x", two, 2, 32, 1); }), "1 to 31"));
    CHECK(has(refusal(KGWAS_ERR_ARG, [&] { build_list("x", two, 2, 3, 0); }), "min_hits must be at least 1"));
    CHECK(has(refusal(KGWAS_ERR_ARG, [&] { build_list("x", two, 0, 3, 1); }), "0 k-mers"));
    CHECK(has(refusal(KGWAS_ERR_ARG, [&] { build_list("x", two, locate::MAX_KMERS + 1, 3, 1); }), "1048577 k-mers"));
    CHECK(has(refusal(KGWAS_ERR_ARG, [&] { build_list("x", two, 2, 2, 1); }), "code 1 has bits"));
    const uint64_t same[] = {0x06, 0x1B};  // ACG and its reverse complement CGT
    CHECK(has(refusal(KGWAS_ERR_ARG, [&] { build_list("x", same, 2, 3, 1); }), "the queries 0 and 1 are the same k-mer"));
    const uint64_t three[] = {0x3F, 0x1B, 0x01};  // TTT (canonical AAA: reversed), CGT (canonical ACG: reversed), AAC (canonical)
    const List l = build_list("x", three, 3, 3, 1);
    CHECK(l.keys == (std::vector<uint64_t>{0x00, 0x01, 0x06}) && l.codes == l.keys && l.ids == (std::vector<uint32_t>{1, 4, 3}) && l.B == 1 && l.spl == l.keys);
    uint32_t kmer, strand;
    CHECK(lookup(l, 0x3F, 3, kmer, strand) && kmer == 0 && strand == 0 && lookup(l, 0x00, 3, kmer, strand) && kmer == 0 && strand == 1);
    CHECK(lookup(l, 0x06, 3, kmer, strand) && kmer == 1 && strand == 1 && lookup(l, 0x01, 3, kmer, strand) && kmer == 2 && strand == 0);
    CHECK(!lookup(l, 0x02, 3, kmer, strand));
    const uint64_t pal[] = {0x1B};  // ACGT, its own reverse complement: strand 0
    const List p = build_list("x", pal, 1, 4, 1);
    CHECK(lookup(p, 0x1B, 4, kmer, strand) && strand == 0 && p.ids[0] == 0);
}

static void check_cut_piece() {
    const uint8_t* s = reinterpret_cast<const uint8_t*>("AC\nGGT\n\nA");
    Cut c = cut_piece("x", s, 9, 100);
    CHECK(c.take == 9 && c.bytes == 10 && c.reads == 4 && c.add_newline && c.last);
    c = cut_piece("x", s, 8, 100);
    CHECK(c.take == 8 && c.bytes == 8 && c.reads == 3 && !c.add_newline && c.last);
    c = cut_piece("x", s, 9, 5);  // "AC\nGG": cut behind the first newline
    CHECK(c.take == 3 && c.bytes == 3 && c.reads == 1 && !c.last);
    c = cut_piece("x", s + 3, 6, 5);  // "GGT\n\n" of "GGT\n\nA"
    CHECK(c.take == 5 && c.reads == 2 && !c.last);
    c = cut_piece("x", s + 8, 1, 5);
    CHECK(c.take == 1 && c.bytes == 2 && c.reads == 1 && c.add_newline && c.last);
    c = cut_piece("x", s, 8, 8);  // exactly a piece
    CHECK(c.take == 8 && c.last && c.reads == 3);
    CHECK(has(refusal(KGWAS_ERR_ARG, [&] { cut_piece("x", s + 3, 6, 3); }), "a read of 3 bytes does not fit a piece of 3 bytes"));
    CHECK(has(refusal(KGWAS_ERR_ARG, [&] { cut_piece("x", reinterpret_cast<const uint8_t*>("ACGTACGT"), 8, 4); }), "a read of 8 bytes"));
    c = cut_piece("x", s, 0, 5);
    CHECK(c.take == 0 && c.bytes == 0 && c.reads == 0 && c.last);
}

// random streams: the pieces' reduction against a loop over every read and window of the whole stream
static void check_reduction() {
    std::mt19937_64 rng(5);
    for (int round = 0; round < 60; round++) {
        static const uint32_t ks[] = {1, 2, 3, 5, 16, 31};
        const uint32_t k = ks[round % 6], min_hits = 1 + (round / 6) % 3;
        const uint64_t n_kmers = round % 5 == 0 ? 5000 : 1 + rng() % 40;
        std::vector<uint64_t> f;
        std::unordered_set<uint64_t> seen;
        const uint64_t space = k < 32 ? (k == 31 ? ~0ull >> 2 : (1ull << (2 * k)) - 1) : 0;
        for (uint64_t tries = 0; f.size() < n_kmers && tries < 4 * n_kmers + 64; tries++) {
            const uint64_t c = rng() & space;
            if (seen.insert(std::min(c, locate::revcomp_code(c, k))).second) f.push_back(c);
        }
        const List l = build_list("x", f.data(), f.size(), k, min_hits);
        CHECK(l.spl.size() <= locate::MAX_SPLITTERS && std::is_sorted(l.keys.begin(), l.keys.end()));
        // a stream of reads of 0 .. 90 bytes over a small alphabet, with planted queries
        std::string s;
        const uint64_t len = 300 + rng() % 3000;
        while (s.size() < len) {
            const uint64_t rl = rng() % 91;
            for (uint64_t i = 0; i < rl; i++) s += "ACGTacgtNAC\r"[rng() % (k <= 5 ? 12 : 8)];
            if (k > 5 && rl >= k && rng() % 2) {
                uint64_t c = f[rng() % f.size()];
                if (rng() % 2) c = locate::revcomp_code(c, k);
                for (uint32_t i = 0; i < k; i++) s[s.size() - rl + i] = "ACGT"[(c >> (2 * (k - 1 - i))) & 3];
            }
            s += '\n';
        }
        if (round % 4 == 1) s.pop_back();  // no final newline
        // the whole stream, window by window
        std::vector<Rec> expect;
        std::vector<uint64_t> expect_windows(f.size(), 0);
        {
            uint64_t read = 0, lo = 0;
            const std::string t = s.back() == '\n' ? s : s + "\n";
            for (uint64_t q = 0; q < t.size(); q++) {
                if (t[q] != '\n') continue;
                uint32_t n_hits = 0, first = 0, fk = 0, fs = 0;
                for (uint64_t w = lo; w + k <= q; w++) {
                    uint64_t a;
                    uint32_t kmer, strand;
                    if (!window_code(reinterpret_cast<const uint8_t*>(t.data()) + w, k, a) || !lookup(l, a, k, kmer, strand)) continue;
                    expect_windows[kmer]++;
                    if (!n_hits++) first = (uint32_t)(w - lo), fk = kmer, fs = strand;
                }
                if (n_hits >= min_hits) expect.emplace_back(read, n_hits, first, fk, fs);
                read++, lo = q + 1;
            }
        }
        // piece by piece
        const uint64_t P = round % 2 ? 92 + rng() % 200 : 1u << 20;
        std::vector<Rec> got;
        std::vector<uint64_t> got_windows(f.size(), 0);
        uint64_t at = 0, read0 = 0;
        for (;;) {
            const Cut c = cut_piece("x", reinterpret_cast<const uint8_t*>(s.data()) + at, s.size() - at, std::min<uint64_t>(P, s.size() + 1));
            std::vector<uint8_t> piece(s.begin() + at, s.begin() + at + c.take);  // (its own allocation: reads past it are caught)
            if (c.add_newline) piece.push_back('\n');
            CHECK(piece.size() == c.bytes && c.bytes <= P && (c.bytes == 0 || piece.back() == '\n'));
            piece_records(piece.data(), piece.size(), c.reads, read0, k, min_hits, l, got, got_windows);
            at += c.take, read0 += c.reads;
            if (c.last) break;
        }
        CHECK(at == s.size());
        CHECK(got == expect);
        CHECK(got_windows == expect_windows);
        if (k > 5 && min_hits == 1) CHECK(!expect.empty());
    }
}

static std::vector<std::tuple<std::string, std::string>> records_of(const std::string& data, size_t block) {
    size_t at = 1;
    RecordReader rd("file", data.empty() ? 0 : data[0], [&](char* dst, size_t n) {
        const size_t m = std::min(n, data.size() - std::min(at, data.size()));
        memcpy(dst, data.data() + at, m);
        at += m;
        return m;
    }, block);
    std::vector<std::tuple<std::string, std::string>> out;
    Record r;
    while (rd.next(r)) out.emplace_back(std::string(r.raw, r.raw_len), std::string(r.seq, r.seq_len));
    return out;
}

static void check_reader() {
    typedef std::vector<std::tuple<std::string, std::string>> V;
    const std::string fq = "@a x\nACGT\n+\nIIII\n@b\r\nGG\r\n+b\r\nII\r\n@c\n\n+\n\n@d\nTT\n+\nII";
    const V fq_exp = {{"@a x\nACGT\n+\nIIII\n", "ACGT"}, {"@b\r\nGG\r\n+b\r\nII\r\n", "GG"}, {"@c\n\n+\n\n", ""}, {"@d\nTT\n+\nII", "TT"}};
    const std::string fa = ">a x\nAC\nGT\n>b\r\nGG\r\n\r\nT\r\n>c\n>d\nTT";
    const V fa_exp = {{">a x\nAC\nGT\n", "ACGT"}, {">b\r\nGG\r\n\r\nT\r\n", "GGT"}, {">c\n", ""}, {">d\nTT", "TT"}};
    for (size_t block : {1u, 2u, 3u, 5u, 7u, 16u, 1000u}) {
        CHECK(records_of(fq, block) == fq_exp);
        CHECK(records_of(fa, block) == fa_exp);
        CHECK(records_of(fq + "\n", block).size() == 4 && std::get<0>(records_of(fq + "\n", block)[3]) == "@d\nTT\n+\nII\n");
        CHECK(records_of("", block).empty());
        CHECK(has(refusal(KGWAS_ERR_FORMAT, [&] { records_of("@a\nAC\n+\n", block); }), "file: the last FASTQ record has fewer than four lines"));
        CHECK(has(refusal(KGWAS_ERR_FORMAT, [&] { records_of(fq + "\n\n", block); }), "fewer than four lines"));
        CHECK(has(refusal(KGWAS_ERR_FORMAT, [&] { records_of("@a\nAC\nx\nII\n", block); }), "does not have '@' and '+' at the head"));
        CHECK(has(refusal(KGWAS_ERR_FORMAT, [&] { records_of("@a\nAC\n+\nII\nb\nAC\n+\nII\n", block); }), "does not have '@' and '+' at the head"));
    }
}

static void check_outputs() {
    char dir[] = "/tmp/fetch_host_check_XXXXXX";
    if (!mkdtemp(dir)) abort();
    const std::string prefix = std::string(dir) + "/out";
    Queries queries;
    for (const char* w : {"AACGG", "CCCCC"}) {
        locate::Query q;
        q.text = w;
        queries.q.push_back(q);
    }
    auto record = [](const char* raw, const char* seq) {
        Record r;
        r.raw = raw, r.raw_len = strlen(raw), r.seq = seq, r.seq_len = strlen(seq);
        return r;
    };
    auto rec = [](uint64_t read, uint32_t n_hits, uint32_t first, uint32_t kmer, uint8_t strand) {
        kgwas_fetch_record r{};
        r.read = read, r.n_hits = n_hits, r.first_pos = first, r.kmer = kmer, r.strand = strand;
        return r;
    };
    {  // pairs, at most one unit per k-mer, two pieces
        Outputs o(prefix, '@', true, queries, 1);
        PieceMeta m;
        m.clear(10, 2);
        m.add(0, record("@p0 x\nTTAACGG\n+\nIIIIIII\n", "TTAACGG")), m.add(1, record("@p0/2\nGG\n+\nII\n", "GG"));
        m.add(0, record("@p1\nGG\n+\nII\n", "GG")), m.add(1, record("@p1/2\tz\nCCGTT\n+\nIIIII\n", "CCGTT"));
        m.add(0, record("@p2\nCCCCCC\n+\nIIIIII\n", "CCCCCC")), m.add(1, record("@p2/2\nAACGG\n+\nIIIII", "AACGG"));
        CHECK(m.units() == 3);
        const kgwas_fetch_record r0[] = {rec(10, 1, 2, 0, 0), rec(13, 1, 0, 0, 1), rec(14, 2, 0, 1, 0), rec(15, 1, 0, 0, 0)};
        o.add(m, r0, 4);
        m.clear(16, 2);
        m.add(0, record("@p3\nCCCCC\n+\nIIIII\n", "CCCCC")), m.add(1, record("@p3/2\nGG\n+\nII\n", "GG"));
        const kgwas_fetch_record r1[] = {rec(16, 1, 0, 1, 0)};
        o.add(m, r1, 1);
        CHECK(has(refusal(KGWAS_ERR_STATE, [&] { o.add(m, r1, 1); }), "out of order"));
        const kgwas_fetch_record bad[] = {rec(18, 1, 0, 1, 0)};
        CHECK(has(refusal(KGWAS_ERR_STATE, [&] { o.add(m, bad, 1); }), "out of order"));  // (no such unit)
        CHECK(o.reads_kept == 5 && o.reads_written == 3 && o.pairs_written == 2 && o.written == (std::vector<uint64_t>{1, 1}));
        o.commit("the log\n");
    }
    CHECK(slurp(prefix + "_1.fastq") == "@p0 x\nTTAACGG\n+\nIIIIIII\n@p2\nCCCCCC\n+\nIIIIII\n");
    CHECK(slurp(prefix + "_2.fastq") == "@p0/2\nGG\n+\nII\n@p2/2\nAACGG\n+\nIIIII\n");
    CHECK(slurp(prefix + ".reads.tsv") == "read\tmate\tn_hits\tfirst_pos\tkmer\tstrand\np0\t1\t1\t3\tAACGG\t+\np2\t1\t2\t1\tCCCCC\t+\np2/2\t2\t1\t1\tAACGG\t+\n");
    CHECK(slurp(prefix + ".log.txt") == "the log\n");
    for (const char* e : {"_1.fastq", "_2.fastq", ".reads.tsv", ".log.txt"}) unlink((prefix + e).c_str());
    {  // single FASTA, no limit, not committed: nothing is left
        Outputs o(prefix, '>', false, queries, 0);
        PieceMeta m;
        m.clear(0, 1);
        m.add(0, record(">s0\r\nAAC\r\nGG\r\n", "AACGG"));
        const kgwas_fetch_record r0[] = {rec(0, 1, 0, 0, 0)};
        o.add(m, r0, 1);
        CHECK(exists(prefix + ".fasta") && exists(prefix + ".reads.tsv") && o.reads_written == 1 && o.pairs_written == 0);
    }
    CHECK(!exists(prefix + ".fasta") && !exists(prefix + ".reads.tsv") && !exists(prefix + ".log.txt"));
    {
        Outputs o(prefix, '>', false, queries, 0);
        PieceMeta m;
        m.clear(0, 1);
        m.add(0, record(">s0\r\nAAC\r\nGG\r\n", "AACGG"));
        const kgwas_fetch_record r0[] = {rec(0, 1, 0, 0, 1)};
        o.add(m, r0, 1);
        o.commit("");
    }
    CHECK(slurp(prefix + ".fasta") == ">s0\r\nAAC\r\nGG\r\n" && slurp(prefix + ".reads.tsv") == "read\tmate\tn_hits\tfirst_pos\tkmer\tstrand\ns0\t0\t1\t1\tAACGG\t-\n");
    for (const char* e : {".fasta", ".reads.tsv", ".log.txt"}) unlink((prefix + e).c_str());
    CHECK(has(refusal(KGWAS_ERR_IO, [&] { Outputs o(std::string(dir) + "/absent/out", '@', true, queries, 0); }), "can't write"));
    rmdir(dir);
}

int main() {
    check_limits_and_list();
    check_cut_piece();
    check_reduction();
    check_reader();
    check_outputs();
    if (failures) {
        fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    printf("fetch_host_check: all checks passed\n");
    return 0;
}
