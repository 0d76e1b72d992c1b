// locate_host_check.cpp - the host side of locate_kmers (csrc/locate_host.h: the limits, the pattern lists, the FASTA reader, the
// --kmers file in its three formats, the buckets, the output lines) on fixed inputs, under the sanitizers. The lists are checked
// with a literal restatement of what locate_kernels.hip does with them - the splitter search, the walk along equal half keys, the
// merge of the two walks - against a loop over every window and pattern: every hit once, in (pos, kmer, strand) order.
// build: g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include
//        -I kmersgwas_amd/csrc tools/locate_host_check.cpp -o tools/bin/locate_host_check
// (a host-only program: run it on the CPU, on its own)
#include <unistd.h>

#include <cstring>
#include <random>
#include <tuple>

#include "locate_host.h"

using namespace kgwas;
using namespace kgwas::locate;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond);      \
            failures++;                                                    \
        }                                                                  \
    } while (0)

static std::string temp_file(const std::string& text) {
    char name[] = "/tmp/locate_host_check_XXXXXX";
    const int fd = mkstemp(name);
    if (fd < 0 || write(fd, text.data(), text.size()) != (ssize_t)text.size()) abort();
    close(fd);
    return name;
}
static bool has(const std::string& s, const char* part) { return s.find(part) != std::string::npos; }

template <class F>
static std::string refusal(int code, F&& f) {
    try {
        f();
    } catch (const Error& e) {
        return e.code == code ? e.what() : std::string("(another code) ") + e.what();
    }
    return "(not refused)";
}

static void check_limits_and_lists() {
    const uint64_t two[] = {0x06, 0x3F};  // ACG, TTT
    CHECK(has(refusal(KGWAS_ERR_ARG, [&] { build_lists("x", two, 2, 0, 0); }), "1 to 31"));
    CHECK(has(refusal(KGWAS_ERR_ARG, [&] { build_lists("x", two, 2, 32, 0); }), "1 to 31"));
    CHECK(has(refusal(KGWAS_ERR_ARG, [&] { build_lists("x", two, 2, 3, 2); }), "0 or 1"));
    CHECK(has(refusal(KGWAS_ERR_ARG, [&] { build_lists("x", two, 2, 1, 1); }), "at least 2"));
    CHECK(has(refusal(KGWAS_ERR_ARG, [&] { build_lists("x", two, 0, 3, 1); }), "0 k-mers"));
    CHECK(has(refusal(KGWAS_ERR_ARG, [&] { build_lists("x", two, MAX_KMERS + 1, 3, 1); }), "1048577 k-mers"));
    CHECK(has(refusal(KGWAS_ERR_ARG, [&] { build_lists("x", two, 2, 2, 1); }), "code 1 has bits"));
    const uint64_t same[] = {0x06, 0x1B};  // ACG and its reverse complement CGT
    CHECK(has(refusal(KGWAS_ERR_ARG, [&] { build_lists("x", same, 2, 3, 1); }), "the queries 0 and 1 are the same k-mer"));
    CHECK(revcomp_code(0x06, 3) == 0x1B && revcomp_code(0x1B, 4) == 0x1B && revcomp_code(0, 31) == (1ull << 62) - 1);
    const uint64_t pal[] = {0x1B, 0x00};  // ACGT (its own reverse complement), AAAA
    const Lists l = build_lists("x", pal, 2, 4, 1);
    CHECK(l.H.keys.size() == 3 && l.L.keys.size() == 3 && l.H.ids == (std::vector<uint32_t>{2, 0, 3}) && l.H.keys == (std::vector<uint64_t>{0, 1, 15}));
    CHECK(l.L.ids == (std::vector<uint32_t>{2, 0, 3}) && l.L.keys == (std::vector<uint64_t>{0, 11, 15}) && l.H.B == 1 && l.H.spl == l.H.keys);
}

// sorted_search.h's fk_bound<false> and fk_list_bound<false>, restated
static uint64_t lower(const uint64_t* a, uint64_t lo, uint64_t hi, uint64_t x) {
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}
static uint64_t list_lower(const List& l, uint64_t x) {
    const uint64_t j = lower(l.spl.data(), 0, l.spl.size(), x), n = l.keys.size();
    if (j == 0) return 0;
    return lower(l.keys.data(), (j - 1) * l.B + 1, std::min(j * l.B, n), x);
}
typedef std::tuple<uint64_t, uint32_t, uint32_t, uint32_t> Rec;  // pos, id, h, offset
struct Walk {
    const List& l;
    uint64_t i, key;
    uint32_t id = 0, h = 0, off = 0;
    Walk(const List& list, uint64_t k) : l(list), i(list_lower(list, k)), key(k) {}
    bool next(uint64_t a, uint32_t k, uint32_t hh, bool second) {
        while (i < l.keys.size() && l.keys[i] == key) {
            const uint64_t x = a ^ l.codes[i], y = (x | (x >> 1)) & 0x5555555555555555ull;
            const uint32_t hm = (uint32_t)__builtin_popcountll(y);
            id = l.ids[i++];
            const uint32_t at = hm ? k - 1 - (63 - (uint32_t)__builtin_clzll(y)) / 2 : 0;
            if (second ? (hm == 1 && at < hh) : hm <= 1) {
                h = hm, off = hm ? at + 1 : 0;
                return true;
            }
        }
        return false;
    }
};
static void window_hits(uint64_t pos, uint64_t a, uint32_t k, uint32_t d, const Lists& ls, std::vector<Rec>& out) {
    const uint32_t hh = (k + 1) / 2, lh = k / 2;
    Walk wh(ls.H, d ? a >> (2 * lh) : a);
    bool has_h = wh.next(a, k, hh, false);
    if (!d) {
        for (; has_h; has_h = wh.next(a, k, hh, false)) out.emplace_back(pos, wh.id, wh.h, wh.off);
        return;
    }
    Walk wl(ls.L, a & ((1ull << (2 * lh)) - 1));
    bool has_l = wl.next(a, k, hh, true);
    while (has_h || has_l) {
        if (has_h && (!has_l || wh.id < wl.id)) {
            out.emplace_back(pos, wh.id, wh.h, wh.off);
            has_h = wh.next(a, k, hh, false);
        } else {
            out.emplace_back(pos, wl.id, wl.h, wl.off);
            has_l = wl.next(a, k, hh, true);
        }
    }
}

static void check_search(uint32_t k, uint32_t d, uint32_t n_queries, uint32_t letters, uint64_t seed) {
    std::mt19937_64 rng(seed);
    const std::string alphabet = std::string("ACGT").substr(0, letters) + "acN\n";
    std::string stream(3000, 'A');
    for (char& c : stream) c = rng() % 50 ? alphabet[rng() % letters] : alphabet[rng() % alphabet.size()];
    // the queries: windows of the stream, as they are, with one base changed, reverse-complemented; and random ones
    std::vector<uint64_t> f;
    std::unordered_set<uint64_t> canon;
    auto code_at = [&](size_t p, uint64_t& a) {
        a = 0;
        for (uint32_t j = 0; j < k; j++) {
            const char* at = strchr("ACGT", stream[p + j] & 0xDF);
            if (!at || !stream[p + j]) return false;
            a = a << 2 | (uint64_t)(at - "ACGT");
        }
        return true;
    };
    for (uint32_t t = 0; f.size() < n_queries && t < 100 * n_queries; t++) {
        uint64_t a;
        if (t % 4 == 3)
            a = rng() & ((1ull << (2 * k)) - 1);
        else if (!code_at(rng() % (stream.size() - k), a))
            continue;
        if (t % 4 == 1) a ^= (1 + rng() % 3) << (2 * (rng() % k));
        if (t % 4 == 2) a = revcomp_code(a, k);
        if (canon.insert(std::min(a, revcomp_code(a, k))).second) f.push_back(a);
    }
    const Lists ls = build_lists("check", f.data(), f.size(), k, d);
    std::vector<Rec> got, want;
    for (size_t p = 0; p + k <= stream.size(); p++) {
        uint64_t a;
        if (!code_at(p, a)) continue;
        window_hits(p, a, k, d, ls, got);
        for (uint32_t i = 0; i < f.size(); i++)
            for (uint32_t s = 0; s < 2; s++) {
                const uint64_t pat = s ? revcomp_code(f[i], k) : f[i];
                if (s && pat == f[i]) continue;
                uint32_t h = 0, off = 0;
                for (uint32_t j = 0; j < k; j++)
                    if (((a >> (2 * (k - 1 - j))) & 3) != ((pat >> (2 * (k - 1 - j))) & 3)) {
                        if (!h) off = j + 1;
                        h++;
                    }
                if (h <= d) want.emplace_back(p, i << 1 | s, h, off);
            }
    }
    CHECK(got == want);
    CHECK(!want.empty());
}

static std::string parse(const std::string& data, size_t block, std::vector<Contig>& contigs) {
    std::string stream;
    FastaParser p("ref.fa", [&](const char* q, size_t n) { stream.append(q, n); });
    for (size_t i = 0; i < data.size(); i += block) p.feed(data.data() + i, std::min(block, data.size() - i));
    p.finish();
    contigs = p.contigs;
    CHECK(p.stream_bytes == stream.size());
    return stream;
}

static void check_fasta() {
    const std::string data = ">one first contig\r\nACGT\r\nAC\n>two\tx\nNN\rNN\n>three\n\n>four\nacgtn\r";
    for (size_t block : {(size_t)1, (size_t)2, (size_t)3, (size_t)7, (size_t)1000}) {
        std::vector<Contig> c;
        const std::string s = parse(data, block, c);
        CHECK(s == "ACGTAC\nNN\rNN\n\nacgtn");
        CHECK(c.size() == 4 && c[0].name == "one" && c[1].name == "two" && c[2].name == "three" && c[3].name == "four");
        CHECK(c.size() == 4 && c[0].start == 0 && c[0].length == 6 && c[1].start == 7 && c[1].length == 5 && c[2].start == 13 && c[2].length == 0 &&
              c[3].start == 14 && c[3].length == 5);
        CHECK(c.size() == 4 && &contig_of(c, 0) == &c[0] && &contig_of(c, 5) == &c[0] && &contig_of(c, 7) == &c[1] && &contig_of(c, 18) == &c[3]);
        CHECK(has(refusal(KGWAS_ERR_STATE, [&] { contig_of(c, 6); }), "outside every contig"));
        CHECK(has(refusal(KGWAS_ERR_STATE, [&] { contig_of(c, 13); }), "outside every contig"));
        CHECK(has(refusal(KGWAS_ERR_STATE, [&] { contig_of(c, 19); }), "outside every contig"));
        std::vector<Contig> x;
        CHECK(has(refusal(KGWAS_ERR_FORMAT, [&] { parse("", block, x); }), "ref.fa: not FASTA"));
        CHECK(has(refusal(KGWAS_ERR_FORMAT, [&] { parse("ACGT\n", block, x); }), "ref.fa: not FASTA"));
        CHECK(has(refusal(KGWAS_ERR_FORMAT, [&] { parse(">a\n>b\n", block, x); }), "ref.fa: no sequence"));
        CHECK(has(refusal(KGWAS_ERR_FORMAT, [&] { parse(">a\nAC\n> x\nAC\n", block, x); }), "ref.fa line 3: a contig without a name"));
        CHECK(has(refusal(KGWAS_ERR_FORMAT, [&] { parse(">a\nAC\n>b\nAC\n>a 2\nAC", block, x); }), "ref.fa line 5: the contig 'a' is given twice"));
        CHECK(has(refusal(KGWAS_ERR_FORMAT, [&] { parse(">a", block, x); }), "ref.fa: no sequence"));
    }
}

static std::string queries_of(const std::string& text, uint32_t k, std::string* why) {
    const std::string path = temp_file(text);
    std::string got;
    why->clear();
    try {
        const Queries q = read_queries(path, k);
        for (const Query& x : q.q) got += x.text + (q.has_p ? ":" + x.p_text : "") + ",";
    } catch (const Error& e) {
        *why = e.what();
    }
    unlink(path.c_str());
    return got;
}

static void check_queries() {
    std::string why;
    CHECK(queries_of("ACG\n\nTTT\r\nCCC", 3, &why) == "ACG,TTT,CCC," && why.empty());
    const std::string assoc = "chr\trs\tps\tn_miss\tallele1\tallele0\taf\tl_mle\tp_lrt\n";
    CHECK(queries_of(assoc + "0\tACG\t0\t0\t0\t1\t0.3\t1.0\t1e-9\n0\tTTT\t0\t0\t0\t1\t0.3\t1.0\t2e-5\n", 3, &why) == "ACG:1e-9,TTT:2e-5," && why.empty());
    CHECK(queries_of("rs\tp_lrt\tclump\tlead\tr2\tn1\tn11\nACG\t1e-3\t1\tACG\t1.000000\t3\t3\nCCC\t1\t1\tACG\t0.9\t3\t3\n", 3, &why) == "ACG:1e-3,CCC:1," && why.empty());
    const std::string proxies = "lead\tkmer\tr2\tphase\tn1\tn11\trow\n";
    CHECK(queries_of(proxies + "ACG\tTTT\t1.0\t+\t3\t3\t0\nACG\tAAA\t1.0\t+\t3\t3\t1\nCCC\tTTT\t1.0\t+\t3\t3\t0\nCCC\tACC\t1.0\t+\t3\t3\t4\n", 3, &why) == "TTT,ACC," && why.empty());
    queries_of("ACG\nCGT\n", 3, &why);
    CHECK(has(why, "line 2: duplicate k-mer 'CGT' (the k-mer of line 1)"));
    queries_of(assoc + "0\tACG\t0\t0\t0\t1\t0.3\t1.0\t1e-9\n0\tACG\t0\t0\t0\t1\t0.3\t1.0\t1e-9\n", 3, &why);
    CHECK(has(why, "line 3: duplicate k-mer 'ACG' (the k-mer of line 2)"));
    queries_of("ACGT\n", 3, &why);
    CHECK(has(why, "line 1: k-mer 'ACGT' has length 4, not 3"));
    queries_of("ACN\n", 3, &why);
    CHECK(has(why, "line 1: k-mer 'ACN' has a letter other than A, C, G, T"));
    queries_of("ACG 1\n", 3, &why);
    CHECK(has(why, "line 1: 2 fields: a list of k-mers has one k-mer per line"));
    queries_of(assoc + "0\tACC\n", 3, &why);
    CHECK(has(why, "line 2: too few fields (2, the header has 9)"));
    for (const std::string& empty : {std::string(), std::string("\n\n"), assoc, proxies}) {
        queries_of(empty, 3, &why);
        CHECK(has(why, "no k-mer"));
    }
    CHECK(has(refusal(KGWAS_ERR_IO, [&] { read_queries("/nonexistent/locate_host_check", 3); }), "can't open k-mers file"));
}

static void check_buckets_and_lines() {
    //                          0123456789A
    const std::string stream = "AAAGGTCAAAA";
    auto ref_at = [&](uint64_t p) { return (uint8_t)stream.at(p); };
    Buckets b(2, 2, 5);
    const kgwas_locate_record recs[] = {{0, 1, 0, 0, 0, 0}, {3, 0, 1, 1, 2, 0}, {3, 1, 0, 1, 5, 0}, {4, 1, 0, 0, 0, 0}, {9, 1, 1, 0, 0, 0}};
    b.add(recs, 2, ref_at);
    b.add(recs + 2, 3, ref_at);
    CHECK(b.total == 5 && b.found[0] == 1 && b.found[1] == 4 && b.kept[0].size() == 1 && b.kept[1].size() == 2 && b.kept[0][0].ref == 'G' && b.kept[1][1].ref == 'A');
    for (const kgwas_locate_record& bad : {kgwas_locate_record{9, 1, 1, 0, 0, 0}, kgwas_locate_record{9, 1, 0, 0, 0, 0}, kgwas_locate_record{8, 0, 0, 0, 0, 0},
                                           kgwas_locate_record{10, 2, 0, 0, 0, 0}, kgwas_locate_record{10, 0, 2, 0, 0, 0}, kgwas_locate_record{10, 0, 0, 1, 0, 0},
                                           kgwas_locate_record{10, 0, 0, 0, 3, 0}, kgwas_locate_record{10, 0, 0, 1, 6, 0}})
        CHECK(has(refusal(KGWAS_ERR_STATE, [&] { b.add(&bad, 1, ref_at); }), "out of order"));
    Buckets all(1, 0, 5);  // 0: no limit
    const kgwas_locate_record three[] = {{0, 0, 0, 0, 0, 0}, {1, 0, 0, 0, 0, 0}, {2, 0, 0, 0, 0, 0}};
    all.add(three, 3, ref_at);
    CHECK(all.kept[0].size() == 3);
    std::vector<Contig> contigs(2);
    contigs[0].name = "c1", contigs[0].start = 0, contigs[0].length = 2, contigs[1].name = "c2", contigs[1].start = 3, contigs[1].length = 8;
    Query q;
    q.text = "TGAAC", q.p_text = "1e-9";
    std::string text = header_line(true);
    append_line(text, q, contigs, b.kept[0][0], true);  // GGTCA against GTTCA, the query's reverse complement: base 2, G for T
    append_line(text, q, contigs, Hit{0, 0, 0, 0, '.'}, true);
    append_line(text, q, contigs, Hit{5, 0, 1, 5, 'A'}, true);
    CHECK(text == "kmer\tcontig\tpos\tstrand\tmismatches\toffset\tref\talt\tp_lrt\nTGAAC\tc2\t1\t-\t1\t2\tG\tT\t1e-9\nTGAAC\tc1\t1\t+\t0\t0\t.\t.\t1e-9\n"
                  "TGAAC\tc2\t3\t+\t1\t5\tA\tC\t1e-9\n");
    CHECK(header_line(false) == "kmer\tcontig\tpos\tstrand\tmismatches\toffset\tref\talt\n");
}

int main() {
    check_limits_and_lists();
    for (uint32_t d = 0; d < 2; d++) {
        if (d == 0) check_search(1, 0, 2, 4, 1);
        check_search(2, d, 6, 4, 2);
        check_search(3, d, 20, 4, 3);
        check_search(5, d, 200, 4, 4);
        check_search(8, d, 300, 2, 5);  // two letters: most windows hit something, long ranges of equal half keys
        check_search(15, d, 300, 4, 6);
        check_search(16, d, 2200, 4, 7);  // more patterns than splitters: B > 1
        check_search(31, d, 300, 4, 8);
        check_search(31, d, 300, 2, 9);
    }
    check_fasta();
    check_queries();
    check_buckets_and_lines();
    printf(failures ? "locate_host_check: %d check(s) FAILED\n" : "locate_host_check: all checks passed\n", failures);
    return failures ? 1 : 0;
}
