// clump_host.h — the host side of clump_kmers that needs no device (clump.cpp; tools/clump_host_check.cpp runs it under the
// sanitizers): the assoc file, the p order, the streaming clump pass and the output's bytes, over ld_host.h's text helpers.
#pragma once
#include "ld_host.h"

namespace kgwas {
namespace clump {

constexpr uint64_t LD_MAX_KMERS = 1ull << 20;

inline void check_clump_shape(const char* who, uint64_t n_kmers, uint64_t n_acc, uint32_t tm) {
    check_ld_shape(who, n_acc, tm);
    if (n_kmers > LD_MAX_KMERS)
        throw Error(KGWAS_ERR_ARG, std::string(who) + ": " + std::to_string(n_kmers) + " k-mers: at most " + std::to_string(LD_MAX_KMERS) + " are clumped at once");
}

struct Hit {
    std::string rs, p_text;
    double p = 0;
    uint64_t code = 0, line = 0;  // line: the hit's place among the file's data lines, from 0
};

// An lmm_lrt or GEMMA .assoc.txt: the columns `rs` (the k-mer's letters) and `p_lrt` are found by their names in the header, so
// the 9-column and the 14-column layouts both read. encode is kgwas_kmer_encode (a status and the code).
inline std::vector<Hit> read_assoc(const std::string& path, uint32_t kmer_len, EncodeFn encode) {
    std::ifstream f(path);
    if (!f.is_open()) throw Error(KGWAS_ERR_IO, "can't open assoc file: " + path);
    std::string line;
    std::vector<std::string> head;
    while (head.empty() && std::getline(f, line)) head = fields_of(line);
    size_t c_rs = head.size(), c_p = head.size();
    for (size_t i = 0; i < head.size(); i++) {
        if (head[i] == "rs" && c_rs == head.size()) c_rs = i;
        if (head[i] == "p_lrt" && c_p == head.size()) c_p = i;
    }
    if (c_rs == head.size()) throw Error(KGWAS_ERR_FORMAT, path + ": the header has no column 'rs'");
    if (c_p == head.size()) throw Error(KGWAS_ERR_FORMAT, path + ": the header has no column 'p_lrt'");
    std::vector<Hit> hits;
    std::unordered_map<uint64_t, uint64_t> seen;  // code -> file line
    for (uint64_t ln = 2; std::getline(f, line); ln++) {
        const std::vector<std::string> fl = fields_of(line);
        if (fl.empty()) continue;
        const std::string at = path + " line " + std::to_string(ln) + ": ";
        if (fl.size() <= std::max(c_rs, c_p))
            throw Error(KGWAS_ERR_FORMAT, at + "too few fields (" + std::to_string(fl.size()) + ", the header has " + std::to_string(head.size()) + ")");
        Hit h;
        h.rs = fl[c_rs];
        h.p_text = fl[c_p];
        h.line = hits.size();
        h.code = parse_kmer_field(h.rs, kmer_len, encode, at);
        char* end = nullptr;
        errno = 0;
        h.p = strtod(h.p_text.c_str(), &end);
        if (end == h.p_text.c_str() || *end != 0 || std::isnan(h.p)) throw Error(KGWAS_ERR_FORMAT, at + "p_lrt '" + h.p_text + "' is not a number");
        const auto ins = seen.emplace(h.code, ln);
        if (!ins.second)
            throw Error(KGWAS_ERR_FORMAT, at + "duplicate k-mer '" + h.rs + "' (the k-mer of line " + std::to_string(ins.first->second) + ")");
        hits.push_back(std::move(h));
    }
    return hits;
}

// The hits with p <= p_max, by p ascending, ties by their line: indices into hits.
inline std::vector<uint32_t> p_order(const std::vector<Hit>& hits, double p_max) {
    std::vector<uint32_t> o;
    for (size_t i = 0; i < hits.size(); i++)
        if (hits[i].p <= p_max) o.push_back((uint32_t)i);
    std::stable_sort(o.begin(), o.end(), [&](uint32_t a, uint32_t b) { return hits[a].p < hits[b].p; });
    return o;
}

// The clump pass over the link matrix's upper triangle as it arrives, a block of consecutive rows at a time. Rows are walked in
// order; a row no lead has taken becomes a lead and takes every later row that is linked to it and not yet taken. Only the rows
// above the diagonal are needed: when row a is reached every row before it is already in a clump.
struct Clumper {
    static constexpr uint32_t NONE = 0xFFFFFFFFu;
    uint64_t N = 0, next_row = 0, pairs = 0;
    std::vector<uint32_t> lead_of;  // per row the row of its lead
    std::vector<uint32_t> leads;    // in lead order
    explicit Clumper(uint64_t n) : N(n), lead_of(n, NONE) {}
    // rows [row0, row0 + rows): adj[(a - row0) * pitch_dw + b / 32] bit b % 32
    void block(uint64_t row0, uint64_t rows, const uint32_t* adj, uint64_t pitch_dw) {
        if (row0 != next_row || row0 + rows > N) throw Error(KGWAS_ERR_STATE, "clump: the link matrix's blocks arrive out of order");
        const uint64_t n_dw = (N + 31) / 32;
        for (uint64_t a = row0; a < row0 + rows; a++) {
            const uint32_t* row = adj + (a - row0) * pitch_dw;
            const bool lead = lead_of[a] == NONE;
            if (lead) {
                lead_of[a] = (uint32_t)a;
                leads.push_back((uint32_t)a);
            }
            for (uint64_t w = a / 32; w < n_dw; w++) {
                uint32_t x = row[w];
                pairs += (uint64_t)__builtin_popcount(x);
                while (lead && x) {
                    const uint64_t b = 32 * w + (uint64_t)__builtin_ctz(x);
                    x &= x - 1;
                    if (b < N && lead_of[b] == NONE) lead_of[b] = (uint32_t)a;
                }
            }
        }
        next_row = row0 + rows;
    }
};

// popcounts over the accessions in use: mask[W] has their bits (all of the row's without a phenotype file)
inline uint32_t count_and(const uint64_t* a, const uint64_t* b, const uint64_t* mask, uint64_t W) {
    uint32_t c = 0;
    for (uint64_t w = 0; w < W; w++) c += (uint32_t)__builtin_popcountll(a[w] & b[w] & mask[w]);
    return c;
}

// One output line: rs, p_lrt (the field's own text), clump (from 1, in lead order), lead, r2 against the lead, n1, n11.
inline void append_line(std::string& text, const Hit& h, uint64_t clump_no, const Hit& lead, bool is_lead, uint64_t n, uint64_t n1, uint64_t n1_lead,
                        uint64_t n11) {
    char buf[64];
    const double r2 = r2_of(n, n1, n1_lead, n11);
    if (std::isnan(r2))
        snprintf(buf, sizeof(buf), "nan");
    else
        snprintf(buf, sizeof(buf), "%.6f", is_lead ? 1.0 : r2);
    text += h.rs + "\t" + h.p_text + "\t" + std::to_string(clump_no) + "\t" + lead.rs + "\t" + buf + "\t" + std::to_string(n1) + "\t" +
            std::to_string(n11) + "\n";
}
inline const char* header_line() { return "rs\tp_lrt\tclump\tlead\tr2\tn1\tn11\n"; }

}  // namespace clump
}  // namespace kgwas
