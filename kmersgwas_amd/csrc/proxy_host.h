// proxy_host.h — the host side of proxy_kmers that needs no device (proxy.cpp; tools/proxy_host_check.cpp runs it under the
// sanitizers): the limits, the leads file in its two formats, the drain rounds of a piece's records, the per-lead buckets and the
// output's bytes, over ld_host.h's text helpers; of clump_host.h it needs a clump_kmers output's header line (a leads format).
#pragma once
#include "clump_host.h"

namespace kgwas {
namespace proxy {

constexpr uint64_t MAX_LEADS = 4096;

// checked before any device call
inline void check_proxy_shape(const char* who, uint64_t n_leads, uint64_t n_acc, uint32_t tm) {
    check_ld_shape(who, n_acc, tm);
    if (n_leads == 0 || n_leads > MAX_LEADS)
        throw Error(KGWAS_ERR_ARG, std::string(who) + ": " + std::to_string(n_leads) + " leads: 1 to " + std::to_string(MAX_LEADS) + " are searched at once");
}

struct Lead {
    std::string text;  // as the file spells it
    uint64_t code = 0;
};

// The leads, in the file's order. Two formats: a plain list, one k-mer per line (filter_kmers --kmers_file), or a clump_kmers
// output, known by its header: then the distinct values of its column `lead`, in clump order (by its column `clump`; the file's
// lines are in the assoc file's order). A k-mer of another length, with a letter other than A, C, G, T, or given twice is refused
// with its line.
inline std::vector<Lead> read_leads(const std::string& path, uint32_t kmer_len, EncodeFn encode) {
    std::ifstream f(path);
    if (!f.is_open()) throw Error(KGWAS_ERR_IO, "can't open leads file: " + path);
    std::string head_text = clump::header_line();
    head_text.pop_back();  // (its newline)
    const std::vector<std::string> clump_head = fields_of(head_text);
    std::vector<Lead> leads;
    std::vector<uint64_t> clump_no;               // per lead of a clump_kmers output
    std::unordered_map<uint64_t, uint64_t> seen;  // code -> file line
    std::string line;
    bool clumps = false, first = true;
    for (uint64_t ln = 1; std::getline(f, line); ln++) {
        const std::vector<std::string> fl = fields_of(line);
        if (fl.empty()) continue;
        const std::string at = path + " line " + std::to_string(ln) + ": ";
        if (first) {
            first = false;
            if (fl == clump_head) {
                clumps = true;
                continue;
            }
        }
        if (clumps && fl.size() != clump_head.size())
            throw Error(KGWAS_ERR_FORMAT, at + std::to_string(fl.size()) + " fields, a clump_kmers line has " + std::to_string(clump_head.size()));
        if (!clumps && fl.size() != 1) throw Error(KGWAS_ERR_FORMAT, at + std::to_string(fl.size()) + " fields: a list of leads has one k-mer per line");
        Lead l;
        l.text = clumps ? fl[3] : fl[0];
        l.code = parse_kmer_field(l.text, kmer_len, encode, at);
        const auto ins = seen.emplace(l.code, ln);
        if (!ins.second) {
            if (clumps) continue;  // (a clump's members all name its lead)
            throw Error(KGWAS_ERR_FORMAT, at + "duplicate k-mer '" + l.text + "' (the k-mer of line " + std::to_string(ins.first->second) + ")");
        }
        if (clumps) {
            char* end = nullptr;
            errno = 0;
            const unsigned long long c = strtoull(fl[2].c_str(), &end, 10);
            if (fl[2].find_first_not_of("0123456789") != std::string::npos || fl[2].empty() || *end != 0 || errno)
                throw Error(KGWAS_ERR_FORMAT, at + "clump '" + fl[2] + "' is not a number");
            clump_no.push_back(c);
        }
        leads.push_back(std::move(l));
    }
    if (clumps) {
        std::vector<uint32_t> o(leads.size());
        for (size_t i = 0; i < o.size(); i++) o[i] = (uint32_t)i;
        std::stable_sort(o.begin(), o.end(), [&](uint32_t a, uint32_t b) { return clump_no[a] < clump_no[b]; });
        std::vector<Lead> sorted;
        for (uint32_t i : o) sorted.push_back(std::move(leads[i]));
        leads.swap(sorted);
    }
    if (leads.empty()) throw Error(KGWAS_ERR_FORMAT, path + ": no lead k-mer");
    return leads;
}

// A piece's records are numbered in (row, lead) order; boff[b] is the number of the first record of block b (256 rows) and
// boff[n_blocks] their count. The device buffer holds `cap` of them: round i takes the records [lo, hi) = [i cap, (i + 1) cap) from
// the blocks [blk0, blk1) that hold any of them.
struct Round {
    uint32_t lo, hi, blk0, blk1;
};
inline std::vector<Round> drain_rounds(const uint32_t* boff, uint32_t n_blocks, uint32_t cap) {
    if (!cap) throw Error(KGWAS_ERR_ARG, "proxy: a record buffer of 0 records");
    for (uint32_t b = 0; b < n_blocks; b++)
        if (boff[b] > boff[b + 1]) throw Error(KGWAS_ERR_STATE, "proxy: the records' block offsets descend");
    std::vector<Round> rounds;
    const uint32_t total = n_blocks ? boff[n_blocks] : 0;
    for (uint64_t lo = 0; lo < total; lo += cap) {
        const uint32_t hi = (uint32_t)std::min<uint64_t>(total, lo + cap);
        // the first block that ends past lo, the first block that starts at or past hi
        const uint32_t blk0 = (uint32_t)(std::upper_bound(boff + 1, boff + n_blocks + 1, (uint32_t)lo) - (boff + 1));
        const uint32_t blk1 = (uint32_t)(std::lower_bound(boff, boff + n_blocks, hi) - boff);
        rounds.push_back(Round{(uint32_t)lo, hi, blk0, blk1});
    }
    return rounds;
}

// Per lead the first max_per_lead records in table order, and the count of all of them. Records arrive in (row, lead) order.
struct Buckets {
    uint64_t max_per_lead, next_row = 0, total = 0;
    uint32_t last_lead = 0;
    bool any = false;
    std::vector<std::vector<kgwas_proxy_record>> kept;
    std::vector<uint64_t> found;
    Buckets(uint64_t n_leads, uint64_t max_per) : max_per_lead(max_per), kept(n_leads), found(n_leads, 0) {}
    void add(const kgwas_proxy_record* rec, uint64_t n) {
        for (uint64_t i = 0; i < n; i++) {
            const kgwas_proxy_record& r = rec[i];
            if (r.lead >= kept.size() || (any && (r.row < next_row || (r.row == next_row && r.lead <= last_lead))))
                throw Error(KGWAS_ERR_STATE, "proxy: the records arrive out of order");
            any = true, next_row = r.row, last_lead = r.lead;
            if (found[r.lead]++ < max_per_lead) kept[r.lead].push_back(r);
            total++;
        }
    }
};

inline const char* header_line() { return "lead\tkmer\tr2\tphase\tn1\tn11\trow\n"; }

// One output line: the lead as its file spells it, the proxy's k-mer, r2 (%.6f of num / den), the sign of n n11 - ca cb, the proxy's
// n1, n11 with the lead, the proxy's table row.
inline void append_line(std::string& text, const std::string& lead, uint32_t kmer_len, uint64_t n, uint64_t n1_lead, const kgwas_proxy_record& r) {
    char buf[64];
    snprintf(buf, sizeof(buf), "%.6f", r2_of(n, r.n1, n1_lead, r.n11));
    const bool minus = n * r.n11 < n1_lead * (uint64_t)r.n1;
    text += lead + "\t" + kmer_letters(r.kmer, kmer_len) + "\t" + buf + "\t" + (minus ? "-" : "+") + "\t" + std::to_string(r.n1) + "\t" +
            std::to_string(r.n11) + "\t" + std::to_string(r.row) + "\n";
}

}  // namespace proxy
}  // namespace kgwas
