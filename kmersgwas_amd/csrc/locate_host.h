// locate_host.h — the host side of locate_kmers that needs no device (locate.cpp; tools/locate_host_check.cpp runs it under the
// sanitizers): the limits, a query's codes, the sorted pattern lists the kernels search, the FASTA reader's line rules, the --kmers
// file in its three formats, the per-k-mer buckets and the output's bytes, over ld_host.h's text helpers; of proxy_host.h it needs
// the drain rounds of a piece's records.
#pragma once
#include <functional>
#include <unordered_set>

#include "proxy_host.h"

namespace kgwas {
namespace locate {

using proxy::drain_rounds;
using proxy::Round;

constexpr uint64_t MAX_KMERS = 1ull << 20;
constexpr uint32_t MAX_SPLITTERS = 2048;  // kernels.h: LOCATE_SPLITTERS (locate.cpp asserts it)

// the reverse complement of a k-base code (first base most significant)
inline uint64_t revcomp_code(uint64_t a, uint32_t k) {
    uint64_t r = 0;
    for (uint32_t i = 0; i < k; i++, a >>= 2) r = (r << 2) | (3 - (a & 3));
    return r;
}

// checked before any device call
inline void check_locate_shape(const char* who, uint32_t kmer_len, uint32_t mismatches, uint64_t n_kmers) {
    const std::string w(who);
    if (kmer_len < 1 || kmer_len > 31) throw Error(KGWAS_ERR_ARG, w + ": k-mers of 1 to 31 bases are supported");
    if (mismatches > 1) throw Error(KGWAS_ERR_ARG, w + ": mismatches must be 0 or 1");
    if (mismatches == 1 && kmer_len < 2) throw Error(KGWAS_ERR_ARG, w + ": one mismatch needs k-mers of at least 2 bases");
    if (n_kmers == 0 || n_kmers > MAX_KMERS)
        throw Error(KGWAS_ERR_ARG, w + ": " + std::to_string(n_kmers) + " k-mers: 1 to " + std::to_string(MAX_KMERS) + " are located at once");
}

// The patterns of the queries f[0..n) - (f_i, +) and, unless r_i == f_i, (r_i, -) - as the lists the kernels search: sorted by
// (key, id), id = kmer << 1 | strand, with the splitters spl[j] = keys[j * B]. d = 0: H alone, keyed by the code. d = 1: H keyed by
// the first ceil(k / 2) bases, L by the last floor(k / 2).
struct List {
    std::vector<uint64_t> keys, codes, spl;
    std::vector<uint32_t> ids;
    uint64_t B = 1;
};
struct Lists {
    List H, L;
};
inline List sorted_list(const std::vector<uint64_t>& codes, const std::vector<uint32_t>& ids, const std::function<uint64_t(uint64_t)>& key) {
    const size_t n = codes.size();
    std::vector<uint32_t> o(n);
    for (size_t i = 0; i < n; i++) o[i] = (uint32_t)i;
    std::vector<uint64_t> k(n);
    for (size_t i = 0; i < n; i++) k[i] = key(codes[i]);
    std::sort(o.begin(), o.end(), [&](uint32_t a, uint32_t b) { return k[a] != k[b] ? k[a] < k[b] : ids[a] < ids[b]; });
    List l;
    l.keys.resize(n), l.codes.resize(n), l.ids.resize(n);
    for (size_t i = 0; i < n; i++) l.keys[i] = k[o[i]], l.codes[i] = codes[o[i]], l.ids[i] = ids[o[i]];
    l.B = std::max<uint64_t>(1, (n + MAX_SPLITTERS - 1) / MAX_SPLITTERS);
    for (size_t j = 0; j * l.B < n; j++) l.spl.push_back(l.keys[j * l.B]);
    return l;
}
inline Lists build_lists(const char* who, const uint64_t* f, uint64_t n, uint32_t k, uint32_t d) {
    check_locate_shape(who, k, d, n);
    std::vector<uint64_t> codes;
    std::vector<uint32_t> ids;
    std::unordered_map<uint64_t, uint64_t> seen;  // canonical code -> query
    for (uint64_t i = 0; i < n; i++) {
        if (f[i] >> (2 * k)) throw Error(KGWAS_ERR_ARG, std::string(who) + ": code " + std::to_string(i) + " has bits at or above 2 * kmer_len");
        const uint64_t r = revcomp_code(f[i], k);
        const auto ins = seen.emplace(std::min(f[i], r), i);
        if (!ins.second)
            throw Error(KGWAS_ERR_ARG, std::string(who) + ": the queries " + std::to_string(ins.first->second) + " and " + std::to_string(i) + " are the same k-mer");
        codes.push_back(f[i]), ids.push_back((uint32_t)(i << 1));
        if (r != f[i]) codes.push_back(r), ids.push_back((uint32_t)(i << 1 | 1));
    }
    Lists out;
    const uint32_t lh = k / 2;
    if (d == 0)
        out.H = sorted_list(codes, ids, [](uint64_t c) { return c; });
    else {
        out.H = sorted_list(codes, ids, [lh](uint64_t c) { return c >> (2 * lh); });
        out.L = sorted_list(codes, ids, [lh](uint64_t c) { return c & ((1ull << (2 * lh)) - 1); });
    }
    return out;
}

// ---- the reference: FASTA in plain text ----------------------------------------------------------------------------------------------
// The first byte must be '>'. A trailing '\r' is dropped from every line; a missing final newline is fine. A contig's name is its
// header line after '>' up to the first blank or tab; its sequence the concatenation of its lines, every byte of which has a position.
// The STREAM is the sequences with one separator byte between contigs; a contig keeps its start in the stream and its length.
struct Contig {
    std::string name;
    uint64_t start = 0, length = 0;
};
constexpr char SEPARATOR = '\n';

// feed() takes the file's bytes in blocks of any size and hands the stream's bytes to `sink` in runs; finish() ends the file.
class FastaParser {
   public:
    std::vector<Contig> contigs;
    uint64_t stream_bytes = 0;
    FastaParser(std::string path, std::function<void(const char*, size_t)> sink) : path_(std::move(path)), sink_(std::move(sink)) {}
    void feed(const char* p, size_t n) {
        size_t i = 0;
        if (n && !any_) {
            any_ = true;
            if (p[0] != '>') throw Error(KGWAS_ERR_FORMAT, path_ + ": not FASTA");
        }
        while (i < n) {
            if (line_start_) {
                line_start_ = false;
                header_ = p[i] == '>';
                if (header_) {
                    head_.clear();
                    i++;
                    continue;
                }
            }
            const char* nl = static_cast<const char*>(memchr(p + i, '\n', n - i));
            const size_t e = nl ? (size_t)(nl - p) : n;  // the line's bytes in this block: [i, e)
            if (e > i) {
                if (held_cr_) put("\r", 1);  // (a '\r' inside a line, not at its end)
                held_cr_ = p[e - 1] == '\r';
                put(p + i, e - i - (held_cr_ ? 1 : 0));
            }
            if (nl) end_line();
            i = e + (nl ? 1 : 0);
        }
    }
    void finish() {
        if (!any_) throw Error(KGWAS_ERR_FORMAT, path_ + ": not FASTA (the file is empty)");
        if (!line_start_) end_line();
        if (!sequence_bytes_) throw Error(KGWAS_ERR_FORMAT, path_ + ": no sequence");
    }
    uint64_t sequence_bytes() const { return sequence_bytes_; }

   private:
    void put(const char* p, size_t n) {
        if (!n) return;
        if (header_) {
            head_.append(p, n);
            return;
        }
        // (the first byte must be '>', so a sequence line always has a contig)
        sink_(p, n);
        contigs.back().length += n, stream_bytes += n, sequence_bytes_ += n;
    }
    void end_line() {
        held_cr_ = false;
        line_++;
        line_start_ = true;
        if (!header_) return;
        const std::string name = head_.substr(0, head_.find_first_of(" \t"));
        const std::string at = path_ + " line " + std::to_string(line_) + ": ";
        if (name.empty()) throw Error(KGWAS_ERR_FORMAT, at + "a contig without a name");
        if (!names_.insert(name).second) throw Error(KGWAS_ERR_FORMAT, at + "the contig '" + name + "' is given twice");
        if (!contigs.empty()) {
            const char sep = SEPARATOR;
            sink_(&sep, 1);
            stream_bytes++;
        }
        Contig c;
        c.name = name, c.start = stream_bytes;
        contigs.push_back(std::move(c));
        header_ = false;
    }
    std::string path_, head_;
    std::function<void(const char*, size_t)> sink_;
    std::unordered_set<std::string> names_;
    uint64_t line_ = 0, sequence_bytes_ = 0;
    bool any_ = false, line_start_ = true, header_ = false, held_cr_ = false;
};

// the contig of a stream offset that lies in one: the last contig that starts at or before it
inline const Contig& contig_of(const std::vector<Contig>& contigs, uint64_t pos) {
    auto it = std::upper_bound(contigs.begin(), contigs.end(), pos, [](uint64_t p, const Contig& c) { return p < c.start; });
    if (it == contigs.begin() || pos - (it - 1)->start >= (it - 1)->length) throw Error(KGWAS_ERR_STATE, "locate: a hit outside every contig");
    return *(it - 1);
}

// ---- the --kmers file ------------------------------------------------------------------------------------------------------------------
// Three formats, told apart by the first line: a tab-separated file whose header has a column `rs` (an lmm_lrt / GEMMA .assoc.txt
// or a clump_kmers output), one whose header has a column `kmer` and no `rs` (a proxy_kmers output: its distinct values in order of
// first appearance), else a plain list, one k-mer per line. A column `p_lrt` is carried along as text.
struct Query {
    std::string text, p_text;
    uint64_t f = 0;  // the code of the letters as spelled
};
struct Queries {
    std::vector<Query> q;
    bool has_p = false;
};
inline uint64_t spelled_code(const std::string& text, uint32_t kmer_len, const std::string& at) {
    if (text.size() != kmer_len)
        throw Error(KGWAS_ERR_FORMAT, at + "k-mer '" + text + "' has length " + std::to_string(text.size()) + ", not " + std::to_string(kmer_len));
    uint64_t c = 0;
    for (char ch : text) {
        const char* p = ch ? strchr("ACGT", ch) : nullptr;
        if (!p) throw Error(KGWAS_ERR_FORMAT, at + "k-mer '" + text + "' has a letter other than A, C, G, T");
        c = c << 2 | (uint64_t)(p - "ACGT");
    }
    return c;
}
inline Queries read_queries(const std::string& path, uint32_t kmer_len) {
    std::ifstream f(path);
    if (!f.is_open()) throw Error(KGWAS_ERR_IO, "can't open k-mers file: " + path);
    Queries out;
    std::unordered_map<uint64_t, uint64_t> seen;  // canonical code -> file line
    std::string line;
    size_t n_head = 0, c_kmer = 0, c_p = 0;
    bool first = true, table = false, distinct = false;
    for (uint64_t ln = 1; std::getline(f, line); ln++) {
        const std::vector<std::string> fl = fields_of(line);
        if (first) {
            first = false;
            const auto rs = std::find(fl.begin(), fl.end(), "rs"), km = std::find(fl.begin(), fl.end(), "kmer"), p = std::find(fl.begin(), fl.end(), "p_lrt");
            table = rs != fl.end() || km != fl.end();
            if (table) {
                distinct = rs == fl.end();
                c_kmer = (size_t)((distinct ? km : rs) - fl.begin());
                out.has_p = p != fl.end();
                c_p = (size_t)(p - fl.begin());
                n_head = fl.size();
                continue;
            }
        }
        if (fl.empty()) continue;
        const std::string at = path + " line " + std::to_string(ln) + ": ";
        if (table && fl.size() <= std::max(c_kmer, out.has_p ? c_p : 0))
            throw Error(KGWAS_ERR_FORMAT, at + "too few fields (" + std::to_string(fl.size()) + ", the header has " + std::to_string(n_head) + ")");
        if (!table && fl.size() != 1) throw Error(KGWAS_ERR_FORMAT, at + std::to_string(fl.size()) + " fields: a list of k-mers has one k-mer per line");
        Query q;
        q.text = fl[table ? c_kmer : 0];
        if (out.has_p) q.p_text = fl[c_p];
        q.f = spelled_code(q.text, kmer_len, at);
        const auto ins = seen.emplace(std::min(q.f, revcomp_code(q.f, kmer_len)), ln);
        if (!ins.second) {
            if (distinct) continue;
            throw Error(KGWAS_ERR_FORMAT, at + "duplicate k-mer '" + q.text + "' (the k-mer of line " + std::to_string(ins.first->second) + ")");
        }
        out.q.push_back(std::move(q));
    }
    if (out.q.empty()) throw Error(KGWAS_ERR_FORMAT, path + ": no k-mer");
    return out;
}

// ---- the hits --------------------------------------------------------------------------------------------------------------------------
// Per k-mer the first max_per_kmer hits in record order (0: all of them) with the reference's letter at the mismatch, and the count
// of all of them. Records arrive in (pos, kmer, strand) order; ref_at(stream offset) is the stream's byte there.
struct Hit {
    uint64_t pos;
    uint8_t strand, mismatches, offset;
    char ref;
};
struct Buckets {
    uint64_t max_per_kmer, total = 0, last_pos = 0;
    uint32_t last_id = 0, kmer_len;
    bool any = false;
    std::vector<std::vector<Hit>> kept;
    std::vector<uint64_t> found;
    Buckets(uint64_t n_kmers, uint64_t max_per, uint32_t k) : max_per_kmer(max_per), kmer_len(k), kept(n_kmers), found(n_kmers, 0) {}
    template <class RefAt>
    void add(const kgwas_locate_record* rec, uint64_t n, RefAt&& ref_at) {
        for (uint64_t i = 0; i < n; i++) {
            const kgwas_locate_record& r = rec[i];
            const uint32_t id = r.kmer << 1 | r.strand;
            if (r.kmer >= kept.size() || r.strand > 1 || r.mismatches > 1 || r.offset > kmer_len || (r.mismatches == 1) != (r.offset != 0) ||
                (any && (r.pos < last_pos || (r.pos == last_pos && id <= last_id))))
                throw Error(KGWAS_ERR_STATE, "locate: the records arrive out of order");
            any = true, last_pos = r.pos, last_id = id;
            total++;
            if (found[r.kmer]++ >= max_per_kmer && max_per_kmer) continue;
            char ref = '.';
            if (r.mismatches) ref = (char)(ref_at(r.pos + r.offset - 1) & 0xDF);
            kept[r.kmer].push_back(Hit{r.pos, r.strand, r.mismatches, r.offset, ref});
        }
    }
};

inline std::string header_line(bool has_p) { return std::string("kmer\tcontig\tpos\tstrand\tmismatches\toffset\tref\talt") + (has_p ? "\tp_lrt\n" : "\n"); }

// One output line: the k-mer as its file spells it, the contig, the 1-based position of the window's first base in it, the strand,
// the mismatches, the offset, ref and alt ('.' for an exact hit), and the k-mer's p_lrt text where the input had the column. alt is
// the k-mer's base at the mismatch in the reference's orientation: on strand - the complement of the query's letter at k - offset.
inline void append_line(std::string& text, const Query& q, const std::vector<Contig>& contigs, const Hit& h, bool has_p) {
    const Contig& c = contig_of(contigs, h.pos);
    const size_t k = q.text.size();
    char alt = '.';
    if (h.mismatches) {
        if (h.offset < 1 || h.offset > k) throw Error(KGWAS_ERR_STATE, "locate: a mismatch outside its window");
        alt = h.strand ? "TGCA"[strchr("ACGT", q.text[k - h.offset]) - "ACGT"] : q.text[h.offset - 1];
    }
    text += q.text + "\t" + c.name + "\t" + std::to_string(h.pos - c.start + 1) + "\t" + (h.strand ? "-" : "+") + "\t" + std::to_string(h.mismatches) + "\t" +
            std::to_string(h.offset) + "\t" + h.ref + "\t" + alt;
    if (has_p) text += "\t" + q.p_text;
    text += "\n";
}

}  // namespace locate
}  // namespace kgwas
