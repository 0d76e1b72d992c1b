// fetch_host.h — the host side of fetch_reads that needs no device (fetch.cpp; tools/fetch_host_check.cpp runs it under the
// sanitizers): the limits, the sorted list of canonical codes the kernels search, the cutting of a read stream into pieces at
// newlines, the reads files' records (over reads_source.h, which count_kmers.cpp shares), and the three outputs' bytes. Of
// locate_host.h it needs the list builder, the --kmers file and the drain rounds.
#pragma once
#include "locate_host.h"
#include "reads_source.h"

namespace kgwas {
namespace fetch {

using locate::drain_rounds;
using locate::List;
using locate::Queries;
using locate::Round;

// checked before any device call
inline void check_fetch_shape(const char* who, uint32_t kmer_len, uint32_t min_hits, uint64_t n_kmers) {
    const std::string w(who);
    if (kmer_len < 1 || kmer_len > 31) throw Error(KGWAS_ERR_ARG, w + ": k-mers of 1 to 31 bases are supported");
    if (min_hits < 1) throw Error(KGWAS_ERR_ARG, w + ": min_hits must be at least 1");
    if (n_kmers == 0 || n_kmers > locate::MAX_KMERS)
        throw Error(KGWAS_ERR_ARG, w + ": " + std::to_string(n_kmers) + " k-mers: 1 to " + std::to_string(locate::MAX_KMERS) + " are fetched at once");
}

// The queries f[0..n) as ONE list sorted by canonical code: keys == codes, ids[i] = query << 1 | (the canonical code is the reverse
// complement of the query as spelled).
inline List build_list(const char* who, const uint64_t* f, uint64_t n, uint32_t k, uint32_t min_hits) {
    check_fetch_shape(who, k, min_hits, n);
    std::vector<uint64_t> codes(n);
    std::vector<uint32_t> ids(n);
    std::unordered_map<uint64_t, uint64_t> seen;  // canonical code -> query
    for (uint64_t i = 0; i < n; i++) {
        if (f[i] >> (2 * k)) throw Error(KGWAS_ERR_ARG, std::string(who) + ": code " + std::to_string(i) + " has bits at or above 2 * kmer_len");
        const uint64_t r = locate::revcomp_code(f[i], k), c = std::min(f[i], r);
        const auto ins = seen.emplace(c, i);
        if (!ins.second)
            throw Error(KGWAS_ERR_ARG, std::string(who) + ": the queries " + std::to_string(ins.first->second) + " and " + std::to_string(i) + " are the same k-mer");
        codes[i] = c, ids[i] = (uint32_t)(i << 1 | (c != f[i]));
    }
    return locate::sorted_list(codes, ids, [](uint64_t c) { return c; });
}

// ---- pieces ----------------------------------------------------------------------------------------------------------------------------
// The next piece of the stream p[0, left): at most P bytes that end behind a newline. What is left and shorter than P goes whole,
// and gets a newline where it has none (add_newline: bytes counts it). A read that does not fit a piece is refused with its length.
struct Cut {
    uint64_t take = 0, bytes = 0, reads = 0;  // bytes of the stream taken, bytes of the piece, its newlines
    bool add_newline = false, last = false;
};
inline Cut cut_piece(const char* who, const uint8_t* p, uint64_t left, uint64_t P) {
    Cut c;
    if (left < P) {
        c.take = left, c.last = true;
        c.add_newline = left && p[left - 1] != '\n';
    } else {
        const void* nl = memrchr(p, '\n', P);
        if (!nl) {
            const void* e = memchr(p, '\n', left);
            const uint64_t len = e ? (uint64_t)(static_cast<const uint8_t*>(e) - p) : left;
            throw Error(KGWAS_ERR_ARG, std::string(who) + ": a read of " + std::to_string(len) + " bytes does not fit a piece of " + std::to_string(P) + " bytes");
        }
        c.take = (uint64_t)(static_cast<const uint8_t*>(nl) - p) + 1;
        c.last = c.take == left;
    }
    c.bytes = c.take + (c.add_newline ? 1 : 0);
    c.reads = (uint64_t)std::count(p, p + c.take, (uint8_t)'\n') + (c.add_newline ? 1 : 0);
    return c;
}

// ---- the reads files -------------------------------------------------------------------------------------------------------------------
// FASTA or FASTQ in plain text, by count_kmers.cpp's rules: a FASTQ record is four lines with '@' and '+' at the head of its first
// and third line; a FASTA record's sequence is the concatenation of its lines; a trailing '\r' is dropped for the stream; a missing
// final newline is fine. next() hands out one record: its bytes as the file has them, and its sequence.
struct Record {
    const char *raw = nullptr, *seq = nullptr;  // valid until the next call
    size_t raw_len = 0, seq_len = 0;
};
class RecordReader {
   public:
    typedef std::function<size_t(char*, size_t)> ReadFn;  // up to n bytes; 0: the end
    // fmt: the first byte, which open_source took ('>' or '@'; 0: an empty file)
    RecordReader(std::string path, char fmt, ReadFn read, size_t block = 4u << 20) : path_(std::move(path)), fmt_(fmt), read_(std::move(read)), block_(block) {
        if (fmt)
            buf_.push_back(fmt);
        else
            eof_ = true;
    }
    bool next(Record& rec) {
        for (;;) {
            const size_t n = buf_.size();
            if (pos_ >= n) {
                if (more()) continue;
                return false;
            }
            const char* d = buf_.data();
            bool whole = true;  // is the record's end in the buffer?
            size_t p = pos_;
            if (fmt_ == '@') {
                size_t b[4], e[4];
                int lines = 0;
                for (; lines < 4 && p < n; lines++) {
                    b[lines] = p, e[lines] = line_end(d, p, n);
                    if (e[lines] == n && !eof_) {
                        whole = false;
                        break;
                    }
                    p = e[lines] + 1;
                }
                if (!whole || (lines < 4 && !eof_)) {
                    more();
                    continue;
                }
                if (lines < 4) throw Error(KGWAS_ERR_FORMAT, path_ + ": the last FASTQ record has fewer than four lines");
                if (d[b[0]] != '@' || b[2] == e[2] || d[b[2]] != '+')
                    throw Error(KGWAS_ERR_FORMAT, path_ + ": a FASTQ record does not have '@' and '+' at the head of its first and third line");
                size_t len = e[1] - b[1];
                if (len && d[b[1] + len - 1] == '\r') len--;
                rec.seq = d + b[1], rec.seq_len = len;
            } else {
                seq_.clear();
                bool head = true;
                while (p < n && (head || d[p] != '>')) {
                    const size_t e = line_end(d, p, n);
                    if (e == n && !eof_) {
                        whole = false;
                        break;
                    }
                    size_t l = e - p;
                    if (l && d[p + l - 1] == '\r') l--;
                    if (!head) seq_.append(d + p, l);
                    head = false;
                    p = e + 1;
                }
                if (!whole || (p >= n && !eof_)) {  // (the next line may still belong to this record)
                    more();
                    continue;
                }
                rec.seq = seq_.data(), rec.seq_len = seq_.size();
            }
            rec.raw = d + pos_, rec.raw_len = std::min(p, n) - pos_;
            pos_ = std::min(p, n);
            return true;
        }
    }
    const std::string& path() const { return path_; }

   private:
    bool more() {  // drops what is consumed and reads one more block
        if (eof_) return false;
        buf_.erase(buf_.begin(), buf_.begin() + pos_);
        pos_ = 0;
        const size_t old = buf_.size();
        buf_.resize(old + block_);
        const size_t r = read_(buf_.data() + old, block_);
        buf_.resize(old + r);
        if (!r) eof_ = true;
        return true;
    }
    std::string path_, seq_;
    char fmt_;
    ReadFn read_;
    size_t block_, pos_ = 0;
    std::vector<char> buf_;
    bool eof_ = false;
};

inline const char* extension_of(char fmt) { return fmt == '>' ? "fasta" : "fastq"; }

// ---- the outputs -----------------------------------------------------------------------------------------------------------------------
// What the host keeps of a piece until its records are back: the records' bytes as the files have them (a newline added where the
// last record lacked one), per file, and where each starts. Unit u of the piece is read read0 + u (no mates) or the pair of the
// reads read0 + 2 u, read0 + 2 u + 1.
struct PieceMeta {
    std::vector<char> raw[2];
    std::vector<uint64_t> off[2];
    uint64_t read0 = 0;
    uint32_t mates = 1;  // files: 1 or 2
    void clear(uint64_t first_read, uint32_t files) {
        read0 = first_read, mates = files;
        for (int f = 0; f < 2; f++) raw[f].clear(), off[f].assign(1, 0);
    }
    void add(int f, const Record& r) {
        raw[f].insert(raw[f].end(), r.raw, r.raw + r.raw_len);
        if (!r.raw_len || r.raw[r.raw_len - 1] != '\n') raw[f].push_back('\n');
        off[f].push_back(raw[f].size());
    }
    uint64_t units() const { return off[0].size() - 1; }
};

// PREFIX.fastq / .fasta (with mates PREFIX_1.*, PREFIX_2.*), PREFIX.reads.tsv and, at commit, PREFIX.log.txt. A unit is written when
// one of its reads is kept and its k-mer - the first kept read's - has fewer than max_per_kmer units so far (0: no limit); the rest
// are counted. What is not committed is removed again.
class Outputs {
   public:
    uint64_t reads_kept = 0, reads_written = 0, pairs_written = 0;
    std::vector<uint64_t> written;  // per query: the units written for it
    Outputs(const std::string& prefix, char fmt, bool mates, const Queries& queries, uint64_t max_per_kmer)
        : written(queries.q.size(), 0), q_(queries), max_(max_per_kmer), mates_(mates) {
        const std::string ext = extension_of(fmt);
        log_path_ = prefix + ".log.txt";
        try {
            if (mates)
                open(prefix + "_1." + ext), open(prefix + "_2." + ext);
            else
                open(prefix + "." + ext);
            open(prefix + ".reads.tsv");
            put(f_.back(), "read\tmate\tn_hits\tfirst_pos\tkmer\tstrand\n");
        } catch (...) {
            discard();
            throw;
        }
    }
    // the records of one piece, in ascending read
    void add(const PieceMeta& m, const kgwas_fetch_record* rec, uint64_t n) {
        const uint32_t files = mates_ ? 2 : 1;
        if (m.mates != files) throw Error(KGWAS_ERR_STATE, "fetch: a piece of another shape");
        for (uint64_t i = 0; i < n;) {
            auto unit_of = [&](const kgwas_fetch_record& r) {
                if (r.read < m.read0 || (r.read - m.read0) / files >= m.units() || r.kmer >= q_.q.size() || r.strand > 1 || (any_ && r.read <= last_))
                    throw Error(KGWAS_ERR_STATE, "fetch: the records arrive out of order");
                any_ = true, last_ = r.read;
                return (r.read - m.read0) / files;
            };
            const uint64_t u = unit_of(rec[i]);
            uint64_t j = i + 1;
            if (j < n && (rec[j].read - m.read0) / files == u) unit_of(rec[j++]);
            const uint32_t owner = rec[i].kmer;
            reads_kept += j - i;
            if (!max_ || written[owner] < max_) {
                written[owner]++;
                for (uint32_t f = 0; f < files; f++) put(f_[f], m.raw[f].data() + m.off[f][u], m.off[f][u + 1] - m.off[f][u]);
                for (uint64_t t = i; t < j; t++) {
                    const uint32_t f = (uint32_t)((rec[t].read - m.read0) % files);
                    const char* h = m.raw[f].data() + m.off[f][u] + 1;  // behind '@' or '>'
                    const char* e = m.raw[f].data() + m.off[f][u + 1];
                    const char* c = h;
                    while (c < e && *c != ' ' && *c != '\t' && *c != '\r' && *c != '\n') c++;
                    const std::string line = std::string(h, c) + "\t" + std::to_string(mates_ ? f + 1 : 0) + "\t" + std::to_string(rec[t].n_hits) + "\t" +
                                             std::to_string(rec[t].first_pos + 1) + "\t" + q_.q[rec[t].kmer].text + "\t" + (rec[t].strand ? "-" : "+") + "\n";
                    put(f_.back(), line.data(), line.size());
                }
                reads_written += j - i, pairs_written += mates_ ? 1 : 0;
            }
            i = j;
        }
    }
    void commit(const std::string& log_text) {
        for (size_t i = 0; i < f_.size(); i++) {
            FILE* f = f_[i];
            f_[i] = nullptr;
            if (fclose(f) != 0) throw Error(KGWAS_ERR_IO, "can't write " + paths_[i]);
        }
        paths_.push_back(log_path_);
        write_text(log_path_, log_text);
        done_ = true;
    }
    ~Outputs() { discard(); }

   private:
    void discard() {
        for (FILE*& f : f_)
            if (f) fclose(f), f = nullptr;
        if (!done_)
            for (const std::string& p : paths_) ::unlink(p.c_str());
    }
    void open(const std::string& path) {
        FILE* f = fopen(path.c_str(), "wb");
        if (!f) throw Error(KGWAS_ERR_IO, "can't write " + path);
        f_.push_back(f), paths_.push_back(path);
    }
    void put(FILE* f, const char* p, size_t n) {
        if (n && fwrite(p, 1, n, f) != n) throw Error(KGWAS_ERR_IO, "can't write " + paths_[0]);
    }
    void put(FILE* f, const char* text) { put(f, text, strlen(text)); }
    const Queries& q_;
    uint64_t max_, last_ = 0;
    bool mates_, any_ = false, done_ = false;
    std::vector<FILE*> f_;
    std::vector<std::string> paths_;
    std::string log_path_;
};

}  // namespace fetch
}  // namespace kgwas
