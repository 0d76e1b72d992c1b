// lmm_files.cpp — the file layer of the lmm_lrt tool over the passes of lmm.cpp and lmm_table.cpp: the parsers,
// the .assoc.txt formatter and the writers. It makes no HIP call of its own; the parsers and the formatter run without a GPU.
//
// run_files: kinship text, .fam phenotype column, .bim, .bed in, .assoc.txt and .log.txt out. Individuals without a phenotype are
//            dropped from K, y and the .bed rows before anything else; beds that keep the same individuals share one handle, so
//            one eigendecomposition;
// run_file_multi: one bfile, several .fam columns with one missing set, one pass over the .bed (the shape of
//            kmers_gwas.py:193-223);
// run_table, run_table_multi: lmm_lrt --kmers_table, with -n and with --pheno_columns.
// -lmm 4   : run_files with all_tests writes the 14-column file (format_assoc4) and four more lines in the log.
// -c       : run_files and run_table with a covariates file (read_covariates): its rows are checked on the host, subset with
//            everything else and handed to the session (set_covariates); the log gains two lines.
// --pattern_cache: run_table with cache_mib > 0 goes through test_table_unique; the same .assoc.txt, six more lines in the log.
// --pattern_skip: run_table_multi with cache_mib > 0 goes through test_table_multi_skip; the same files, seven more lines in the logs.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "fdist_tail.h"
#include "kernels.h"
#include "lmm_internal.h"
#include "table_session.h"

using namespace kgwas;
using namespace kgwas::lmm;

namespace {

std::vector<std::string> read_lines(const std::string& path, const char* what) {
    std::ifstream f(path);
    if (!f.is_open()) throw Error(KGWAS_ERR_IO, std::string("can't open ") + what + " file: " + path);
    std::vector<std::string> lines;
    for (std::string l; std::getline(f, l);)
        if (l.find_first_not_of(" \t\r") != std::string::npos) lines.push_back(l);
    return lines;
}

}  // namespace

std::vector<double> kgwas::lmm::read_kinship(const std::string& path, uint64_t n_expected, const char* counted_in) {
    const std::vector<std::string> lines = read_lines(path, "kinship");
    if (lines.size() != n_expected)
        throw Error(KGWAS_ERR_FORMAT, "kinship file " + path + " has " + std::to_string(lines.size()) + " rows, " + counted_in + " has " +
                                          std::to_string(n_expected) + " individuals");
    std::vector<double> K(n_expected * n_expected);
    for (uint64_t r = 0; r < n_expected; r++) {
        const char* s = lines[r].c_str();
        uint64_t c = 0;
        for (;; c++) {
            char* end = nullptr;
            const double v = strtod(s, &end);
            if (end == s) break;
            if (c < n_expected) K[r * n_expected + c] = v;
            s = end;
        }
        while (*s == ' ' || *s == '\t' || *s == '\r') s++;
        if (*s) throw Error(KGWAS_ERR_FORMAT, "kinship file " + path + ": row " + std::to_string(r + 1) + " holds text that is no number");
        if (c != n_expected)
            throw Error(KGWAS_ERR_FORMAT, "kinship file " + path + ": row " + std::to_string(r + 1) + " has " + std::to_string(c) +
                                              " values, expected " + std::to_string(n_expected));
    }
    return K;
}

void kgwas::lmm::read_covariates(const std::string& path, std::vector<double>& values, std::vector<uint8_t>& keep, uint32_t& q) {
    const std::vector<std::string> lines = read_lines(path, "covariates");
    if (lines.empty()) throw Error(KGWAS_ERR_FORMAT, "covariates file " + path + " has no rows");
    q = 0;
    values.clear();
    keep.assign(lines.size(), 1);
    for (size_t r = 0; r < lines.size(); r++) {
        const std::vector<std::string> f = fields_of(lines[r]);
        if (r == 0) {
            if (f.size() > LMM_MAXC)
                throw Error(KGWAS_ERR_FORMAT, "covariates file " + path + " has " + std::to_string(f.size()) + " columns; at most " +
                                                  std::to_string(LMM_MAXC) + " are built");
            q = (uint32_t)f.size();
        } else if (f.size() != q) {
            throw Error(KGWAS_ERR_FORMAT, "covariates file " + path + ": row " + std::to_string(r + 1) + " has " + std::to_string(f.size()) +
                                              " fields, row 1 has " + std::to_string(q));
        }
        for (const std::string& t : f) {
            double v = std::nan("");
            if (t == "NA") {
                keep[r] = 0;
            } else {
                char* end = nullptr;
                v = strtod(t.c_str(), &end);
                if (end == t.c_str() || *end || !std::isfinite(v))
                    throw Error(KGWAS_ERR_FORMAT, "covariates file " + path + ": row " + std::to_string(r + 1) + ": '" + t + "' is no number");
            }
            values.push_back(v);
        }
    }
}

namespace {

// the covariates of a run: the file's rows, and the rows of the individuals idx as set_covariates takes them (checked on the host)
struct Covariates {
    std::string path;
    uint32_t q = 0;
    std::vector<double> values;
    std::vector<uint8_t> keep;
    void load(const char* p, uint64_t rows_expected, const char* counted_in) {
        path = p;
        read_covariates(path, values, keep, q);
        if (keep.size() != rows_expected)
            throw Error(KGWAS_ERR_FORMAT, "covariates file " + path + " has " + std::to_string(keep.size()) + " rows, " + counted_in + " has " +
                                              std::to_string(rows_expected) + " individuals");
    }
    // The rows as given, after orthonormal_covariates has accepted them. Its basis and log |det R| are discarded on purpose:
    // set_covariates makes them again once the handle exists; this call is only there to refuse before the kinship file is read.
    std::vector<double> checked_rows_of(const std::vector<uint32_t>& idx) const {
        std::vector<double> W(idx.size() * q);
        for (size_t r = 0; r < idx.size(); r++)
            for (uint32_t j = 0; j < q; j++) W[r * q + j] = values[(uint64_t)idx[r] * q + j];
        std::vector<double> Qw;
        double log_det_R;
        orthonormal_covariates(idx.size(), q, W.data(), Qw, log_det_R, "covariates file " + path);
        return W;
    }
};

// a phenotype field as a .fam gives it: "-9" and "NA" are missing, anything else must be one finite number
enum class Pheno { missing, number, no_number };
Pheno parse_phenotype(const std::string& t, double& v) {
    if (t == "-9" || t == "NA") return Pheno::missing;
    char* end = nullptr;
    v = strtod(t.c_str(), &end);
    return end == t.c_str() || *end || !std::isfinite(v) ? Pheno::no_number : Pheno::number;
}

// values[i] and keep[i] of every .fam line; the phenotype is field 5 + pheno_col (1-based)
void read_fam(const std::string& path, uint32_t pheno_col, std::vector<double>& values, std::vector<uint8_t>& keep) {
    if (pheno_col < 1) throw Error(KGWAS_ERR_ARG, "the phenotype column (-n) starts at 1");
    const std::vector<std::string> lines = read_lines(path, "fam");
    values.assign(lines.size(), std::nan(""));
    keep.assign(lines.size(), 0);
    for (size_t i = 0; i < lines.size(); i++) {
        const std::vector<std::string> f = fields_of(lines[i]);
        if (f.size() < 5u + pheno_col)
            throw Error(KGWAS_ERR_FORMAT, path + ": line " + std::to_string(i + 1) + " has no phenotype column " + std::to_string(pheno_col));
        const std::string& t = f[4 + pheno_col];
        double v = 0;
        const Pheno kind = parse_phenotype(t, v);
        if (kind == Pheno::missing) continue;
        if (kind == Pheno::no_number)
            throw Error(KGWAS_ERR_FORMAT, path + ": line " + std::to_string(i + 1) + ": phenotype '" + t + "' is no number");
        values[i] = v;
        keep[i] = 1;
    }
}

// One line of an .assoc.txt (chr = null: the header): columns 1-7, then every column of cols, a number as %.6e. `limit` is the
// length a line is refused at.
struct AssocColumn {
    const char* name;
    double value;
};
uint64_t format_line(const char* chr, const char* rs, const char* ps, uint32_t n_miss, const char* a1, const char* a0, double af,
                     const AssocColumn* cols, size_t n_cols, size_t limit, char* out, uint64_t cap) {
    char buf[1280];
    int len = chr ? snprintf(buf, limit, "%s\t%s\t%s\t%u\t%s\t%s\t%.3f", chr, rs, ps, n_miss, a1, a0, af)
                  : snprintf(buf, limit, "chr\trs\tps\tn_miss\tallele1\tallele0\taf");
    for (size_t k = 0; k <= n_cols && len >= 0 && (size_t)len < limit; k++) {  // (k = n_cols: the end of the line)
        const int m = k == n_cols ? snprintf(buf + len, limit - len, "\n")
                      : chr       ? snprintf(buf + len, limit - len, "\t%.6e", cols[k].value)
                                  : snprintf(buf + len, limit - len, "\t%s", cols[k].name);
        len = m < 0 ? m : len + m;
    }
    if (len < 0 || (size_t)len >= limit) throw Error(KGWAS_ERR_FORMAT, "a .bim line is too long");
    if (out && cap >= (uint64_t)len) memcpy(out, buf, (size_t)len);
    return (uint64_t)len;
}

uint64_t format_assoc(const char* chr, const char* rs, const char* ps, uint32_t n_miss, const char* a1, const char* a0, double af,
                      double l_mle, double p, char* out, uint64_t cap) {
    const AssocColumn cols[] = {{"l_mle", l_mle}, {"p_lrt", p}};
    return format_line(chr, rs, ps, n_miss, a1, a0, af, cols, 2, 1024, out, cap);
}

// the -lmm 4 line: columns 1-7, l_mle and p_lrt with the bytes of format_assoc's
uint64_t format_assoc4(const char* chr, const char* rs, const char* ps, uint32_t n_miss, const char* a1, const char* a0, double af,
                       double beta, double se, double l_remle, double l_mle, double p_wald, double p_lrt, double p_score, char* out,
                       uint64_t cap) {
    const AssocColumn cols[] = {{"beta", beta},     {"se", se},       {"l_remle", l_remle}, {"l_mle", l_mle},
                                {"p_wald", p_wald}, {"p_lrt", p_lrt}, {"p_score", p_score}};
    return format_line(chr, rs, ps, n_miss, a1, a0, af, cols, 7, 1280, out, cap);
}

std::string log_path_of(const std::string& out) {
    const std::string suf = ".assoc.txt";
    if (out.size() >= suf.size() && out.compare(out.size() - suf.size(), suf.size(), suf) == 0)
        return out.substr(0, out.size() - suf.size()) + ".log.txt";
    return out + ".log.txt";
}

void add_stats(kgwas_lmm_stats& a, const kgwas_lmm_stats& b) {
    a.eigen_ms += b.eigen_ms;
    a.rotate_ms += b.rotate_ms;
    a.grid_ms += b.grid_ms;
    a.refine_ms += b.refine_ms;
    a.variants_read += b.variants_read;
    a.variants_tested += b.variants_tested;
    a.chunks += b.chunks;
    a.eigendecompositions += b.eigendecompositions;
    a.n_individuals = b.n_individuals;
}

// ---- what run_files and run_file_multi share ----

std::vector<uint32_t> kept_lines(const std::vector<uint8_t>& keep) {
    std::vector<uint32_t> idx;
    for (uint64_t i = 0; i < keep.size(); i++)
        if (keep[i]) idx.push_back((uint32_t)i);
    return idx;
}

kgwas_lmm* create_for_kept(const std::vector<double>& Kfull, uint64_t nf, const std::vector<uint32_t>& idx, int device, double lmin,
                           double lmax, uint64_t chunk_variants) {
    const uint64_t n = idx.size();
    std::vector<double> K(n * n);
    for (uint64_t r = 0; r < n; r++)
        for (uint64_t c = 0; c < n; c++) K[r * n + c] = Kfull[(uint64_t)idx[r] * nf + idx[c]];
    return create(n, K.data(), device, lmin, lmax, chunk_variants);
}

// the .bim lines and the .bed body of <base>, the latter with the codes of the kept individuals idx (of nf .fam lines) alone
void read_bim_bed(const std::string& base, uint64_t nf, const std::vector<uint32_t>& idx, std::vector<std::string>& bim,
                  std::vector<uint8_t>& body) {
    bim = read_lines(base + ".bim", "bim");
    const uint64_t n = idx.size(), M = bim.size(), bps_f = (nf + 3) / 4, bps = (n + 3) / 4;
    {
        std::ifstream f(base + ".bed", std::ios::binary | std::ios::ate);
        if (!f.is_open()) throw Error(KGWAS_ERR_IO, "can't open bed file: " + base + ".bed");
        const uint64_t size = (uint64_t)f.tellg();
        if (size != 3 + M * bps_f)
            throw Error(KGWAS_ERR_FORMAT, base + ".bed has " + std::to_string(size) + " bytes, " + std::to_string(M) + " variants of " +
                                              std::to_string(nf) + " individuals need " + std::to_string(3 + M * bps_f));
        f.seekg(0);
        uint8_t magic[3];
        f.read((char*)magic, 3);
        if (magic[0] != 0x6C || magic[1] != 0x1B || magic[2] != 0x01)
            throw Error(KGWAS_ERR_FORMAT, base + ".bed: not a SNP-major PLINK .bed (magic 6C 1B 01)");
        body.resize(M * bps_f);
        f.read((char*)body.data(), (std::streamsize)body.size());
        if (!f) throw Error(KGWAS_ERR_IO, "short read of " + base + ".bed");
    }
    if (n != nf) {  // the kept individuals' codes, packed again
        std::vector<uint8_t> packed(M * bps, 0);
        for (uint64_t v = 0; v < M; v++) {
            const uint8_t* src = &body[v * bps_f];
            uint8_t* dst = &packed[v * bps];
            for (uint64_t r = 0; r < n; r++) dst[r >> 2] |= (uint8_t)(((src[idx[r] >> 2] >> (2 * (idx[r] & 3))) & 3) << (2 * (r & 3)));
        }
        body.swap(packed);
    }
}

std::string assoc_header(bool all_tests = false) {
    char line[1280];
    return std::string(line, all_tests ? format_assoc4(nullptr, "", "", 0, "", "", 0, 0, 0, 0, 0, 0, 0, 0, line, sizeof(line))
                                       : format_assoc(nullptr, "", "", 0, "", "", 0, 0, 0, line, sizeof(line)));
}

// the fields of the .bim lines of the tested ones among variants first .. first + cnt (tested starts at `first`; the others stay empty)
std::vector<std::vector<std::string>> bim_fields(const std::string& base, const std::vector<std::string>& bim, uint64_t first, uint64_t cnt,
                                                 const uint8_t* tested) {
    std::vector<std::vector<std::string>> fields(cnt);
    for (uint64_t v = 0; v < cnt; v++) {
        if (!tested[v]) continue;
        fields[v] = fields_of(bim[first + v]);
        if (fields[v].size() < 6)
            throw Error(KGWAS_ERR_FORMAT, base + ".bim: line " + std::to_string(first + v + 1) + " has fewer than 6 fields");
    }
    return fields;
}

// -lmm 4's five further columns of a .bed pass
struct WaldColumns {
    std::vector<double> beta, se, lam, p_wald, p_score;
    explicit WaldColumns(uint64_t m) : beta(m), se(m), lam(m), p_wald(m), p_score(m) {}
    WaldArrays arrays() { return {beta.data(), se.data(), lam.data(), p_wald.data(), p_score.data()}; }
};

// appends the lines of the tested ones among fields.size() variants (all arrays start at the first of them), the 14-column lines
// of -lmm 4 with w; returns their number
uint64_t append_assoc(std::string& text, const std::vector<std::vector<std::string>>& fields, const uint32_t* n_miss, const double* af,
                      const double* lam, const double* p, const uint8_t* tested, const WaldColumns* w = nullptr) {
    uint64_t n_tested = 0;
    for (uint64_t v = 0; v < fields.size(); v++) {
        if (!tested[v]) continue;
        const std::vector<std::string>& f = fields[v];
        const char *chr = f[0].c_str(), *rs = f[1].c_str(), *ps = f[3].c_str(), *a1 = f[4].c_str(), *a0 = f[5].c_str();
        char line[1280];
        const uint64_t len = w ? format_assoc4(chr, rs, ps, n_miss[v], a1, a0, af[v], w->beta[v], w->se[v], w->lam[v], lam[v], w->p_wald[v],
                                               p[v], w->p_score[v], line, sizeof(line))
                               : format_assoc(chr, rs, ps, n_miss[v], a1, a0, af[v], lam[v], p[v], line, sizeof(line));
        text.append(line, len);
        n_tested++;
    }
    return n_tested;
}

// the log beside `out`: what snprintf left in log[cap], ll being its return value
void write_log_text(const std::string& out, const char* log, size_t cap, int ll) {
    if (ll < 0) throw Error(KGWAS_ERR_IO, "can't write " + log_path_of(out));
    write_text(log_path_of(out), std::string(log, std::min((size_t)ll, cap - 1)), "wb");
}

// the two lines a log gains behind `kinship` with -c (nothing without)
std::string covariate_lines(const Covariates* cov) {
    return cov ? "covariates\t" + cov->path + "\nn_covariates\t" + std::to_string(cov->q) + "\n" : std::string();
}

// the log of a .bed pass; with reml (-lmm 4: a handle whose REML null model is fitted) under the other title, with that model's
// four lines behind logl_H0
void write_log(const std::string& out, const std::string& base, const char* kinship_path, uint64_t nf, uint64_t n, uint64_t M,
               uint64_t n_tested, double lambda0, double l0, double eigen_ms, double rotate_ms, double grid_ms, double refine_ms,
               double total_ms, const Covariates* cov = nullptr, const kgwas_lmm* reml = nullptr) {
    char log[2304], reml_lines[1024] = "";
    if (reml)
        snprintf(reml_lines, sizeof(reml_lines), "lambda0_remle\t%.6e\nlogl_remle_H0\t%.6f\nvg\t%.6e\nve\t%.6e\n", reml->lambda0_reml,
                 reml->l0_reml, reml->vg, reml->ve);
    const size_t cap = reml ? sizeof(log) : 2048;  // (where each of the two logs is cut)
    const int ll = snprintf(log, cap,
                            "lmm_lrt: ML likelihood-ratio test%s\nbfile\t%s\nkinship\t%s\n%sindividuals_in_fam\t%llu\n"
                            "individuals_used\t%llu\nvariants_read\t%llu\nvariants_tested\t%llu\nlambda0\t%.6e\nlogl_H0\t%.6f\n%s"
                            "ms: eigen=%.3f rotate=%.3f grid=%.3f refine=%.3f total=%.3f\n",
                            reml ? ", REML Wald test and score test (-lmm 4)" : " (-lmm 2)", base.c_str(), kinship_path,
                            covariate_lines(cov).c_str(), (unsigned long long)nf, (unsigned long long)n, (unsigned long long)M,
                            (unsigned long long)n_tested, lambda0, l0, reml_lines, eigen_ms, rotate_ms, grid_ms, refine_ms, total_ms);
    write_log_text(out, log, cap, ll);
}

void run_files(const char* kinship_path, uint64_t n_beds, const char* const* bases, const char* const* outs, uint32_t pheno_col,
               double maf, double miss, double lmin, double lmax, uint64_t chunk_variants, int device, kgwas_lmm_stats* total,
               bool all_tests = false, const char* covar_path = nullptr) {
    if (!kinship_path || (n_beds && (!bases || !outs)))
        throw Error(KGWAS_ERR_ARG, std::string(all_tests ? "kgwas_lmm_run_files_all" : "kgwas_lmm_run_files") + ": null argument");
    kgwas_lmm_stats sum{};
    Covariates cov_file;  // -c: read at the first .fam, whose lines its rows follow
    const Covariates* cov = covar_path ? &cov_file : nullptr;
    std::vector<double> Kfull;
    Handle h;
    std::vector<uint8_t> keep_cur;
    for (uint64_t b = 0; b < n_beds; b++) {
        const std::string base = bases[b], out = outs[b];
        const double t_start = now_ms();
        std::vector<double> vals;
        std::vector<uint8_t> keep;
        read_fam(base + ".fam", pheno_col, vals, keep);
        const uint64_t nf = vals.size();
        if (cov) {  // an individual is used iff its phenotype is present and no covariate is NA
            if (cov_file.keep.size() != nf) cov_file.load(covar_path, nf, "the .fam");
            for (uint64_t i = 0; i < nf; i++) keep[i] &= cov_file.keep[i];
        }
        const std::vector<uint32_t> idx = kept_lines(keep);
        const uint64_t n = idx.size();
        std::vector<double> W;
        if (cov && (!h || keep != keep_cur)) W = cov_file.checked_rows_of(idx);  // (refused here, before the kinship file and the device)
        if (Kfull.empty() || Kfull.size() != nf * nf) Kfull = read_kinship(kinship_path, nf);
        if (!h || keep != keep_cur) {
            if (h) add_stats(sum, h->st);
            h.reset();
            h.reset(create_for_kept(Kfull, nf, idx, device, lmin, lmax, chunk_variants));
            if (cov) set_covariates(h.get(), cov_file.q, W.data());
            keep_cur = keep;
        }
        std::vector<double> y(n);
        for (uint64_t r = 0; r < n; r++) y[r] = vals[idx[r]];
        std::vector<std::string> bim;
        std::vector<uint8_t> body;
        read_bim_bed(base, nf, idx, bim, body);
        const uint64_t M = bim.size();
        std::vector<double> lrt(M), lam(M), p(M), af(M);
        std::vector<uint32_t> n_miss(M);
        std::vector<uint8_t> tested(M);
        const kgwas_lmm_stats before = h->st;
        std::unique_ptr<WaldColumns> w;  // -lmm 4
        WaldArrays wa{};
        if (all_tests) {
            w.reset(new WaldColumns(M));
            wa = w->arrays();
            fit_null_reml(h.get(), y.data());
        }
        test_bed(h.get(), y.data(), body.data(), M, maf, miss, lrt.data(), lam.data(), p.data(), af.data(), n_miss.data(), tested.data(),
                 w ? &wa : nullptr);
        std::string text = assoc_header(all_tests);
        const uint64_t n_tested = append_assoc(text, bim_fields(base, bim, 0, M, tested.data()), n_miss.data(), af.data(), lam.data(),
                                               p.data(), tested.data(), w.get());
        write_text(out, text, "wb");
        write_log(out, base, kinship_path, nf, n, M, n_tested, h->lambda0, h->l0, h->st.eigen_ms, h->st.rotate_ms - before.rotate_ms,
                  h->st.grid_ms - before.grid_ms, h->st.refine_ms - before.refine_ms, now_ms() - t_start, cov, w ? h.get() : nullptr);
    }
    if (h) add_stats(sum, h->st);
    if (total) *total = sum;
}

// One bfile, n_cols phenotype columns of its .fam with one missing set: the .bed, the .bim and the kinship matrix are read once,
// K is eigendecomposed once, and every chunk of variants goes through the multi-phenotype pass. Results are written in slabs
// of variants, so that the [column][variant] arrays stay small for a panel of millions of variants.
void run_file_multi(const char* kinship_path, const char* bfile_base, uint32_t n_cols, const uint32_t* cols, const char* const* outs,
                    double maf, double miss, double lmin, double lmax, uint64_t chunk_variants, int device, kgwas_lmm_stats* total) {
    if (!kinship_path || !bfile_base || !cols || !outs) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_run_file_multi: null argument");
    if (!n_cols) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_run_file_multi: no phenotype column given");
    const std::string base = bfile_base;
    const double t_start = now_ms();
    std::vector<std::vector<double>> vals(n_cols);
    std::vector<uint8_t> keep;
    for (uint32_t k = 0; k < n_cols; k++) {
        std::vector<uint8_t> keep_k;
        read_fam(base + ".fam", cols[k], vals[k], keep_k);
        if (k == 0)
            keep = keep_k;
        else if (keep_k != keep)
            throw Error(KGWAS_ERR_FORMAT, base + ".fam: phenotype column " + std::to_string(cols[k]) + " marks other individuals as missing than column " +
                                              std::to_string(cols[0]) + "; columns of one run must share their missing set");
    }
    const uint64_t nf = keep.size();
    const std::vector<double> Kfull = read_kinship(kinship_path, nf);
    const std::vector<uint32_t> idx = kept_lines(keep);
    const uint64_t n = idx.size();
    Handle h(create_for_kept(Kfull, nf, idx, device, lmin, lmax, chunk_variants));
    std::vector<double> Y((uint64_t)n_cols * n);
    for (uint32_t k = 0; k < n_cols; k++)
        for (uint64_t r = 0; r < n; r++) Y[k * n + r] = vals[k][idx[r]];
    std::vector<std::string> bim;
    std::vector<uint8_t> body;
    read_bim_bed(base, nf, idx, bim, body);
    const uint64_t M = bim.size(), bps = (n + 3) / 4;
    std::vector<double> l0(n_cols), lambda0(n_cols);
    multi_prepare(h.get(), n_cols, Y.data(), l0.data(), lambda0.data());
    for (uint32_t k = 0; k < n_cols; k++) write_text(outs[k], assoc_header(), "wb");
    // a slab: whole chunks, about 4 M (variant, column) pairs
    const uint64_t slab = std::max<uint64_t>(1, (1u << 22) / ((uint64_t)n_cols * h->chunk)) * h->chunk;
    std::vector<double> lrt(std::min(slab, M) * n_cols), lam(lrt.size()), p(lrt.size()), af(std::min(slab, M));
    std::vector<uint32_t> n_miss(af.size());
    std::vector<uint8_t> tested(af.size());
    std::vector<uint64_t> n_tested(n_cols, 0);
    for (uint64_t first = 0; first < M; first += slab) {
        const uint64_t cnt = std::min(slab, M - first);
        multi_run(h.get(), n_cols, body.data() + first * bps, cnt, maf, miss, lrt.data(), lam.data(), p.data(), af.data(), n_miss.data(),
                  tested.data());
        const std::vector<std::vector<std::string>> fields = bim_fields(base, bim, first, cnt, tested.data());  // once for all columns
        for (uint32_t k = 0; k < n_cols; k++) {
            std::string text;
            n_tested[k] += append_assoc(text, fields, n_miss.data(), af.data(), &lam[k * cnt], &p[k * cnt], tested.data());
            write_text(outs[k], text, "ab");
        }
    }
    const double total_ms = now_ms() - t_start;
    for (uint32_t k = 0; k < n_cols; k++)  // (the kernels' times are the shared pass's, the same in every column's log)
        write_log(outs[k], base, kinship_path, nf, n, M, n_tested[k], lambda0[k], l0[k], h->st.eigen_ms, h->st.rotate_ms, h->st.grid_ms,
                  h->st.refine_ms, total_ms);
    if (total) *total = h->st;
}

// ---- what run_table and run_table_multi share ----

// The inputs of lmm_lrt --kmers_table, each read once: the phenotype file (its accessions, in its order, are the individuals), the
// open table with its column map, the kinship text.
struct TableRun : TableSession {
    uint64_t min_count = 0;
    const float* Y = nullptr;
    std::vector<double> K;
    void need_column(uint32_t pheno_col) const {
        if (pheno_col > n_pheno) throw Error(KGWAS_ERR_FORMAT, pheno_path + " has no phenotype column " + std::to_string(pheno_col));
    }
    void load_values() { ck(kgwas_pheno_values(ph, &Y)); }
    // y as it would arrive through kmers_table_to_bed's .fam: the loader's float in ostream's default format, parsed as read_fam does
    void column(uint32_t pheno_col, double* y) const {
        for (uint64_t i = 0; i < S; i++) {
            std::ostringstream os;
            os << Y[(uint64_t)(pheno_col - 1) * S + i];
            const std::string text = os.str();
            const Pheno kind = parse_phenotype(text, y[i]);
            if (kind == Pheno::missing)
                throw Error(KGWAS_ERR_FORMAT, pheno_path + ": the phenotype of " + acc[i] + " is " + text +
                                                  ", which a .fam reads as missing; remove the accession from the phenotype file");
            if (kind == Pheno::no_number)
                throw Error(KGWAS_ERR_FORMAT, pheno_path + ": phenotype '" + text + "' of " + acc[i] + " is no number");
        }
    }
    void open_table(const char* table_base, uint32_t kmer_len, const char* kinship_path, double maf, uint64_t mac) {
        TableSession::open_table(table_base, kmer_len);
        check_squeeze_fits("lmm_lrt --kmers_table");
        K = read_kinship(kinship_path, S, "the phenotype file");
        min_count = kgwas_min_count(S, maf, mac);
    }
};

// one column's kept k-mers to `out` in table order, with the bytes run_files writes for them after kmers_table_to_bed, and the log
void write_table_result(const std::string& out, const std::vector<TableHit>& kept, const TableRun& r, const char* table_base,
                        uint32_t pheno_col, const char* kinship_path, uint64_t rows_read, uint64_t rows_tested, uint64_t best_n,
                        double lambda0, double l0, const kgwas_lmm_stats& st, double total_ms, const Covariates* cov = nullptr,
                        const kgwas_lmm_unique_stats* u = nullptr, const kgwas_lmm_skip_stats* skip = nullptr) {
    std::string text = assoc_header();
    for (const TableHit& k : kept) {
        char line[1024];  // (the k-mer's letters as in kmers_table_to_bed's .bim)
        const uint64_t len = format_assoc("0", kmer_letters(k.kmer, r.klen).c_str(), "0", 0, "0", "1", k.af, k.lam, k.p, line, sizeof(line));
        text.append(line, len);
    }
    write_text(out, text, "wb");
    char log[3584], cache_lines[512] = "";
    if (u)  // --pattern_cache: six lines behind the others
        snprintf(cache_lines, sizeof(cache_lines),
                 "pattern_cache_slots\t%llu\npatterns_cached\t%llu\nrows_from_cache\t%llu\nrows_collided\t%llu\nrows_rejected\t%llu\n"
                 "rows_rotated\t%llu\n",
                 (unsigned long long)u->slots, (unsigned long long)u->patterns_cached, (unsigned long long)u->rows_from_cache,
                 (unsigned long long)u->rows_collided, (unsigned long long)u->rows_rejected, (unsigned long long)u->rows_rotated);
    if (skip)  // --pattern_skip: seven lines behind the others
        snprintf(cache_lines, sizeof(cache_lines),
                 "pattern_skip_slots\t%llu\npatterns_cached\t%llu\npatterns_dead\t%llu\nrows_skipped\t%llu\nrows_collided\t%llu\n"
                 "rows_rejected\t%llu\nrows_rotated\t%llu\n",
                 (unsigned long long)skip->slots, (unsigned long long)skip->patterns_cached, (unsigned long long)skip->patterns_dead,
                 (unsigned long long)skip->rows_skipped, (unsigned long long)skip->rows_collided, (unsigned long long)skip->rows_rejected,
                 (unsigned long long)skip->rows_rotated);
    const int ll = snprintf(log, sizeof(log),
                            "lmm_lrt: ML likelihood-ratio test (-lmm 2)\nkmers_table\t%s\nphenotypes\t%s\nphenotype_column\t%u\nkinship\t%s\n%s"
                            "individuals_used\t%llu\nmin_count\t%llu\nrows_read\t%llu\nrows_tested\t%llu\nrows_kept\t%llu\nbest_n\t%llu\n"
                            "lambda0\t%.6e\nlogl_H0\t%.6f\nms: eigen=%.3f rotate=%.3f grid=%.3f refine=%.3f total=%.3f\n%s",
                            table_base, r.pheno_path.c_str(), pheno_col, kinship_path, covariate_lines(cov).c_str(), (unsigned long long)r.S,
                            (unsigned long long)r.min_count,
                            (unsigned long long)rows_read, (unsigned long long)rows_tested, (unsigned long long)kept.size(),
                            (unsigned long long)best_n, lambda0, l0, st.eigen_ms, st.rotate_ms, st.grid_ms, st.refine_ms, total_ms,
                            cache_lines);
    write_log_text(out, log, sizeof(log), ll);
}

// The file layer of lmm_lrt --kmers_table: the accessions and their order are the phenotype file's, y its column pheno_col (from
// 1), the k-mers come straight from <table_base>.table. The best best_n k-mers by the exact test go to `out` in table order, with
// the bytes run_files writes for them after kmers_table_to_bed; a log goes beside it. With cache_mib > 0 the pass is
// test_table_unique's with a pattern cache of that many MiB: the same bytes in `out`, six more lines in the log, *u the counters.
void run_table(const char* kinship_path, const char* table_base, uint32_t kmer_len, const char* pheno_path, uint32_t pheno_col,
               uint64_t mac, double maf, uint64_t best_n, double lmin, double lmax, uint64_t chunk_variants, int device, const char* out,
               kgwas_lmm_stats* total, const char* covar_path = nullptr, uint64_t cache_mib = 0, kgwas_lmm_unique_stats* u = nullptr) {
    if (!kinship_path || !table_base || !pheno_path || !out) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_run_table: null argument");
    if (pheno_col < 1) throw Error(KGWAS_ERR_ARG, "the phenotype column (-n) starts at 1");
    if (!best_n) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_run_table: best_n is 0");
    const double t_start = now_ms();
    TableRun r;
    r.load_pheno(pheno_path);
    r.need_column(pheno_col);
    r.load_values();
    std::vector<double> y(r.S);
    r.column(pheno_col, y.data());
    Covariates cov_file;  // -c: one row per accession, none missing; refused before the table, the kinship file and the device
    const Covariates* cov = covar_path ? &cov_file : nullptr;
    std::vector<double> W;
    if (cov) {
        cov_file.load(covar_path, r.S, "the phenotype file");
        std::vector<uint32_t> all(r.S);
        for (uint64_t i = 0; i < r.S; i++) {
            if (!cov_file.keep[i])
                throw Error(KGWAS_ERR_FORMAT, "covariates file " + cov_file.path + ": row " + std::to_string(i + 1) +
                                                  " has an NA; with --kmers_table remove the accession from the phenotype file");
            all[i] = (uint32_t)i;
        }
        W = cov_file.checked_rows_of(all);
    }
    r.open_table(table_base, kmer_len, kinship_path, maf, mac);
    Handle h(create(r.S, r.K.data(), device, lmin, lmax, chunk_variants));
    if (cov) set_covariates(h.get(), cov_file.q, W.data());
    std::vector<TableHit> kept;
    uint64_t rows_read = 0, rows_tested = 0;
    kgwas_lmm_unique_stats us{};
    if (cache_mib)  // as many slots as the bytes hold (test_table_unique takes a power of two, and refuses fewer than 64)
        test_table_unique(h.get(), y.data(), r.t, r.col.data(), r.S, r.min_count, maf, best_n,
                          std::min<uint64_t>(cache_mib, 1ull << 40) * (1ull << 20) / lmm_cache_slot_bytes(h->dm), kept, rows_read, rows_tested, us);
    else
        test_table(h.get(), y.data(), r.t, r.col.data(), r.S, r.min_count, maf, best_n, kept, rows_read, rows_tested);
    write_table_result(out, kept, r, table_base, pheno_col, kinship_path, rows_read, rows_tested, best_n, h->lambda0, h->l0, h->st,
                       now_ms() - t_start, cov, cache_mib ? &us : nullptr);
    if (total) *total = h->st;
    if (u && cache_mib) *u = us;
}

// The same for n_cols columns of the phenotype file (pheno_cols, from 1) in ONE pass over the table: the files are read once, K is
// eigendecomposed once, and outs[k] with its log gets what run_table writes for column pheno_cols[k] (the kernels' times are the
// shared pass's, the same in every column's log). With cache_mib > 0 the pass is test_table_multi_skip's with a table of that many
// MiB: the same bytes in the files, seven more lines in every log, *u the counters.
void run_table_multi(const char* kinship_path, const char* table_base, uint32_t kmer_len, const char* pheno_path, uint32_t n_cols,
                     const uint32_t* cols, const char* const* outs, uint64_t mac, double maf, uint64_t best_n, double lmin, double lmax,
                     uint64_t chunk_variants, int device, kgwas_lmm_stats* total, uint64_t cache_mib = 0, kgwas_lmm_skip_stats* u = nullptr) {
    if (!kinship_path || !table_base || !pheno_path || !cols || !outs) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_run_table_multi: null argument");
    if (!n_cols) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_run_table_multi: no phenotype column given");
    for (uint32_t k = 0; k < n_cols; k++) {
        if (!outs[k]) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_run_table_multi: null argument");
        if (cols[k] < 1) throw Error(KGWAS_ERR_ARG, "phenotype columns start at 1");
    }
    if (!best_n) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_run_table_multi: best_n is 0");
    const double t_start = now_ms();
    TableRun r;
    r.load_pheno(pheno_path);
    for (uint32_t k = 0; k < n_cols; k++) r.need_column(cols[k]);
    r.load_values();
    std::vector<double> Y((uint64_t)n_cols * r.S);
    for (uint32_t k = 0; k < n_cols; k++) r.column(cols[k], &Y[k * r.S]);
    r.open_table(table_base, kmer_len, kinship_path, maf, mac);
    Handle h(create(r.S, r.K.data(), device, lmin, lmax, chunk_variants));
    std::vector<std::vector<TableHit>> kept;
    std::vector<double> l0(n_cols), lambda0(n_cols);
    uint64_t rows_read = 0, rows_tested = 0, shipped = 0;
    kgwas_lmm_skip_stats ks{};
    if (cache_mib)  // as many slots as the bytes hold (test_table_multi_skip takes a power of two, and refuses fewer than 64)
        test_table_multi_skip(h.get(), n_cols, Y.data(), r.t, r.col.data(), r.S, r.min_count, maf, best_n,
                              std::min<uint64_t>(cache_mib, 1ull << 40) * (1ull << 20) / lmm_skip_slot_bytes(h->dm), kept, l0.data(),
                              lambda0.data(), rows_read, rows_tested, shipped, ks);
    else
        test_table_multi(h.get(), n_cols, Y.data(), r.t, r.col.data(), r.S, r.min_count, maf, best_n, kept, l0.data(), lambda0.data(),
                         rows_read, rows_tested, shipped);
    const double total_ms = now_ms() - t_start;
    for (uint32_t k = 0; k < n_cols; k++)
        write_table_result(outs[k], kept[k], r, table_base, cols[k], kinship_path, rows_read, rows_tested, best_n, lambda0[k], l0[k], h->st,
                           total_ms, nullptr, nullptr, cache_mib ? &ks : nullptr);
    if (total) *total = h->st;
    if (u && cache_mib) *u = ks;
}

}  // namespace

extern "C" {

int kgwas_lmm_run_files(const char* kinship_path, uint64_t n_beds, const char* const* bfile_bases, const char* const* out_paths,
                        uint32_t pheno_col, double maf, double miss, double lmin, double lmax, uint64_t chunk_variants, int32_t device,
                        kgwas_lmm_stats* total) {
    return guarded([&] { run_files(kinship_path, n_beds, bfile_bases, out_paths, pheno_col, maf, miss, lmin, lmax, chunk_variants, device, total); });
}

int kgwas_lmm_run_files_all(const char* kinship_path, uint64_t n_beds, const char* const* bfile_bases, const char* const* out_paths,
                            uint32_t pheno_col, double maf, double miss, double lmin, double lmax, uint64_t chunk_variants, int32_t device,
                            kgwas_lmm_stats* total) {
    return guarded(
        [&] { run_files(kinship_path, n_beds, bfile_bases, out_paths, pheno_col, maf, miss, lmin, lmax, chunk_variants, device, total, true); });
}

int kgwas_lmm_run_file_multi(const char* kinship_path, const char* bfile_base, uint32_t n_cols, const uint32_t* pheno_cols,
                             const char* const* out_paths, double maf, double miss, double lmin, double lmax, uint64_t chunk_variants,
                             int32_t device, kgwas_lmm_stats* total) {
    return guarded([&] {
        run_file_multi(kinship_path, bfile_base, n_cols, pheno_cols, out_paths, maf, miss, lmin, lmax, chunk_variants, device, total);
    });
}

int kgwas_lmm_run_table(const char* kinship_path, const char* table_base, uint32_t kmer_len, const char* pheno_path, uint32_t pheno_col,
                        uint64_t mac, double maf, uint64_t best_n, double lmin, double lmax, uint64_t chunk_variants, int32_t device,
                        const char* out_path, kgwas_lmm_stats* total) {
    return guarded([&] {
        run_table(kinship_path, table_base, kmer_len, pheno_path, pheno_col, mac, maf, best_n, lmin, lmax, chunk_variants, device, out_path,
                  total);
    });
}

int kgwas_lmm_run_table_multi(const char* kinship_path, const char* table_base, uint32_t kmer_len, const char* pheno_path, uint32_t n_cols,
                              const uint32_t* pheno_cols, const char* const* out_paths, uint64_t mac, double maf, uint64_t best_n,
                              double lmin, double lmax, uint64_t chunk_variants, int32_t device, kgwas_lmm_stats* total) {
    return guarded([&] {
        run_table_multi(kinship_path, table_base, kmer_len, pheno_path, n_cols, pheno_cols, out_paths, mac, maf, best_n, lmin, lmax,
                        chunk_variants, device, total);
    });
}

int kgwas_lmm_run_files_cov(const char* kinship_path, const char* covar_path, uint64_t n_beds, const char* const* bfile_bases,
                            const char* const* out_paths, uint32_t pheno_col, double maf, double miss, double lmin, double lmax,
                            uint64_t chunk_variants, int32_t device, int32_t all_tests, kgwas_lmm_stats* total) {
    return guarded([&] {
        run_files(kinship_path, n_beds, bfile_bases, out_paths, pheno_col, maf, miss, lmin, lmax, chunk_variants, device, total, all_tests != 0,
                  covar_path);
    });
}

int kgwas_lmm_run_table_cov(const char* kinship_path, const char* covar_path, const char* table_base, uint32_t kmer_len,
                            const char* pheno_path, uint32_t pheno_col, uint64_t mac, double maf, uint64_t best_n, double lmin, double lmax,
                            uint64_t chunk_variants, int32_t device, const char* out_path, kgwas_lmm_stats* total) {
    return guarded([&] {
        run_table(kinship_path, table_base, kmer_len, pheno_path, pheno_col, mac, maf, best_n, lmin, lmax, chunk_variants, device, out_path,
                  total, covar_path);
    });
}

int kgwas_lmm_run_table_unique(const char* kinship_path, const char* covar_path, const char* table_base, uint32_t kmer_len,
                               const char* pheno_path, uint32_t pheno_col, uint64_t mac, double maf, uint64_t best_n, double lmin,
                               double lmax, uint64_t chunk_variants, int32_t device, const char* out_path, kgwas_lmm_stats* total,
                               uint64_t cache_mib, kgwas_lmm_unique_stats* u) {
    return guarded([&] {
        if (!cache_mib) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_run_table_unique: cache_mib is 0");
        run_table(kinship_path, table_base, kmer_len, pheno_path, pheno_col, mac, maf, best_n, lmin, lmax, chunk_variants, device, out_path,
                  total, covar_path, cache_mib, u);
    });
}

int kgwas_lmm_run_table_multi_skip(const char* kinship_path, const char* table_base, uint32_t kmer_len, const char* pheno_path,
                                   uint32_t n_cols, const uint32_t* pheno_cols, const char* const* out_paths, uint64_t mac, double maf,
                                   uint64_t best_n, double lmin, double lmax, uint64_t chunk_variants, int32_t device,
                                   kgwas_lmm_stats* total, uint64_t cache_mib, kgwas_lmm_skip_stats* u) {
    return guarded([&] {
        if (!cache_mib) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_run_table_multi_skip: cache_mib is 0");
        run_table_multi(kinship_path, table_base, kmer_len, pheno_path, n_cols, pheno_cols, out_paths, mac, maf, best_n, lmin, lmax,
                        chunk_variants, device, total, cache_mib, u);
    });
}

int kgwas_lmm_read_covariates(const char* path, uint64_t n_expected, uint64_t cap, double* values, uint8_t* keep, uint32_t* q_out) {
    return guarded([&] {
        if (!path || !q_out) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_read_covariates: null argument");
        std::vector<double> v;
        std::vector<uint8_t> k;
        uint32_t q = 0;
        read_covariates(path, v, k, q);
        if (n_expected && k.size() != n_expected)
            throw Error(KGWAS_ERR_FORMAT, std::string("covariates file ") + path + " has " + std::to_string(k.size()) + " rows, expected " +
                                              std::to_string(n_expected));
        *q_out = q;
        if (v.size() > cap) return;
        if (values) memcpy(values, v.data(), v.size() * sizeof(double));
        if (keep) memcpy(keep, k.data(), k.size());
    });
}

int kgwas_lmm_read_kinship(const char* path, uint64_t n_expected, double* K) {
    return guarded([&] {
        if (!path || !K) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_read_kinship: null argument");
        const std::vector<double> k = read_kinship(path, n_expected);
        memcpy(K, k.data(), k.size() * sizeof(double));
    });
}

int kgwas_lmm_read_fam(const char* path, uint32_t pheno_col, uint64_t cap, double* values, uint8_t* keep, uint64_t* n_lines) {
    return guarded([&] {
        if (!path || !n_lines) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_read_fam: null argument");
        std::vector<double> v;
        std::vector<uint8_t> k;
        read_fam(path, pheno_col, v, k);
        *n_lines = v.size();
        for (uint64_t i = 0; i < std::min<uint64_t>(cap, v.size()); i++) {
            if (values) values[i] = v[i];
            if (keep) keep[i] = k[i];
        }
    });
}

uint64_t kgwas_lmm_format_assoc(const char* chr, const char* rs, const char* ps, uint32_t n_miss, const char* allele1, const char* allele0,
                                double af, double l_mle, double p_lrt, char* out, uint64_t cap) {
    uint64_t need = 0;
    guarded([&] {
        if (chr && (!rs || !ps || !allele1 || !allele0)) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_format_assoc: null argument");
        need = format_assoc(chr, rs, ps, n_miss, allele1, allele0, af, l_mle, p_lrt, out, cap);
    });
    return need;
}

uint64_t kgwas_lmm_format_assoc4(const char* chr, const char* rs, const char* ps, uint32_t n_miss, const char* allele1, const char* allele0,
                                 double af, double beta, double se, double l_remle, double l_mle, double p_wald, double p_lrt, double p_score,
                                 char* out, uint64_t cap) {
    uint64_t need = 0;
    guarded([&] {
        if (chr && (!rs || !ps || !allele1 || !allele0)) throw Error(KGWAS_ERR_ARG, "kgwas_lmm_format_assoc4: null argument");
        need = format_assoc4(chr, rs, ps, n_miss, allele1, allele0, af, beta, se, l_remle, l_mle, p_wald, p_lrt, p_score, out, cap);
    });
    return need;
}

double kgwas_fdist_tail(double F, double df) { return kgwas::fdist_tail(F, df); }

}  // extern "C"
