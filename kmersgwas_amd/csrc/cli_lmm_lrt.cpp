// lmm_lrt — the mixed-model likelihood-ratio test of the variants of PLINK files, on GPU 0 (kgwas_lmm_*). A tool of this
// project that takes the GEMMA command line the pipeline issues (kmers_gwas.py:150-165),
//     lmm_lrt -bfile B -lmm 2 -k KINSHIP -outdir D -o NAME [-n i] [-maf f] [-miss f] [-lmin x] [-lmax x]
// and writes D/NAME.assoc.txt (chr rs ps n_miss allele1 allele0 af l_mle p_lrt; p_lrt is field 9, which functions.py reads)
// and D/NAME.log.txt. Its own addition: --bfiles LIST, a file of "bfile<TAB>name" lines that all run against one
// eigendecomposition of the kinship matrix; and --columns LIST (with -bfile), a file of "col<TAB>name" lines: the listed phenotype
// columns of B.fam are all tested in ONE pass over B.bed (the SNP branch's 101 GEMMA runs over one panel, kmers_gwas.py:193-223),
// output D/name.assoc.txt. Defaults of -maf, -miss, -lmin, -lmax and -outdir are GEMMA's. And, in place of -bfile,
//     lmm_lrt --kmers_table T --kmers_len K -p PHENO -lmm 2 -k KINSHIP [--mac M] [-maf f] [--best N] [-n i] [-outdir D] [-o NAME]
// the exact test of EVERY k-mer of the table T that kmers_table_to_bed (--mac M --maf f) would write and lmm_lrt (-maf f) would then
// test, without the PLINK files in between; the best N by the test are written, in table order (kgwas_lmm_run_table). With
//     --pheno_columns LIST   (a file of "col<TAB>name" lines, in place of -n and -o)
// the listed columns of PHENO - the phenotype and its permutations - are all tested in ONE pass over the table, the best N of each
// to D/name.assoc.txt with a log (kgwas_lmm_run_table_multi): what calc_best_pvals / get_threshold_from_perm read.
// -lmm 4 (with -bfile or --bfiles only) writes chr rs ps n_miss allele1 allele0 af beta se l_remle l_mle p_wald p_lrt p_score: the
// REML effect estimate, its standard error, the Wald and the score test beside the LRT (kgwas_lmm_run_files_all).
// -c FILE (with -bfile, --bfiles or --kmers_table -n; -lmm 2 or 4) gives the model covariates beside the variant, GEMMA's format: one
// row per individual (.fam lines, or the accessions of PHENO), whitespace-separated numbers, NA missing, a column of 1s among them.
// --pattern_cache MIB (with --kmers_table -n, with or without -c) tests each distinct presence/absence pattern once: rows that repeat
// a pattern take its result from a cache of MIB MiB on the device (kgwas_lmm_run_table_unique). The output's bytes are the same.
// --pattern_skip MIB (with --kmers_table --pheno_columns) leaves out the rows whose pattern can no longer enter any column's best N:
// a table of MIB MiB on the device remembers them (kgwas_lmm_run_table_multi_skip). The outputs' bytes are the same.
#include <sys/stat.h>

#include <cstdlib>
#include <fstream>
#include <iostream>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../include/kgwas.h"
#include "cli_args.h"

using namespace std;

static void usage(const char* prog) {
    cerr << "usage: " << prog
         << " -bfile B [--columns LIST] | --bfiles LIST  -lmm 2|4  -k KINSHIP  [-c COVARIATES] [-outdir D] [-o NAME] [-n i] [-maf f] [-miss f] [-lmin x] [-lmax x]\n"
            "  -bfile B       PLINK base name (B.bed, B.bim, B.fam)\n"
            "  --bfiles LIST  file of 'bfile<TAB>name' lines: every bfile is tested, output D/name.assoc.txt\n"
            "  --columns LIST file of 'col<TAB>name' lines, with -bfile: every listed phenotype column of B.fam (from 1) is tested in\n"
            "                 one pass over B.bed, output D/name.assoc.txt (no -n, no -o); the columns must share their missing individuals\n"
            "  -lmm 2         the likelihood-ratio test: columns l_mle and p_lrt\n"
            "  -lmm 4         that, and the REML effect size, the Wald test and the score test: columns beta se l_remle l_mle p_wald p_lrt\n"
            "                 p_score (with -bfile or --bfiles; not with --columns, --kmers_table or --pheno_columns). -lmm 1 and -lmm 3\n"
            "                 are not built as formats of their own: their columns are in the -lmm 4 file\n"
            "  -k FILE        kinship matrix, text, one row per .fam line\n"
            "  -c FILE        covariates, text: one row per .fam line (with --kmers_table: per accession of PHENO), up to 8 numbers per\n"
            "                 row, NA for a missing value; the columns must span the constant (give a column of 1s). An individual is used\n"
            "                 iff its phenotype is present and no covariate is NA (NA is refused with --kmers_table). Not with --columns\n"
            "                 or --pheno_columns\n"
            "  -outdir D      output directory (default ./output), -o NAME output prefix (default result)\n"
            "  -n i           phenotype column of the .fam, from 1 (default 1)\n"
            "  -maf f         minor allele frequency filter (default 0.01), -miss f missingness filter (default 0.05)\n"
            "  -lmin x, -lmax x  search range of lambda (defaults 1e-5, 1e5)\n"
            "or, every k-mer of a k-mers table (no PLINK files in between):\n"
            "       " << prog
         << " --kmers_table T --kmers_len K -p PHENO  -lmm 2  -k KINSHIP  [-c COVARIATES] [--mac M] [-maf f] [--best N] [-n i | --pheno_columns LIST]\n"
            "       [--pattern_cache MIB | --pattern_skip MIB] [-outdir D] [-o NAME]\n"
            "       [-lmin x] [-lmax x] [--chunk_variants c] [--device d]\n"
            "  --kmers_table T  k-mers table base name (T.table, T.names); excludes -bfile, --bfiles and --columns\n"
            "  --kmers_len K    length of the k-mers (10-31)\n"
            "  -p PHENO         phenotype file: its accessions, in its order, are the individuals (each must be in the table); -k has\n"
            "                   one row per accession; -n i picks its phenotype column, from 1 (default 1)\n"
            "  --mac M, -maf f  a k-mer is tested iff kmers_table_to_bed --mac M --maf f would write it (presence count within\n"
            "                   max(ceil(n f), M) of both ends) and lmm_lrt -maf f would then test it (defaults 5, 0.01); -miss is accepted\n"
            "                   and has no effect (a table has no missing calls)\n"
            "  --best N         the N k-mers with the largest likelihood ratio are written, in table order (default 10001)\n"
            "  --pheno_columns LIST  file of 'col<TAB>name' lines: every listed phenotype column of PHENO (from 1) is tested in one pass\n"
            "                   over the table, the best N of each to D/name.assoc.txt (no -n, no -o)\n"
            "  --pattern_cache MIB  each distinct presence/absence pattern over the accessions of PHENO is tested once; the rows that\n"
            "                   repeat it take its result from a cache of MIB MiB of device memory (a whole number >= 1; a slot takes\n"
            "                   40 bytes + a byte per 4 accessions). The output is the same, byte for byte; the log gains the cache's\n"
            "                   counters. Not with --pheno_columns\n"
            "  --pattern_skip MIB  with --pheno_columns: a presence/absence pattern of which no column kept or could still keep a row is\n"
            "                   remembered in a table of MIB MiB of device memory (a whole number >= 1; a slot takes 16 bytes + a byte\n"
            "                   per 4 accessions), and the later rows that repeat it are not computed. The outputs are the same, byte\n"
            "                   for byte; the logs gain the table's counters. Not with -n (--pattern_cache is the option for one column)\n"
            "  --device d       GPU ordinal (default 0)\n";
}

static double num(const string& name, const string& s) {
    try {
        size_t pos = 0;
        const double v = stod(s, &pos);
        if (pos != s.size()) throw invalid_argument("");
        return v;
    } catch (const exception&) {
        cerr << "lmm_lrt: argument '" << s << "' of " << name << " failed to parse" << endl;
        exit(1);
    }
}

static uint64_t whole(const string& name, const string& s, uint64_t lo, uint64_t hi) {
    if (s.empty() || s.size() > 18 || s.find_first_not_of("0123456789") != string::npos || stoull(s) < lo || stoull(s) > hi) {
        cerr << "lmm_lrt: argument '" << s << "' of " << name << " is not a whole number within " << lo << ".." << hi << endl;
        exit(1);
    }
    return stoull(s);
}

// LIST of --columns and --pheno_columns: 'col<TAB>name' lines -> the columns (from 1) and the outputs outdir/name.assoc.txt
static bool read_column_list(const string& path, const string& outdir, vector<uint32_t>& columns, vector<string>& outs) {
    ifstream f(path);
    if (!f.is_open()) {
        cerr << "lmm_lrt: can't open " << path << endl;
        return false;
    }
    set<string> names;
    for (string line; getline(f, line);) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty()) continue;
        const size_t tab = line.find('\t');
        const string col = line.substr(0, tab == string::npos ? 0 : tab), name = tab == string::npos ? string() : line.substr(tab + 1);
        if (col.empty() || col.size() > 6 || col.find_first_not_of("0123456789") != string::npos || name.empty() ||
            name.find('\t') != string::npos) {
            cerr << "lmm_lrt: " << path << ": a line is not 'col<TAB>name': " << line << endl;
            return false;
        }
        if (stoul(col) < 1) {
            cerr << "lmm_lrt: " << path << ": phenotype columns start at 1: " << line << endl;
            return false;
        }
        if (!names.insert(name).second) {
            cerr << "lmm_lrt: " << path << ": the name '" << name << "' is given twice" << endl;
            return false;
        }
        columns.push_back((uint32_t)stoul(col));
        outs.push_back(outdir + "/" + name + ".assoc.txt");
    }
    if (columns.empty()) {
        cerr << "lmm_lrt: " << path << " lists no column" << endl;
        return false;
    }
    return true;
}

// lmm_lrt --kmers_table: every check that needs no device comes before the library call
static int table_mode(map<string, string>& a, const char* prog) {
    if (a.count("bfile") || a.count("bfiles") || a.count("columns")) {
        cerr << "lmm_lrt: --kmers_table excludes -bfile, --bfiles and --columns (the k-mers come from the table)" << endl;
        return 1;
    }
    if (!a.count("k") || !a.count("kmers_len") || !a.count("p")) {
        cerr << "lmm_lrt: --kmers_table needs --kmers_len, -p and -k" << endl;
        usage(prog);
        return 1;
    }
    if (a.count("pheno_columns") && (a.count("n") || a.count("o"))) {
        cerr << "lmm_lrt: --pheno_columns excludes -n and -o (LIST names the columns and the outputs)" << endl;
        return 1;
    }
    const uint64_t klen = whole("--kmers_len", a["kmers_len"], 0, 1000);
    if (klen > 31 || klen < 10) {
        cerr << "kmer length has to be between 10-31" << endl;
        return 1;
    }
    const uint64_t mac = a.count("mac") ? whole("--mac", a["mac"], 0, 1ull << 32) : 5;
    const uint64_t col = a.count("n") ? whole("-n", a["n"], 1, 1000000) : 1;
    const uint64_t chunk = a.count("chunk_variants") ? whole("--chunk_variants", a["chunk_variants"], 0, 1000000000) : 0;
    const uint64_t device = a.count("device") ? whole("--device", a["device"], 0, 1023) : 0;
    const uint64_t cache_mib = a.count("pattern_cache") ? whole("--pattern_cache", a["pattern_cache"], 1, 1ull << 20) : 0;
    const uint64_t skip_mib = a.count("pattern_skip") ? whole("--pattern_skip", a["pattern_skip"], 1, 1ull << 20) : 0;
    if (a.count("best") && a["best"].find_first_not_of("0") == string::npos) {
        cerr << "lmm_lrt: --best 0: at least one k-mer must be kept" << endl;
        return 1;
    }
    const uint64_t best = a.count("best") ? whole("--best", a["best"], 1, 1ull << 32) : 10001;
    const double maf = a.count("maf") ? num("-maf", a["maf"]) : 0.01;
    if (a.count("miss")) (void)num("-miss", a["miss"]);
    const double lmin = a.count("lmin") ? num("-lmin", a["lmin"]) : 1e-5, lmax = a.count("lmax") ? num("-lmax", a["lmax"]) : 1e5;
    vector<string> inputs = {a["kmers_table"] + ".names", a["kmers_table"] + ".table", a["p"], a["k"]};
    if (a.count("c")) inputs.push_back(a["c"]);
    for (const string& f : inputs) {
        ifstream probe(f);
        if (!probe.good()) {
            cerr << "Couldn't find file: " << f << endl;
            return 1;
        }
    }
    const string outdir = a.count("outdir") ? a["outdir"] : "./output";
    vector<uint32_t> columns;
    vector<string> outs;
    if (a.count("pheno_columns")) {
        if (!read_column_list(a["pheno_columns"], outdir, columns, outs)) return 1;
    } else {
        outs.push_back(outdir + "/" + (a.count("o") ? a["o"] : string("result")) + ".assoc.txt");
    }
    (void)mkdir(outdir.c_str(), 0777);
    vector<const char*> op;
    for (const string& o : outs) op.push_back(o.c_str());
    kgwas_lmm_stats st{};
    kgwas_lmm_unique_stats us{};
    kgwas_lmm_skip_stats ks{};
    const int rc = skip_mib        ? kgwas_lmm_run_table_multi_skip(a["k"].c_str(), a["kmers_table"].c_str(), (uint32_t)klen, a["p"].c_str(),
                                                                    (uint32_t)columns.size(), columns.data(), op.data(), mac, maf, best,
                                                                    lmin, lmax, chunk, (int32_t)device, &st, skip_mib, &ks)
                   : cache_mib     ? kgwas_lmm_run_table_unique(a["k"].c_str(), a.count("c") ? a["c"].c_str() : nullptr, a["kmers_table"].c_str(),
                                                                (uint32_t)klen, a["p"].c_str(), (uint32_t)col, mac, maf, best, lmin, lmax, chunk,
                                                                (int32_t)device, op[0], &st, cache_mib, &us)
                   : a.count("c")  ? kgwas_lmm_run_table_cov(a["k"].c_str(), a["c"].c_str(), a["kmers_table"].c_str(), (uint32_t)klen, a["p"].c_str(),
                                                             (uint32_t)col, mac, maf, best, lmin, lmax, chunk, (int32_t)device, op[0], &st)
                   : columns.empty() ? kgwas_lmm_run_table(a["k"].c_str(), a["kmers_table"].c_str(), (uint32_t)klen, a["p"].c_str(), (uint32_t)col,
                                                         mac, maf, best, lmin, lmax, chunk, (int32_t)device, op[0], &st)
                                   : kgwas_lmm_run_table_multi(a["k"].c_str(), a["kmers_table"].c_str(), (uint32_t)klen, a["p"].c_str(),
                                                               (uint32_t)columns.size(), columns.data(), op.data(), mac, maf, best, lmin,
                                                               lmax, chunk, (int32_t)device, &st);
    if (rc != KGWAS_OK) {
        cerr << "lmm_lrt: " << kgwas_last_error() << endl;
        return rc == KGWAS_ERR_DEVICE ? 3 : 1;
    }
    cerr << "[kgwas] lmm_lrt: kmers_table=" << a["kmers_table"] << " columns=" << (columns.empty() ? 1 : columns.size())
         << " individuals=" << st.n_individuals << " rows_read=" << st.variants_read
         << " rows_tested=" << st.variants_tested << (cache_mib ? " rows_rotated=" + to_string(us.rows_rotated) : string())
         << (skip_mib ? " rows_skipped=" + to_string(ks.rows_skipped) + " rows_rotated=" + to_string(ks.rows_rotated) : string())
         << " best=" << best << " eigendecompositions=" << st.eigendecompositions
         << " ms: eigen=" << st.eigen_ms << " rotate=" << st.rotate_ms << " grid=" << st.grid_ms << " refine=" << st.refine_ms << endl;
    cli_finish();
    return 0;
}

int main(int argc, char* argv[]) {
    static const char* const valued[] = {"bfile", "bfiles", "lmm", "k", "outdir", "o", "n", "maf", "miss", "lmin", "lmax", "chunk_variants", "columns",
                                         "kmers_table", "kmers_len", "p", "mac", "best", "device", "pheno_columns", "c",
                                         "pattern_cache", "pattern_skip"};
    map<string, string> a;
    for (int i = 1; i < argc; i++) {
        string s = argv[i];
        if (s == "-h" || s == "--help" || s == "-help") {
            usage(argv[0]);
            return 0;
        }
        const size_t dashes = s.rfind("--", 0) == 0 ? 2 : s.rfind("-", 0) == 0 ? 1 : 0;
        const string name = s.substr(dashes);
        bool known = false;
        for (const char* v : valued) known |= name == v;
        if (!dashes || !known) {
            cerr << "lmm_lrt: unknown option '" << s << "'" << endl;
            usage(argv[0]);
            return 1;
        }
        if (i + 1 >= argc) {
            cerr << "lmm_lrt: option '" << s << "' is missing an argument" << endl;
            return 1;
        }
        a[name] = argv[++i];
    }
    if (!a.count("lmm") || (a["lmm"] != "2" && a["lmm"] != "4")) {
        cerr << "lmm_lrt: -lmm " << (a.count("lmm") ? a["lmm"] : string("(missing)"))
             << ": only -lmm 2 and -lmm 4 are built; -lmm 4 writes the Wald and score columns too" << endl;
        return 1;
    }
    const bool all_tests = a["lmm"] == "4";
    if (all_tests) {  // (before any file is opened)
        string given;
        for (const char* o : {"columns", "kmers_table", "pheno_columns"})
            if (a.count(o)) given += string(given.empty() ? "" : ", ") + "--" + o;
        if (!given.empty()) {
            cerr << "lmm_lrt: -lmm 4 is not built for " << given << ": it takes -bfile or --bfiles (-lmm 2 runs with them)" << endl;
            return 1;
        }
    }
    if (a.count("c")) {  // (before any file is opened)
        for (const char* o : {"columns", "pheno_columns"})
            if (a.count(o)) {
                cerr << "lmm_lrt: -c is not built for --" << o << ": covariates go with one phenotype column (-n)" << endl;
                return 1;
            }
    }
    if (a.count("pattern_cache") && a.count("pheno_columns")) {  // (before any file is opened)
        cerr << "lmm_lrt: --pattern_cache is not built for --pheno_columns: the cache goes with one phenotype column (-n)" << endl;
        return 1;
    }
    if (a.count("pattern_skip") && !a.count("pheno_columns")) {  // (before any file is opened)
        cerr << "lmm_lrt: --pattern_skip goes with --pheno_columns: with one phenotype column (-n) the option is --pattern_cache" << endl;
        return 1;
    }
    if (a.count("kmers_table")) return table_mode(a, argv[0]);
    for (const char* o : {"kmers_len", "p", "mac", "best", "device", "pheno_columns", "pattern_cache", "pattern_skip"})
        if (a.count(o)) {
            cerr << "lmm_lrt: option '" << o << "' needs --kmers_table" << endl;
            return 1;
        }
    if (a.count("columns") && (a.count("bfiles") || a.count("n") || a.count("o") || !a.count("bfile"))) {
        cerr << "lmm_lrt: --columns needs -bfile and excludes --bfiles, -n and -o (LIST names the outputs)" << endl;
        return 1;
    }
    if (!a.count("k") || a.count("bfile") + a.count("bfiles") != 1) {
        cerr << "lmm_lrt: need -k and one of -bfile, --bfiles" << endl;
        usage(argv[0]);
        return 1;
    }
    const string outdir = a.count("outdir") ? a["outdir"] : "./output";
    vector<string> bases, outs;
    vector<uint32_t> columns;
    if (a.count("columns")) {
        if (!read_column_list(a["columns"], outdir, columns, outs)) return 1;
        bases.push_back(a["bfile"]);
    } else if (a.count("bfile")) {
        bases.push_back(a["bfile"]);
        outs.push_back(outdir + "/" + (a.count("o") ? a["o"] : string("result")) + ".assoc.txt");
    } else {
        ifstream f(a["bfiles"]);
        if (!f.is_open()) {
            cerr << "lmm_lrt: can't open " << a["bfiles"] << endl;
            return 1;
        }
        for (string line; getline(f, line);) {
            if (!line.empty() && line.back() == '\r') line.pop_back();
            if (line.empty()) continue;
            const size_t tab = line.find('\t');
            if (tab == string::npos || tab == 0 || tab + 1 == line.size()) {
                cerr << "lmm_lrt: " << a["bfiles"] << ": a line is not 'bfile<TAB>name': " << line << endl;
                return 1;
            }
            bases.push_back(line.substr(0, tab));
            outs.push_back(outdir + "/" + line.substr(tab + 1) + ".assoc.txt");
        }
    }
    const double maf = a.count("maf") ? num("-maf", a["maf"]) : 0.01, miss = a.count("miss") ? num("-miss", a["miss"]) : 0.05;
    const double lmin = a.count("lmin") ? num("-lmin", a["lmin"]) : 1e-5, lmax = a.count("lmax") ? num("-lmax", a["lmax"]) : 1e5;
    const double col = a.count("n") ? num("-n", a["n"]) : 1, chunk = a.count("chunk_variants") ? num("--chunk_variants", a["chunk_variants"]) : 0;
    if (col < 1 || col > 1e6 || col != (double)(uint32_t)col || chunk < 0 || chunk > 1e9) {
        cerr << "lmm_lrt: -n or --chunk_variants out of range" << endl;
        return 1;
    }
    (void)mkdir(outdir.c_str(), 0777);  // (an existing directory is fine; a failure shows when the output is written)
    vector<const char*> bp, op;
    for (const string& b : bases) bp.push_back(b.c_str());
    for (const string& o : outs) op.push_back(o.c_str());
    kgwas_lmm_stats st{};
    const int rc = a.count("c")    ? kgwas_lmm_run_files_cov(a["k"].c_str(), a["c"].c_str(), bases.size(), bp.data(), op.data(), (uint32_t)col, maf,
                                                             miss, lmin, lmax, (uint64_t)chunk, 0, all_tests ? 1 : 0, &st)
                   : all_tests     ? kgwas_lmm_run_files_all(a["k"].c_str(), bases.size(), bp.data(), op.data(), (uint32_t)col, maf, miss, lmin,
                                                             lmax, (uint64_t)chunk, 0, &st)
                   : columns.empty() ? kgwas_lmm_run_files(a["k"].c_str(), bases.size(), bp.data(), op.data(), (uint32_t)col, maf, miss, lmin,
                                                           lmax, (uint64_t)chunk, 0, &st)
                                     : kgwas_lmm_run_file_multi(a["k"].c_str(), bp[0], (uint32_t)columns.size(), columns.data(), op.data(), maf,
                                                              miss, lmin, lmax, (uint64_t)chunk, 0, &st);
    if (rc != KGWAS_OK) {
        cerr << "lmm_lrt: " << kgwas_last_error() << endl;
        return rc == KGWAS_ERR_DEVICE ? 3 : 1;
    }
    cerr << "[kgwas] lmm_lrt: files=" << bases.size() << " columns=" << (columns.empty() ? 1 : columns.size()) << " individuals=" << st.n_individuals << " variants_read=" << st.variants_read
         << " variants_tested=" << st.variants_tested << " eigendecompositions=" << st.eigendecompositions << " ms: eigen=" << st.eigen_ms
         << " rotate=" << st.rotate_ms << " grid=" << st.grid_ms << " refine=" << st.refine_ms << endl;
    cli_finish();
    return 0;
}
