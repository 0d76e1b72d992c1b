// clump_kmers — the k-mers of an association file grouped by exact r^2 on the GPU (kgwas_clump_kmers_run). A tool of this
// project: what `plink --clump` is to SNPs, for the list of k-mers lmm_lrt ends with.
//     clump_kmers --kmers_table T --kmers_len K --assoc FILE [-p PHENO] [--r2 0.8] [--p_max x] [-o OUT] [--tile_rows B] [--device d]
// Every check that needs no device comes first: the options, the text of --r2, the files' existence, then (inside the library
// call) the assoc file's lines - all before a file of the table is opened.
#include <sys/stat.h>

#include <cmath>
#include <fstream>
#include <iostream>
#include <limits>
#include <string>
#include <vector>

#include "../../include/kgwas.h"
#include "cli_args.h"

using namespace std;

int main(int argc, char* argv[]) {
    CliArgs args({{"kmers_table", 't', true, "k-mers table base name (T.table, T.names)", ""},
                  {"kmers_len", 'k', true, "length of the k-mers (10-31)", ""},
                  {"assoc", 'a', true, "lmm_lrt or GEMMA .assoc.txt: its columns rs and p_lrt are read", ""},
                  {"pheno", 'p', true, "phenotype file: its accessions are the ones r2 is taken over (default: all of the table)", ""},
                  {"r2", 0, true, "k-mers are linked iff r2 >= this; decimal, at most 6 digits after the point, 0 < r2 <= 1", "0.8"},
                  {"p_max", 0, true, "only hits with p_lrt <= this are used", "no cut"},
                  {"output", 'o', true, "output file (its log: OUT.log.txt)", "./output/clumps.txt"},
                  {"tile_rows", 0, true, "rows of the link matrix per block (0: blocks of at most 256 MiB)", "0"},
                  {"device", 0, true, "GPU ordinal", "0"},
                  {"help", 'h', false, "print help", ""}});
    const string desc = "Group the k-mers of an association file by exact r2 between their presence/absence patterns";
    string table, assoc, out;
    uint64_t klen = 0, tile_rows = 0, device = 0;
    uint32_t tm = 0;
    double p_max = numeric_limits<double>::infinity();
    try {
        args.parse(argc, argv);
        if (args.count("help")) {
            cout << args.help(argv[0], desc);
            return 0;
        }
        for (const char* need : {"kmers_table", "kmers_len", "assoc"})
            if (!args.count(need)) {
                cerr << "clump_kmers: option --" << need << " is missing" << endl << args.help(argv[0], desc);
                return 1;
            }
        table = args.str("kmers_table");
        assoc = args.str("assoc");
        out = args.str("output", "./output/clumps.txt");
        klen = args.u64("kmers_len");
        tile_rows = args.u64("tile_rows", 0);
        device = args.u64("device", 0);
        if (args.count("p_max")) p_max = args.f64("p_max");
    } catch (const exception& e) {
        cerr << "clump_kmers: " << e.what() << endl;
        return 1;
    }
    if (kgwas_r2_millionths(args.str("r2", "0.8").c_str(), &tm) != KGWAS_OK) {
        cerr << "clump_kmers: " << kgwas_last_error() << endl;
        return 1;
    }
    if (klen > 31 || klen < 10) {
        cerr << "kmer length has to be between 10-31" << endl;
        return 1;
    }
    if (std::isnan(p_max) || tile_rows > (1ull << 20) || device > 1023) {
        cerr << "clump_kmers: --p_max, --tile_rows (at most 1048576) or --device (at most 1023) out of range" << endl;
        return 1;
    }
    // the table's own files are looked for by the library, behind the assoc file's checks
    for (const string& f : args.count("pheno") ? vector<string>{assoc, args.str("pheno")} : vector<string>{assoc}) {
        ifstream probe(f);
        if (!probe.good()) {
            cerr << "Couldn't find file: " << f << endl;
            return 1;
        }
    }
    if (!args.count("output")) (void)mkdir("./output", 0777);  // (an existing directory is fine; a failure shows when the output is written)
    kgwas_clump_stats st{};
    const string pheno = args.str("pheno", "");
    const int rc = kgwas_clump_kmers_run(table.c_str(), (uint32_t)klen, args.count("pheno") ? pheno.c_str() : nullptr, assoc.c_str(), tm, p_max,
                                         (int32_t)device, tile_rows, out.c_str(), &st);
    if (rc != KGWAS_OK) {
        cerr << "clump_kmers: " << kgwas_last_error() << endl;
        return rc == KGWAS_ERR_DEVICE ? 3 : 1;
    }
    cerr << "[kgwas] clump_kmers: kmers_table=" << table << " accessions=" << st.accessions << " hits_read=" << st.hits_read
         << " hits_used=" << st.hits_used << " clumps=" << st.clumps << " largest_clump=" << st.largest_clump << " linked_pairs=" << st.linked_pairs
         << " ms: search=" << st.search_ms << " ld=" << st.ld_ms << " clump=" << st.clump_ms << endl;
    cli_finish();
    return 0;
}
