// proxy_kmers — every k-mer of the table in LD with a lead k-mer, by exact r^2 on the GPU (kgwas_proxy_kmers_run). A tool of this
// project: clump_kmers ends with one lead per signal, this lists the k-mers that travel with each lead.
//     proxy_kmers --kmers_table T --kmers_len K --leads FILE [-p PHENO] [--r2 0.8] [--max_per_lead M] [-o OUT] [--device d]
// Every check that needs no device comes first: the options, the text of --r2, the files' existence, then (inside the library
// call) the leads file's lines - all before a file of the table is opened.
#include <sys/stat.h>

#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../../include/kgwas.h"
#include "cli_args.h"

using namespace std;

int main(int argc, char* argv[]) {
    CliArgs args({{"kmers_table", 't', true, "k-mers table base name (T.table, T.names)", ""},
                  {"kmers_len", 'k', true, "length of the k-mers (10-31)", ""},
                  {"leads", 'l', true, "the lead k-mers: one per line, or a clump_kmers output (its distinct leads)", ""},
                  {"pheno", 'p', true, "phenotype file: its accessions are the ones r2 is taken over (default: all of the table)", ""},
                  {"r2", 0, true, "a k-mer is a proxy iff r2 >= this; decimal, at most 6 digits after the point, 0 < r2 <= 1", "0.8"},
                  {"max_per_lead", 0, true, "proxies kept per lead, the first in table order (the rest are counted)", "100000"},
                  {"output", 'o', true, "output file (its log: OUT.log.txt)", "./output/proxies.txt"},
                  {"device", 0, true, "GPU ordinal", "0"},
                  {"help", 'h', false, "print help", ""}});
    const string desc = "List every k-mer of the table whose presence/absence pattern has r2 >= the threshold with a lead k-mer";
    string table, leads, out;
    uint64_t klen = 0, max_per_lead = 100000, device = 0;
    uint32_t tm = 0;
    try {
        args.parse(argc, argv);
        if (args.count("help")) {
            cout << args.help(argv[0], desc);
            return 0;
        }
        for (const char* need : {"kmers_table", "kmers_len", "leads"})
            if (!args.count(need)) {
                cerr << "proxy_kmers: option --" << need << " is missing" << endl << args.help(argv[0], desc);
                return 1;
            }
        table = args.str("kmers_table");
        leads = args.str("leads");
        out = args.str("output", "./output/proxies.txt");
        klen = args.u64("kmers_len");
        max_per_lead = args.u64("max_per_lead", 100000);
        device = args.u64("device", 0);
    } catch (const exception& e) {
        cerr << "proxy_kmers: " << e.what() << endl;
        return 1;
    }
    if (kgwas_r2_millionths(args.str("r2", "0.8").c_str(), &tm) != KGWAS_OK) {
        cerr << "proxy_kmers: " << kgwas_last_error() << endl;
        return 1;
    }
    if (klen > 31 || klen < 10) {
        cerr << "kmer length has to be between 10-31" << endl;
        return 1;
    }
    if (device > 1023) {
        cerr << "proxy_kmers: --device (at most 1023) out of range" << endl;
        return 1;
    }
    // the table's own files are looked for by the library, behind the leads file's checks
    for (const string& f : args.count("pheno") ? vector<string>{leads, args.str("pheno")} : vector<string>{leads}) {
        ifstream probe(f);
        if (!probe.good()) {
            cerr << "Couldn't find file: " << f << endl;
            return 1;
        }
    }
    if (!args.count("output")) (void)mkdir("./output", 0777);  // (an existing directory is fine; a failure shows when the output is written)
    kgwas_proxy_stats st{};
    const string pheno = args.str("pheno", "");
    const int rc = kgwas_proxy_kmers_run(table.c_str(), (uint32_t)klen, args.count("pheno") ? pheno.c_str() : nullptr, leads.c_str(), tm, max_per_lead,
                                         (int32_t)device, out.c_str(), &st);
    if (rc != KGWAS_OK) {
        cerr << "proxy_kmers: " << kgwas_last_error() << endl;
        return rc == KGWAS_ERR_DEVICE ? 3 : 1;
    }
    cerr << "[kgwas] proxy_kmers: kmers_table=" << table << " accessions=" << st.accessions << " leads=" << st.leads << " rows_read=" << st.rows_read
         << " pairs_tested=" << st.pairs_tested << " proxies_found=" << st.proxies_found << " proxies_kept=" << st.proxies_kept
         << " drain_rounds=" << st.drain_rounds << " ms: search=" << st.search_ms << " kernels=" << st.kernel_ms << " copy=" << st.copy_ms
         << " total=" << st.total_ms << endl;
    cli_finish();
    return 0;
}
