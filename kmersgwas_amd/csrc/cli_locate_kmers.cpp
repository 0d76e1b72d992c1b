// locate_kmers — the genome positions of k-mers, exact or with one mismatch, on the GPU (kgwas_locate_kmers_run). A tool of this
// project: proxy_kmers ends with the k-mers one maps, this gives each a contig and a position.
//     locate_kmers --reference FASTA --kmers FILE --kmers_len K [--mismatches 0|1] [--max_per_kmer M] [--device d] -o OUT
// Every check that needs no device comes first: the options, the files' existence, then (inside the library call) the k-mers
// file's lines - all before the reference is opened.
#include <sys/stat.h>

#include <fstream>
#include <iostream>
#include <string>

#include "../../include/kgwas.h"
#include "cli_args.h"

using namespace std;

int main(int argc, char* argv[]) {
    CliArgs args({{"reference", 'r', true, "the reference genome: FASTA in plain text", ""},
                  {"kmers", 'q', true, "the k-mers: one per line, an lmm_lrt / GEMMA .assoc.txt or clump_kmers output (column rs), or a proxy_kmers output (column kmer)", ""},
                  {"kmers_len", 'k', true, "length of the k-mers (1-31)", ""},
                  {"mismatches", 'm', true, "mismatching bases allowed in a hit: 0 or 1", "1"},
                  {"max_per_kmer", 0, true, "hits kept per k-mer, the first in genome order (the rest are counted); 0: no limit", "100"},
                  {"output", 'o', true, "output file (its log: OUT.log.txt)", "./output/located.txt"},
                  {"device", 0, true, "GPU ordinal", "0"},
                  {"help", 'h', false, "print help", ""}});
    const string desc = "List where in the reference each k-mer, or its reverse complement, occurs exactly or with one mismatching base";
    string reference, kmers, out;
    uint64_t klen = 0, mismatches = 1, max_per_kmer = 100, device = 0;
    try {
        args.parse(argc, argv);
        if (args.count("help")) {
            cout << args.help(argv[0], desc);
            return 0;
        }
        for (const char* need : {"reference", "kmers", "kmers_len"})
            if (!args.count(need)) {
                cerr << "locate_kmers: option --" << need << " is missing" << endl << args.help(argv[0], desc);
                return 1;
            }
        reference = args.str("reference");
        kmers = args.str("kmers");
        out = args.str("output", "./output/located.txt");
        klen = args.u64("kmers_len");
        mismatches = args.u64("mismatches", 1);
        max_per_kmer = args.u64("max_per_kmer", 100);
        device = args.u64("device", 0);
    } catch (const exception& e) {
        cerr << "locate_kmers: " << e.what() << endl;
        return 1;
    }
    if (klen > 31 || klen < 1) {
        cerr << "kmer length has to be between 1-31" << endl;
        return 1;
    }
    if (mismatches > 1 || (mismatches == 1 && klen < 2)) {
        cerr << "locate_kmers: --mismatches is 0 or 1 (1 needs k-mers of at least 2 bases)" << endl;
        return 1;
    }
    if (device > 1023) {
        cerr << "locate_kmers: --device (at most 1023) out of range" << endl;
        return 1;
    }
    // the k-mers file first: its lines are checked by the library before the reference is opened
    {
        ifstream probe(kmers);
        if (!probe.good()) {
            cerr << "Couldn't find file: " << kmers << endl;
            return 1;
        }
    }
    if (!args.count("output")) (void)mkdir("./output", 0777);  // (an existing directory is fine; a failure shows when the output is written)
    kgwas_locate_stats st{};
    const int rc = kgwas_locate_kmers_run(reference.c_str(), kmers.c_str(), (uint32_t)klen, (uint32_t)mismatches, max_per_kmer, (int32_t)device,
                                          out.c_str(), &st);
    if (rc != KGWAS_OK) {
        const string msg = kgwas_last_error();
        if (rc == KGWAS_ERR_IO && msg == "can't open file: " + reference)
            cerr << "Couldn't find file: " << reference << endl;
        else
            cerr << "locate_kmers: " << msg << endl;
        return rc == KGWAS_ERR_DEVICE ? 3 : 1;
    }
    cerr << "[kgwas] locate_kmers: reference=" << reference << " contigs=" << st.contigs << " bases=" << st.bases << " windows_tested=" << st.windows_tested
         << " kmers=" << st.kmers << " hits_found=" << st.hits_found << " hits_kept=" << st.hits_kept << " kmers_without_hit=" << st.kmers_without_hit
         << " kmers_with_one_hit=" << st.kmers_with_one_hit << " drain_rounds=" << st.drain_rounds << " ms: parse=" << st.parse_ms << " copy=" << st.copy_ms
         << " kernels=" << st.kernel_ms << " total=" << st.total_ms << endl;
    cli_finish();
    return 0;
}
