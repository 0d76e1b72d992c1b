// fetch_reads — the reads of an accession that contain listed k-mers, on the GPU (kgwas_fetch_reads_run). A tool of this project:
// proxy_kmers ends with the k-mers one assembles or maps, this pulls the reads to assemble.
//     fetch_reads --reads FILE [--mates FILE] --kmers FILE --kmers_len K -o PREFIX [--min_hits m] [--max_reads_per_kmer M] [--device d]
// Every check that needs no device comes first: the options, the files' existence, then (inside the library call) the k-mers
// file's lines - all before the reads are opened.
#include <fstream>
#include <iostream>
#include <string>

#include "../../include/kgwas.h"
#include "cli_args.h"

using namespace std;

int main(int argc, char* argv[]) {
    CliArgs args({{"reads", 'r', true, "the reads: FASTQ or FASTA in plain text, - for standard input", ""},
                  {"mates", 0, true, "the reads' mates, record by record, in the same format", ""},
                  {"kmers", 'q', true, "the k-mers: one per line, an lmm_lrt / GEMMA .assoc.txt or clump_kmers output (column rs), or a proxy_kmers output (column kmer)", ""},
                  {"kmers_len", 'k', true, "length of the k-mers (1-31)", ""},
                  {"min_hits", 'm', true, "windows of a read that must spell a k-mer for the read to be kept", "1"},
                  {"max_reads_per_kmer", 0, true, "reads (pairs) written per k-mer, the first in input order (the rest are counted); 0: no limit", "0"},
                  {"output", 'o', true, "output prefix: PREFIX.fastq / .fasta (PREFIX_1.*, PREFIX_2.* with mates), PREFIX.reads.tsv, PREFIX.log.txt", ""},
                  {"device", 0, true, "GPU ordinal", "0"},
                  {"help", 'h', false, "print help", ""}});
    const string desc = "Pull the reads that contain a listed k-mer, or its reverse complement, out of an accession's reads";
    string reads, mates, kmers, out;
    uint64_t klen = 0, min_hits = 1, max_reads = 0, device = 0;
    try {
        args.parse(argc, argv);
        if (args.count("help")) {
            cout << args.help(argv[0], desc);
            return 0;
        }
        for (const char* need : {"reads", "kmers", "kmers_len", "output"})
            if (!args.count(need)) {
                cerr << "fetch_reads: option --" << need << " is missing" << endl << args.help(argv[0], desc);
                return 1;
            }
        reads = args.str("reads");
        if (args.count("mates")) mates = args.str("mates");
        kmers = args.str("kmers");
        out = args.str("output");
        klen = args.u64("kmers_len");
        min_hits = args.u64("min_hits", 1);
        max_reads = args.u64("max_reads_per_kmer", 0);
        device = args.u64("device", 0);
    } catch (const exception& e) {
        cerr << "fetch_reads: " << e.what() << endl;
        return 1;
    }
    if (klen > 31 || klen < 1) {
        cerr << "kmer length has to be between 1-31" << endl;
        return 1;
    }
    if (min_hits < 1 || min_hits > 0xFFFFFFFFull) {
        cerr << "fetch_reads: --min_hits is at least 1" << endl;
        return 1;
    }
    if (device > 1023) {
        cerr << "fetch_reads: --device (at most 1023) out of range" << endl;
        return 1;
    }
    if (args.count("mates") && (reads == "-" || mates == "-")) {
        cerr << "fetch_reads: standard input cannot be one of two files" << endl;
        return 1;
    }
    // the k-mers file first: its lines are checked by the library before the reads are opened
    {
        ifstream probe(kmers);
        if (!probe.good()) {
            cerr << "Couldn't find file: " << kmers << endl;
            return 1;
        }
    }
    kgwas_fetch_stats st{};
    const int rc = kgwas_fetch_reads_run(reads.c_str(), args.count("mates") ? mates.c_str() : nullptr, kmers.c_str(), (uint32_t)klen, (uint32_t)min_hits,
                                         max_reads, (int32_t)device, out.c_str(), &st);
    if (rc != KGWAS_OK) {
        const string msg = kgwas_last_error();
        if (rc == KGWAS_ERR_IO && msg.rfind("can't open file: ", 0) == 0)
            cerr << "Couldn't find file: " << msg.substr(17) << endl;
        else
            cerr << "fetch_reads: " << msg << endl;
        return rc == KGWAS_ERR_DEVICE ? 3 : 1;
    }
    cerr << "[kgwas] fetch_reads: reads=" << st.reads << " bases=" << st.bases << " windows_tested=" << st.windows_tested << " kmers=" << st.kmers
         << " windows_hit=" << st.windows_hit << " reads_kept=" << st.reads_kept << " reads_written=" << st.reads_written << " pairs_written=" << st.pairs_written
         << " kmers_without_read=" << st.kmers_without_read << " drain_rounds=" << st.drain_rounds << " ms: parse=" << st.parse_ms << " copy=" << st.copy_ms
         << " kernels=" << st.kernel_ms << " total=" << st.total_ms << endl;
    cli_finish();
    return 0;
}
