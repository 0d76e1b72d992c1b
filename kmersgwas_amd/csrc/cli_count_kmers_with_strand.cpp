// count_kmers_with_strand — an accession's sorted k-mer file from its reads (kgwas_count_kmers_files): one run of this tool
// stands where the reference pipeline runs `kmc -ci<T>`, `kmc -ci0 -b` and kmers_add_strand_information
// (examples/resistence_e_coli/run_example.sh:55-61). It is a tool of this project, not a drop-in: its options are its own, its
// output file and the lines on stdout are kmers_add_strand_information's (src/kmers_add_strand_information.cpp:97,115-116,
// 125-126,140). The rules of the count are in include/kgwas.h. Every guard happens before the device is touched.
#include <chrono>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../../include/kgwas.h"
#include "cli_args.h"

using namespace std;

static const char* const PROG = "count_kmers_with_strand";

static bool file_exists(const string& fn) {
    ifstream f(fn);
    return f.good();
}
static void ck(int rc) {
    if (rc == KGWAS_OK) return;
    cerr << PROG << ": " << kgwas_last_error() << endl;
    exit(rc == KGWAS_ERR_DEVICE ? 3 : 1);
}
static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int main(int argc, char* argv[]) {
    const double t_main = now_s();
    CliArgs result({
        {"input", 'i', true, "FASTA or FASTQ file with the reads, - for standard input", ""},
        {"list_files", 'l', true, "file with one path of a FASTA or FASTQ file per line", ""},
        {"kmers_len", 'k', true, "length of k-mers", ""},
        {"ci", 0, true, "minimum count of a k-mer (canonical form) to be kept", "2"},
        {"cx", 0, true, "maximum count of a k-mer (canonical form) to be kept", "1000000000"},
        {"output", 'o', true, "path to output file", ""},
        {"device", 0, true, "GPU ordinal", "0"},
        {"help", 0, false, "print help", ""},
    });
    const string desc = "Counts the k-mers of reads in canonical form and writes the sorted k-mers with their strand information";
    try {
        result.parse(argc, argv);
        if (result.count("help")) {
            cerr << result.help(PROG, desc) << endl;
            exit(0);
        }
        if (result.count("input") + result.count("list_files") == 0) {
            cerr << "input is a required parameter" << endl;
            cerr << result.help(PROG, desc) << endl;
            exit(1);
        }
        if (result.count("input") && result.count("list_files")) {
            cerr << "input and list_files can not be given together" << endl;
            cerr << result.help(PROG, desc) << endl;
            exit(1);
        }
        for (const char* req : {"kmers_len", "output"}) {
            if (result.count(req) == 0) {
                cerr << req << " is a required parameter" << endl;
                cerr << result.help(PROG, desc) << endl;
                exit(1);
            }
        }
        const size_t kmer_len = result.u64("kmers_len");
        const uint64_t ci = result.u64("ci", 2), cx = result.u64("cx", 1000000000ull);
        const string fn_output(result.str("output"));
        const int device = (int)result.u64("device", 0);
        vector<string> paths;
        if (result.count("input"))
            paths.push_back(result.str("input"));
        else {
            const string fn_list(result.str("list_files"));
            if (!file_exists(fn_list)) {
                cerr << "Couldn't find file: " << fn_list << endl;
                exit(1);
            }
            ifstream fin(fn_list);
            string line;
            while (getline(fin, line)) {
                if (!line.empty() && line.back() == '\r') line.pop_back();
                if (!line.empty()) paths.push_back(line);
            }
        }
        for (const string& p : paths) {
            if (p != "-" && !file_exists(p)) {
                cerr << "Couldn't find file: " << p << endl;
                exit(1);
            }
        }
        if ((kmer_len > 31) || (kmer_len < 10)) {
            cerr << "kmer length has to be between 10-31" << endl;
            exit(1);
        }
        if (ci > cx) {
            cerr << "ci has to be at most cx" << endl;
            exit(1);
        }
        const double t_setup = now_s();
        vector<const char*> cpaths;
        for (const string& p : paths) cpaths.push_back(p.c_str());
        uint64_t counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        ck(kgwas_count_kmers_files(cpaths.data(), cpaths.size(), (uint32_t)kmer_len, ci, cx, device, fn_output.c_str(), counts));
        cout << "Canonized kmers:\t" << counts[0] << endl;
        cout << "Non-canon kmers:\t" << counts[1] << endl;
        cout << "Non-canon kmers found:\t" << counts[2] << endl;
        for (int f = 0; f < 4; f++) cout << "flag\t" << f << "\tcount is\t" << counts[3 + f] << endl;
        cout << "kmers to save:\t" << counts[0] << endl;
        cerr << "[kgwas] seconds: setup=" << (t_setup - t_main) << " count=" << (now_s() - t_setup) << " total=" << (now_s() - t_main)
             << " windows=" << counts[7] << endl;
        cli_finish();
    } catch (const std::invalid_argument& e) {
        cerr << "error parsing options: " << e.what() << endl;
        cerr << result.help(PROG, desc) << endl;
        exit(1);
    }
    return 0;
}
