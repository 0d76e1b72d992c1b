// list_kmers_found_in_multiple_samples — drop-in for the reference tool of the same name
// (src/list_kmers_found_in_multiple_samples.cpp): same options, guards, messages, exit statuses and output files (<output>,
// .no_pass_kmers, .shareness, .stats.only_canonical, .stats.only_non_canonical, .stats.both); the k-mers are counted and
// filtered on the GPU (kgwas_list_kmers). Extra option: --device N. Every guard of the reference happens before the device is
// touched. The deliberate differences are listed in INTEGRATION.md §1: of the reference's stderr only the three closing lines
// are printed (its 5001 progress lines are not), "kmers lower than MAC" is the true count (the reference prints an
// uninitialised variable), and three inputs on which the reference has undefined behaviour are refused.
#include <sys/stat.h>

#include <chrono>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../../include/kgwas.h"
#include "cli_args.h"

using namespace std;

static const char* const PROG = "list_kmers_found_in_multiple_samples";

static bool file_exists(const string& fn) {
    ifstream f(fn);
    return f.good();
}
[[noreturn]] static void logic_error_abort(const string& what) {  // an uncaught std::logic_error of the reference
    cerr << "terminate called after throwing an instance of 'std::logic_error'\n  what():  " << what << endl;
    abort();
}
static void ck(int rc) {
    if (rc == KGWAS_OK) return;
    if (rc == KGWAS_ERR_FORMAT) logic_error_abort(kgwas_last_error());
    cerr << PROG << ": " << kgwas_last_error() << endl;
    exit(rc == KGWAS_ERR_DEVICE ? 3 : 1);
}
static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int main(int argc, char* argv[]) {
    const double t_main = now_s();
    CliArgs result({
        {"list_kmers_files", 'l', true, "list of separate k-mers files", ""},
        {"kmers_len", 'k', true, "length of k-mers", ""},
        {"mac", 0, true, "minor allele count (minimum allowed appearence of a k-mer)", ""},
        {"min_strand_percent", 'p', true, "minimum percent of apperence in each strand form", ""},
        {"output", 'o', true, "path to output file", ""},
        {"device", 0, true, "GPU ordinal", "0"},
        {"help", 0, false, "print help", ""},
    });
    const string desc = "Combines and filters information from all samples k-mers lists to one sorted k-mers list";
    try {
        result.parse(argc, argv);
        if (result.count("help")) {
            cerr << result.help(PROG, desc) << endl;
            exit(0);
        }
        for (const char* req : {"list_kmers_files", "mac", "kmers_len", "min_strand_percent", "output"}) {
            if (result.count(req) == 0) {
                cerr << req << " is a required parameter" << endl;
                cerr << result.help(PROG, desc) << endl;
                exit(1);
            }
        }
        const string fn_kmers_list(result.str("list_kmers_files"));
        const size_t minimum_kmer_count = result.u64("mac");
        const size_t kmer_len = result.u64("kmers_len");
        const double minimum_strand_per = result.f64("min_strand_percent");
        const string fn_output(result.str("output"));
        const int device = (int)result.u64("device", 0);
        if (!file_exists(fn_kmers_list)) {
            cerr << "Couldn't find file: " << fn_kmers_list << endl;
            exit(1);
        }
        if ((kmer_len > 31) || (kmer_len < 10)) {
            cerr << "kmer length has to be between 10-31" << endl;
            exit(1);
        }

        // read_accessions_path_list (src/kmer_general.cpp:32-43): tokens alternately path and name
        vector<string> paths;
        {
            ifstream fin(fn_kmers_list);
            string path, name;
            while (fin >> path) {
                fin >> name;
                paths.push_back(path);
            }
        }
        // every file is opened as it is checked (:112-118): an empty one ends the run before a later missing one is looked for
        for (const string& p : paths) {
            if (!file_exists(p)) {
                cerr << "Couldn't find file: " << p << endl;
                exit(1);
            }
            struct stat sb;
            if (stat(p.c_str(), &sb) == 0 && ((uint64_t)sb.st_size >> 3) == 0) logic_error_abort("sorted kmer file is empty: " + p);
        }
        const double t_setup = now_s();
        vector<const char*> cpaths;
        for (const string& p : paths) cpaths.push_back(p.c_str());
        uint64_t counts[3] = {0, 0, 0};
        ck(kgwas_list_kmers(cpaths.data(), cpaths.size(), (uint32_t)kmer_len, minimum_kmer_count, minimum_strand_per, device,
                            fn_output.c_str(), counts));
        cerr << "kmers lower than MAC:\t" << counts[2] << endl;
        cerr << "passed kmers:\t" << counts[0] << endl;
        cerr << "passed MAC bot not pass strand filter:\t" << counts[1] << endl;
        cerr << "[kgwas] seconds: setup=" << (t_setup - t_main) << " list=" << (now_s() - t_setup) << " total=" << (now_s() - t_main) << endl;
        cli_finish();
    } catch (const std::invalid_argument& e) {
        cerr << "error parsing options: " << e.what() << endl;
        cerr << result.help(PROG, desc) << endl;
        exit(1);
    }
    return 0;
}
