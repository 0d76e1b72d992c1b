// build_kmers_table — drop-in for the reference tool of the same name (src/build_kmers_table.cpp): same options, messages,
// exit statuses, <output>.names and <output>.table; the presence/absence bits are matched on the GPU (kgwas_build_table).
// Extra option: --device N. Every guard of the reference, the partial .names of a missing accession path included, happens
// before the device is touched. The one deliberate difference: of the reference's progress log on stderr (more than 10 000
// lines, hash-map sizes among them) only "Create merger", "Opens file" and "close file" are printed.
#include <chrono>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../../include/kgwas.h"
#include "cli_args.h"

using namespace std;

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
    cerr << "build_kmers_table: " << kgwas_last_error() << endl;
    exit(rc == KGWAS_ERR_DEVICE ? 3 : 1);
}
static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int main(int argc, char* argv[]) {
    const double t_main = now_s();
    CliArgs result({
        {"list_kmers_files", 'l', true, "list of separate k-mers files", ""},
        {"kmers_len", 'k', true, "length of k-mers", ""},
        {"all_kmers", 'a', true, "path to file with all k-mers", ""},
        {"output", 'o', true, "prefix for kmers-table files", ""},
        {"device", 0, true, "GPU ordinal", "0"},
        {"help", 0, false, "print help", ""},
    });
    const string desc = "Build the k-mers table";
    try {
        result.parse(argc, argv);
        if (result.count("help")) {
            cerr << result.help("build_kmers_table", desc) << endl;
            exit(0);
        }
        for (const char* req : {"list_kmers_files", "kmers_len", "all_kmers", "output"}) {
            if (result.count(req) == 0) {
                cerr << req << " is a required parameter" << endl;
                cerr << result.help("build_kmers_table", desc) << endl;
                exit(1);
            }
        }
        const string fn_list_kmers_files(result.str("list_kmers_files"));
        const string fn_all_kmers(result.str("all_kmers"));
        const size_t kmer_len = result.u64("kmers_len");
        const string output_base(result.str("output"));
        const int device = (int)result.u64("device", 0);
        for (const string& f : {fn_list_kmers_files, fn_all_kmers}) {
            if (!file_exists(f)) {
                cerr << "Couldn't find file: " << f << endl;
                exit(1);
            }
        }
        if ((kmer_len > 31) || (kmer_len < 10)) {
            cerr << "kmer length has to be between 10-31" << endl;
            exit(1);
        }

        // read_accessions_path_list (src/kmer_general.cpp:32-43): tokens alternately path and name; a last path without a
        // name keeps the name read before it (the failed extraction leaves the string as it was)
        vector<string> paths, names;
        {
            ifstream fin(fn_list_kmers_files);
            string path, name;
            while (fin >> path) {
                fin >> name;
                paths.push_back(path);
                names.push_back(name);
            }
        }
        {  // .names is written while the paths are checked (:80-91)
            ofstream fout_names(output_base + ".names", ios::binary);
            for (size_t i = 0; i < paths.size(); i++) {
                fout_names << names[i] << endl;
                if (!file_exists(paths[i])) {
                    cerr << "Couldn't find file: " << paths[i] << endl;
                    exit(1);
                }
            }
        }
        cerr << "Create merger" << endl;
        const double t_setup = now_s();
        vector<const char*> cpaths;
        for (const string& p : paths) cpaths.push_back(p.c_str());
        uint64_t rows = 0;
        ck(kgwas_build_table(fn_all_kmers.c_str(), cpaths.data(), nullptr, cpaths.size(), (uint32_t)kmer_len, device, output_base.c_str(),
                             &rows));
        cerr << "Opens file" << endl;
        cerr << "close file" << endl;
        cerr << "[kgwas] seconds: setup=" << (t_setup - t_main) << " build=" << (now_s() - t_setup) << " total=" << (now_s() - t_main)
             << " rows=" << rows << endl;
        cli_finish();
    } catch (const std::invalid_argument& e) {
        cerr << "error parsing options: " << e.what() << endl;
        cerr << result.help("build_kmers_table", desc) << endl;
        exit(1);
    }
    return 0;
}
