// filter_kmers — drop-in for the reference tool of the same name (src/filter_kmers.cpp): same options, messages, exit
// statuses and output file; the match, the row selection and the text lines run on the GPU (kgwas_filter_kmers_write).
// Extra option: --device N. Every guard of the reference, and the opening of the output file, happens before the device
// is touched. The one deliberate difference: a list of k-mers longer than 32 bases exits 1 with a message, where the
// reference's kmer2bits shifts past 64 bits (undefined behaviour).
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
    cerr << "filter_kmers: " << kgwas_last_error() << endl;
    exit(rc == KGWAS_ERR_DEVICE ? 3 : 1);
}
static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int main(int argc, char* argv[]) {
    const double t_main = now_s();
    CliArgs result({
        {"kmers_table", 't', true, "k-mers table path", ""},
        {"kmers_file", 'k', true, "file with k-mers, each k-mer in a seperate line", ""},
        {"output", 'o', true, "output file", ""},
        {"device", 0, true, "GPU ordinal", "0"},
        {"help", 0, false, "print help", ""},
    });
    const string desc = "Output the presence/absence patterns of set of k-mers from the k-mers table";
    try {
        result.parse(argc, argv);
        if (result.count("help")) {
            cerr << result.help("filter_kmers", desc) << endl;
            exit(0);
        }
        for (const char* req : {"kmers_table", "kmers_file", "output"}) {
            if (result.count(req) == 0) {
                cerr << req << " is a required parameter" << endl;
                cerr << result.help("filter_kmers", desc) << endl;
                exit(1);
            }
        }
        const string fn_kmers_table(result.str("kmers_table"));
        const string fn_kmers_file(result.str("kmers_file"));
        const string fn_output_file(result.str("output"));
        const int device = (int)result.u64("device", 0);
        for (const string& f : {fn_kmers_table + ".names", fn_kmers_table + ".table", fn_kmers_file}) {
            if (!file_exists(f)) {
                cerr << "Couldn't find file: " << f << endl;
                exit(1);
            }
        }

        // read_and_sort_kmers (:30-50): words split on whitespace, the first one sets the length (the library sorts)
        vector<uint64_t> kmers;
        size_t kmer_len = 0;
        {
            ifstream fin(fn_kmers_file);
            string word;
            while (fin >> word) {
                if (kmers.empty()) {
                    kmer_len = word.size();
                    if (kmer_len > 32) {
                        cerr << "filter_kmers: k-mers longer than 32 bases are not supported: " << word << endl;
                        exit(1);
                    }
                }
                if (word.size() != kmer_len) {
                    cerr << "all kmers should be of the same size: " << word << endl;
                    logic_error_abort("kmers of different size");
                }
                uint64_t code = 0;
                ck(kgwas_kmer_encode(word.data(), word.size(), &code));  // "Ilegal kmer"
                kmers.push_back(code);
            }
        }
        if (kmers.empty()) {
            cerr << "kmers file is empty" << endl;
            return 1;
        }
        uint64_t n_names = 0;
        {
            ifstream fin(fn_kmers_table + ".names");
            string word;
            while (fin >> word) n_names++;
        }
        const uint64_t words_per_kmer = (n_names + 63) / 64;
        // the table guards with filter_kmers' own messages (:105-134)
        {
            ifstream th(fn_kmers_table + ".table", ios::binary | ios::ate);
            if (!th.is_open()) {
                cerr << "Can't open table file" << endl;
                return 1;
            }
            size_t left_in_file = th.tellg();
            if (left_in_file <= (4 + 8 + 4)) {
                cerr << "table file is too small" << endl;
                return 1;
            }
            th.seekg(0, ios::beg);
            uint32_t prefix = 0, file_kmer_len = 0;
            uint64_t file_accession_number = 0;
            th.read(reinterpret_cast<char*>(&prefix), sizeof(prefix));
            th.read(reinterpret_cast<char*>(&file_accession_number), sizeof(file_accession_number));
            th.read(reinterpret_cast<char*>(&file_kmer_len), sizeof(file_kmer_len));
            left_in_file -= 16;
            if (prefix != 0xDDCCBBAA) logic_error_abort("Incorrect prefix");
            if (file_accession_number != n_names) logic_error_abort("number of accession in file not as defined in class");
            if (file_kmer_len != kmer_len) logic_error_abort("kmer length in table and in list are not the same");
            const size_t size_per_kmer = sizeof(uint64_t) * (1 + words_per_kmer);
            if ((left_in_file % size_per_kmer) != 0) logic_error_abort("size of file not valid");
            cerr << "We have " << left_in_file / size_per_kmer << endl;
        }
        {
            ofstream fout(fn_output_file);
            if (!fout.is_open()) {
                cerr << "can't open output file " << endl;
                return 1;
            }
        }
        const double t_setup = now_s();
        kgwas_table* tbl = nullptr;
        ck(kgwas_table_open(fn_kmers_table.c_str(), (uint32_t)kmer_len, &tbl));
        uint64_t found = 0;
        ck(kgwas_filter_kmers_write(tbl, kmers.data(), kmers.size(), device, fn_output_file.c_str(), &found));
        cerr << "[kgwas] seconds: setup=" << (t_setup - t_main) << " filter=" << (now_s() - t_setup) << " total=" << (now_s() - t_main)
             << " rows=" << found << endl;
        cli_finish();
        kgwas_table_close(tbl);
    } catch (const std::invalid_argument& e) {
        cerr << "error parsing options: " << e.what() << endl;
        cerr << result.help("filter_kmers", desc) << endl;
        exit(1);
    }
    return 0;
}
