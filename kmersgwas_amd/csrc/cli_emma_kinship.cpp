// emma_kinship — drop-in for the reference tool of the same name (src/emma_kinship.cpp): one positional argument (the
// base name of the .bed/.bim/.fam files), the kinship matrix on stdout, the same first stderr line and progress dots; the
// accumulation runs on GPU 0 (kgwas_snpkin_*). The one deliberate difference: a .fam without lines is an error (exit 1)
// where the reference divides by zero.
#include <chrono>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../../include/kgwas.h"
#include "cli_args.h"

using namespace std;

static void ck(int rc) {
    if (rc == KGWAS_OK) return;
    if (rc == KGWAS_ERR_FORMAT || rc == KGWAS_ERR_IO) {  // the reference's uncaught std::runtime_error (is_not_true, :27-31)
        cerr << "terminate called after throwing an instance of 'std::runtime_error'\n  what():  " << kgwas_last_error() << endl;
        abort();
    }
    cerr << "emma_kinship: " << kgwas_last_error() << endl;
    exit(rc == KGWAS_ERR_DEVICE ? 3 : 1);
}

static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int main(int argc, char* argv[]) {
    if (argc != 2) {
        cerr << "usage: " << argv[0] << " base file name for bed/bim/fam files" << endl;
        return -1;
    }
    const double t_main = now_s();
    kgwas_snpkin* h = nullptr;
    ck(kgwas_snpkin_open(argv[1], 0, &h));  // the file guards come first, then the device
    const double t_created = now_s();
    uint64_t S = 0, M = 0;
    ck(kgwas_snpkin_info(h, &S, &M, nullptr));
    cerr << argv[1] << "\t(snps,samples) = " << M << ", " << S << endl;
    ck(kgwas_snpkin_feed_file(h));
    // the reference's progress marks (:108-109): "." every 100 000 SNPs and "M" every 1 000 000, from SNP 0
    for (uint64_t i = 0; i < M; i += 100000) {
        cerr << ".";
        if (i % 1000000 == 0) cerr << "M";
    }
    cerr << endl;
    vector<double> K(S * S);
    uint64_t n_used = 0;
    ck(kgwas_snpkin_matrix(h, K.data(), &n_used));
    const double t_fed = now_s();
    // (one call: a cell is at most 12 characters - six significant digits, a point or an exponent - and a separator)
    string text(S * S * 16 + 16, '\0');
    const uint64_t need = kgwas_snpkin_format(S, K.data(), &text[0], text.size());
    if (need > text.size()) {
        text.assign(need, '\0');
        kgwas_snpkin_format(S, K.data(), &text[0], need);
    } else
        text.resize(need);
    const double t_text = now_s();
    cout << text;
    cout.flush();
    cerr << "[kgwas] seconds: session_create=" << (t_created - t_main) << " accumulate=" << (t_fed - t_created)
         << " matrix_text=" << (t_text - t_fed) << " stdout=" << (now_s() - t_text) << " total=" << (now_s() - t_main) << endl;
    cli_finish();
    kgwas_snpkin_close(h);
    return 0;
}
