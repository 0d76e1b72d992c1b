// table_session.h — what clump.cpp, proxy.cpp and lmm_files.cpp's TableRun set up before they walk a k-mers table under a phenotype
// file's accessions: one owner of the open table and the loaded phenotype file, the table's shape, the column map, the accession mask,
// the rows of a list of k-mers (kgwas_filter_kmers: its only device work). Each step is a call, so a tool keeps its order of refusals.
#pragma once
#include "kernels.h"
#include "ld_host.h"

namespace kgwas {

struct TableSession {
    kgwas_table* t = nullptr;
    kgwas_pheno* ph = nullptr;  // null: no phenotype file, every accession of the table in the table's order
    std::string pheno_path;
    uint64_t n_pheno = 0, S = 0;  // S: the accessions in use
    uint64_t S_f = 0, n_rows = 0, W_f = 0;
    uint32_t klen = 0;
    std::vector<const char*> acc;  // [S] the phenotype file's accessions, in its order
    std::vector<uint64_t> col;     // [S] their table columns (empty without a phenotype file)
    ~TableSession() {
        if (t) kgwas_table_close(t);
        if (ph) kgwas_pheno_free(ph);
    }
    uint64_t stride() const { return 1 + W_f; }  // words of a table row: its k-mer, then its bits

    // (fetching the accession names and, below, the table's shape cannot fail for an open handle, so where they stand decides no
    // refusal: lmm_lrt's load_pheno -> need_column -> load_values -> open_table order of refusals is what it was)
    void load_pheno(const char* path) {
        pheno_path = path;
        ck(kgwas_pheno_load(path, &ph));
        ck(kgwas_pheno_info(ph, &n_pheno, &S));
        acc.resize(S);
        for (uint64_t i = 0; i < S; i++) ck(kgwas_pheno_accession(ph, i, &acc[i]));
    }
    // opens the table, takes its shape and, with a phenotype file, maps its accessions to the table's columns
    void open_table(const char* table_base, uint32_t kmer_len) {
        ck(kgwas_table_open(table_base, kmer_len, &t));
        ck(kgwas_table_info(t, &S_f, &n_rows, &W_f, &klen));
        if (!ph) S = S_f;
        col.resize(ph ? S : 0);
        if (ph) ck(kgwas_table_column_map(t, acc.data(), S, col.data()));
    }
    // the bits of a table row that belong to the accessions in use; refuse_twice: an accession listed twice is refused
    std::vector<uint64_t> accession_mask(bool refuse_twice = false) const {
        std::vector<uint64_t> mask(W_f, 0);
        for (uint64_t i = 0; i < S; i++) {
            const uint64_t c = ph ? col[i] : i;
            if (refuse_twice && (mask[c / 64] >> (c % 64) & 1)) throw Error(KGWAS_ERR_FORMAT, pheno_path + " lists the accession " + acc[i] + " twice");
            mask[c / 64] |= 1ull << (c % 64);
        }
        return mask;
    }
    void refuse_duplicate_accessions() const { accession_mask(true); }
    void check_squeeze_fits(const char* who) const { if (ph) kgwas::check_squeeze_fits(who, S_f, S); }  // (no phenotype file, no squeeze)
    // Codes in the caller's order in, their table rows [n][stride()] in that order out (the table's own search, kgwas_filter_kmers);
    // the caller words the refusal of a code the table lacks from `missing`.
    PlacedRows rows_of_codes(const std::vector<uint64_t>& codes, int32_t device) const {
        std::vector<uint64_t> found(codes.size() * stride());
        uint64_t n_found = 0;
        ck(kgwas_filter_kmers(t, codes.data(), codes.size(), device, nullptr, found.data(), &n_found));
        return place_rows(codes.data(), codes.size(), found.data(), n_found, stride());
    }
};

}  // namespace kgwas
