// ld_host.h — host-side pieces of the exact r^2 tools that need no device and are about neither clumping nor proxies (clump_host.h and
// proxy_host.h build on it; tools/clump_host_check.cpp runs it under the sanitizers): the fields of a text line, the threshold's
// text, r^2 as a quotient, a k-mer field of a text file, the limits every r^2 pass shares, and the placement of a k-mer list's rows.
#pragma once
#include <cerrno>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <limits>
#include <unordered_map>
#include <vector>

#include "common.h"

namespace kgwas {

constexpr uint64_t LD_MAX_ACC = 8192;

// checked before any device call; the k-mer and lead limits stay with their tools
inline void check_ld_shape(const char* who, uint64_t n_acc, uint32_t tm) {
    const std::string w(who);
    if (n_acc == 0 || n_acc > LD_MAX_ACC)
        throw Error(KGWAS_ERR_ARG, w + ": " + std::to_string(n_acc) + " accessions: the exact r2 test is built for 1 to " + std::to_string(LD_MAX_ACC) +
                                       " (its integers are sized for them)");
    if (tm == 0 || tm > 1000000) throw Error(KGWAS_ERR_ARG, w + ": r2_millionths must be within 1..1000000");
}

// "0.8" -> 800000: decimal text with at most 6 digits after the point, 0 < t <= 1, read digit by digit (never through a double)
inline uint32_t r2_millionths(const std::string& text) {
    const Error bad(KGWAS_ERR_ARG, "--r2 '" + text + "' is not a decimal number with at most 6 digits after the point and 0 < r2 <= 1");
    const size_t dot = text.find('.');
    const std::string whole = text.substr(0, dot), frac = dot == std::string::npos ? std::string() : text.substr(dot + 1);
    if ((whole.empty() && frac.empty()) || whole.size() > 6 || frac.size() > 6) throw bad;
    if (whole.find_first_not_of("0123456789") != std::string::npos || frac.find_first_not_of("0123456789") != std::string::npos) throw bad;
    uint64_t v = 0;
    for (char c : whole) v = v * 10 + (uint64_t)(c - '0');
    for (size_t i = 0; i < 6; i++) v = v * 10 + (i < frac.size() ? (uint64_t)(frac[i] - '0') : 0);
    if (v < 1 || v > 1000000) throw bad;
    return (uint32_t)v;
}

inline std::vector<std::string> fields_of(const std::string& line) {
    std::vector<std::string> f;
    size_t i = 0;
    while (i < line.size()) {
        while (i < line.size() && (line[i] == ' ' || line[i] == '\t' || line[i] == '\r')) i++;
        size_t j = i;
        while (j < line.size() && line[j] != ' ' && line[j] != '\t' && line[j] != '\r') j++;
        if (j > i) f.push_back(line.substr(i, j - i));
        i = j;
    }
    return f;
}

// r^2 as the quotient of two integers below 2^53; nan for a constant row
inline double r2_of(uint64_t n, uint64_t ca, uint64_t cb, uint64_t n11) {
    const int64_t d = (int64_t)(n * n11) - (int64_t)(ca * cb);
    const uint64_t num = (uint64_t)(d * d), den = ca * (n - ca) * cb * (n - cb);
    return den ? (double)num / (double)den : std::numeric_limits<double>::quiet_NaN();
}

// A k-mer field of a text file -> its code: kmer_len letters of A, C, G, T. encode is kgwas_kmer_encode (a status and the code);
// `at` ("FILE line N: ") starts the message.
typedef int (*EncodeFn)(const char* word, uint64_t len, uint64_t* code);
inline uint64_t parse_kmer_field(const std::string& text, uint32_t kmer_len, EncodeFn encode, const std::string& at) {
    uint64_t code = 0;
    if (text.size() != kmer_len)
        throw Error(KGWAS_ERR_FORMAT, at + "k-mer '" + text + "' has length " + std::to_string(text.size()) + ", not " + std::to_string(kmer_len));
    if (encode(text.c_str(), text.size(), &code) != KGWAS_OK) throw Error(KGWAS_ERR_FORMAT, at + "k-mer '" + text + "' has a letter other than A, C, G, T");
    return code;
}

// The rows of a list of distinct k-mers, in the list's order, from what the table's search found: found[n_found][stride], word 0 of
// a row its k-mer, in table order. Of a key the table holds twice the first row is taken. missing: the place of the first code the
// table lacks, or NONE.
struct PlacedRows {
    static constexpr uint64_t NONE = ~0ull;
    std::vector<uint64_t> rows;  // [n][stride]
    uint64_t missing = NONE;
};
inline PlacedRows place_rows(const uint64_t* codes, uint64_t n, const uint64_t* found, uint64_t n_found, uint64_t stride) {
    PlacedRows out;
    out.rows.assign(n * stride, 0);
    std::unordered_map<uint64_t, uint64_t> at;  // code -> place in the list
    for (uint64_t i = 0; i < n; i++) at.emplace(codes[i], i);
    std::vector<uint8_t> have(n, 0);
    for (uint64_t i = 0; i < n_found; i++) {
        const auto it = at.find(found[i * stride]);
        if (it == at.end() || have[it->second]) continue;  // (a key the table holds twice: its first row)
        have[it->second] = 1;
        memcpy(&out.rows[it->second * stride], &found[i * stride], stride * 8);
    }
    for (uint64_t i = 0; i < n && out.missing == PlacedRows::NONE; i++)
        if (!have[i]) out.missing = i;
    return out;
}

}  // namespace kgwas
