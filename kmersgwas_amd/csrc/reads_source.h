// reads_source.h — a reads file as count_kmers.cpp (count_kmers_with_strand) and fetch_host.h (fetch_reads) open and read it: FASTA
// or FASTQ in plain text, told apart by the first byte; "-" is standard input.
#pragma once
#include "sorted_file_io.h"

namespace kgwas {

struct Source {
    std::string path;
    Fd fd;
    char fmt = 0;  // '>' FASTA, '@' FASTQ, 0: an empty file
};

inline size_t read_some(int fd, char* dst, size_t n, const std::string& path) {
    for (;;) {
        const ssize_t r = ::read(fd, dst, n);
        if (r < 0 && errno == EINTR) continue;
        if (r < 0) throw Error(KGWAS_ERR_IO, "read error on " + path + ": " + std::strerror(errno));
        return (size_t)r;
    }
}

// opens the file and takes its first byte
inline void open_source(Source& s, const char* path) {
    s.path = path;
    if (s.path == "-") {
        s.fd.fd = ::dup(0);
        s.path = "standard input";
    } else
        s.fd.fd = ::open(path, O_RDONLY);
    if (s.fd.fd < 0) throw Error(KGWAS_ERR_IO, "can't open file: " + s.path);
    char c;
    if (read_some(s.fd.fd, &c, 1, s.path) == 0) return;
    if (c != '>' && c != '@') throw Error(KGWAS_ERR_FORMAT, s.path + ": neither FASTA nor FASTQ");
    s.fmt = c;
}

// the end of the line that starts at `from`: its '\n', or n
inline size_t line_end(const char* d, size_t from, size_t n) {
    const void* e = memchr(d + from, '\n', n - from);
    return e ? (size_t)(static_cast<const char*>(e) - d) : n;
}

}  // namespace kgwas
