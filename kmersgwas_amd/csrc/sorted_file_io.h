// sorted_file_io.h — the accessions' sorted k-mer files (KmersSingleDataBaseSortedFile, src/kmers_single_database.cpp:90-177) as
// build_table.cpp and list_kmers.cpp read them: 64-bit little-endian words, opened as they are read, with pread.
#pragma once
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstring>
#include <string>

#include "common.h"

namespace kgwas {

constexpr uint64_t SORTED_KEY_MASK = 0x3FFFFFFFFFFFFFFFull;  // the top two bits of a word are flags (src/kmers_single_database.cpp:147)

struct Fd {
    int fd = -1;
    Fd() = default;
    Fd(const Fd&) = delete;
    Fd& operator=(const Fd&) = delete;
    ~Fd() { reset(); }
    void reset() {
        if (fd >= 0) ::close(fd);
        fd = -1;
    }
};

inline void write_all(int fd, const void* data, size_t n, const std::string& path) {
    const char* d = static_cast<const char*>(data);
    while (n) {
        const ssize_t w = ::write(fd, d, n);
        if (w < 0 && errno == EINTR) continue;
        if (w <= 0) throw Error(KGWAS_ERR_IO, "write error on " + path + ": " + std::strerror(w < 0 ? errno : EIO));
        d += w;
        n -= (size_t)w;
    }
}

inline void open_output(Fd& f, const std::string& path) {
    f.reset();
    f.fd = ::open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
    if (f.fd < 0) throw Error(KGWAS_ERR_IO, "can't open output file " + path + ": " + std::strerror(errno));
}

// closes a file that was written, and reports a close that fails
inline void close_output(Fd& f, const std::string& path) {
    const int rc = ::close(f.fd);
    f.fd = -1;
    if (rc != 0) throw Error(KGWAS_ERR_IO, "write error on " + path + ": " + std::strerror(errno));
}

inline void open_input(Fd& f, const std::string& path) {
    f.reset();
    f.fd = ::open(path.c_str(), O_RDONLY);
    if (f.fd < 0) throw Error(KGWAS_ERR_FORMAT, "can't open file: " + path);  // (a std::logic_error of the reference)
}

// words [off, off + cnt) of the file
inline void read_words(int fd, uint64_t* dst, uint64_t off, uint64_t cnt, const std::string& path) {
    char* d = reinterpret_cast<char*>(dst);
    uint64_t o = off * 8, n = cnt * 8;
    while (n) {
        const ssize_t r = ::pread(fd, d, n, (off_t)o);
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) throw Error(KGWAS_ERR_IO, "read error on " + path + (r < 0 ? std::string(": ") + std::strerror(errno) : ": file got shorter"));
        d += r;
        o += (uint64_t)r;
        n -= (uint64_t)r;
    }
}

// KmersSingleDataBaseSortedFile::open_file (:109-132): the file's length in words, size >> 3; *first (may be null): its first word
inline uint64_t words_in_file(const std::string& path, uint64_t* first = nullptr) {
    Fd f;
    open_input(f, path);
    struct stat sb;
    if (fstat(f.fd, &sb) != 0) throw Error(KGWAS_ERR_FORMAT, "can't open file: " + path);
    const uint64_t w = (uint64_t)sb.st_size >> 3;
    if (w == 0) throw Error(KGWAS_ERR_FORMAT, "sorted kmer file is empty: " + path);
    if (first) read_words(f.fd, first, 0, 1, path);
    return w;
}

// Index of the first word of h[0, cnt) whose masked value is above thr; cnt when there is none.
inline uint64_t first_above(const uint64_t* h, uint64_t cnt, uint64_t thr) {
    for (uint64_t o = 0; o < cnt; o += 256) {  // (a group at a time without an early exit: the compiler vectorises the test)
        const uint64_t e = std::min(cnt, o + 256);
        uint64_t any = 0;
        for (uint64_t i = o; i < e; i++) any |= (uint64_t)((h[i] & SORTED_KEY_MASK) > thr);
        if (any)
            for (uint64_t i = o; i < e; i++)
                if ((h[i] & SORTED_KEY_MASK) > thr) return i;
    }
    return cnt;
}

// kmers_step_to_threshold (src/kmer_general.cpp:255-258): the width of one of `steps` key windows for k-mers of kmer_len bases
inline uint64_t kmers_step_to_threshold(uint64_t steps, uint32_t kmer_len) { return ((1ull << (2ull * kmer_len)) - 1ull) / steps + 1; }

// The window of key x, windows counted from 1: max(1, ceil(x / step)).
inline uint64_t window_of(uint64_t x, uint64_t step) { return x == 0 ? 1 : (x - 1) / step + 1; }

// Where a walk over one file's slice ended: the words handed over so far, and, when a word above the threshold ended it, that
// word's masked key.
struct SliceEnd {
    uint64_t pos = 0;
    bool above = false;
    uint64_t head = 0;
};

// The reference's rule for one accession's slice (KmersSingleDataBaseSortedFile::load_kmers_upto_x, :153-177): words are read from
// `pos` in blocks of at most block_words, up to the first one whose masked value is above thr or to the end of the file.
// take() gives the block to read into (room for block_words words); use(block, e) is handed the block and the e words of it that
// belong to the slice, and returns false to stop the walk, in which case these e words do not count as handed over.
template <class Take, class Use>
SliceEnd walk_slice(const std::string& path, uint64_t pos, uint64_t words, uint64_t block_words, uint64_t thr, Take&& take, Use&& use) {
    Fd f;
    open_input(f, path);
    SliceEnd r;
    r.pos = pos;
    while (!r.above && r.pos < words) {
        uint64_t* h = take();
        const uint64_t cnt = std::min(block_words, words - r.pos);
        read_words(f.fd, h, r.pos, cnt, path);
        const uint64_t e = first_above(h, cnt, thr);
        if (!use(h, e)) break;
        if (e < cnt) r.above = true, r.head = h[e] & SORTED_KEY_MASK;
        r.pos += e;
    }
    return r;
}

}  // namespace kgwas
