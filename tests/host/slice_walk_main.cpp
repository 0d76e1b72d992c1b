// slice_walk_main.cpp — stand-alone check of sorted_file_io.h's walk_slice, open_input and open_output (tests/test_slice_walk.py
// builds it with the address and undefined-behaviour sanitizers and runs it).
//
// It writes small sorted files into the directory given as argv[1], walks them with plain std::vector blocks and compares what the
// walk handed over, the position and the head key it returned with the rule written out below as one loop over the whole file.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "sorted_file_io.h"

namespace kgwas {
void set_error(const std::string&) {}
}  // namespace kgwas

using namespace kgwas;

namespace {

int failures = 0;

#define CHECK(cond, ...)                          \
    do {                                          \
        if (!(cond)) {                            \
            failures++;                           \
            fprintf(stderr, "FAIL %s: ", #cond);  \
            fprintf(stderr, __VA_ARGS__);         \
            fprintf(stderr, "\n");                \
        }                                         \
    } while (0)

void write_file(const std::string& path, const std::vector<uint64_t>& w) {
    Fd f;
    open_output(f, path);
    write_all(f.fd, w.data(), w.size() * 8, path);
    close_output(f, path);
}

// The rule, straight: words from pos up to the first one whose masked value is above thr, or to the end of the file.
struct Expect {
    std::vector<uint64_t> handed;
    uint64_t pos;
    bool above;
    uint64_t head;
};
Expect straight(const std::vector<uint64_t>& file, uint64_t pos, uint64_t thr) {
    Expect x{{}, pos, false, 0};
    for (; x.pos < file.size(); x.pos++) {
        if ((file[x.pos] & SORTED_KEY_MASK) > thr) {
            x.above = true;
            x.head = file[x.pos] & SORTED_KEY_MASK;
            break;
        }
        x.handed.push_back(file[x.pos]);
    }
    return x;
}

// One walk of `file` (written at `path`) against the straight rule. stop_after: the caller refuses the block with that index
// (~0: never); the walk then ends with the blocks before it handed over.
void check_walk(const char* what, const std::string& path, const std::vector<uint64_t>& file, uint64_t pos, uint64_t block_words,
                uint64_t thr, uint64_t stop_after = ~0ull) {
    std::vector<uint64_t> block(block_words), handed;
    uint64_t takes = 0, uses = 0;
    const SliceEnd r = walk_slice(
        path, pos, file.size(), block_words, thr,
        [&] {
            takes++;
            std::fill(block.begin(), block.end(), 0xDEADBEEFDEADBEEFull);  // (nothing of an earlier block may be read again)
            return block.data();
        },
        [&](const uint64_t* h, uint64_t e) {
            CHECK(h == block.data(), "%s: a block that is not the caller's", what);
            CHECK(e <= block_words, "%s: e = %llu of a block of %llu", what, (unsigned long long)e, (unsigned long long)block_words);
            if (uses++ == stop_after) return false;
            handed.insert(handed.end(), h, h + e);
            return true;
        });
    CHECK(takes == uses, "%s: %llu blocks taken, %llu handed over", what, (unsigned long long)takes, (unsigned long long)uses);
    Expect x = straight(file, pos, thr);
    if (stop_after != ~0ull && stop_after < uses) {
        // stopped by the caller: exactly the whole blocks before the refused one count, and no head is reported
        const uint64_t n = stop_after * block_words;
        CHECK(n <= x.handed.size(), "%s: the refused block lies behind the slice", what);
        x.handed.resize(std::min<uint64_t>(n, x.handed.size()));
        x.pos = pos + x.handed.size();
        x.above = false;
        x.head = 0;
    }
    CHECK(handed == x.handed, "%s: %zu words handed over, %zu expected", what, handed.size(), x.handed.size());
    CHECK(r.pos == x.pos, "%s: pos %llu, expected %llu", what, (unsigned long long)r.pos, (unsigned long long)x.pos);
    CHECK(r.above == x.above, "%s: above %d, expected %d", what, (int)r.above, (int)x.above);
    if (x.above) CHECK(r.head == x.head, "%s: head %llx, expected %llx", what, (unsigned long long)r.head, (unsigned long long)x.head);
}

template <class F>
void check_throws(const char* what, int code, const std::string& text, F&& f) {
    try {
        f();
        CHECK(false, "%s: nothing thrown", what);
    } catch (const Error& e) {
        CHECK(e.code == code, "%s: code %d, expected %d", what, e.code, code);
        CHECK(std::string(e.what()) == text, "%s: message \"%s\", expected \"%s\"", what, e.what(), text.c_str());
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: slice_walk_main <scratch directory>\n");
        return 2;
    }
    const std::string dir = argv[1];
    const uint64_t CANON = 0x4000000000000000ull, NON = 0x8000000000000000ull;

    // twelve keys 10, 20 .. 120, every flag combination among them: unmasked, each word is above every threshold used below
    std::vector<uint64_t> file;
    for (uint64_t i = 1; i <= 12; i++) file.push_back(10 * i | (i % 3 == 0 ? CANON : i % 3 == 1 ? NON : CANON | NON));
    const std::string path = dir + "/twelve";
    write_file(path, file);

    for (uint64_t block_words : {1ull, 2ull, 3ull, 5ull, 12ull, 64ull})  // (12: the file is one block; 64: larger than the file)
        for (uint64_t pos : {0ull, 5ull, 11ull, 12ull})                   // (12: nothing is left)
            for (uint64_t thr : {0ull, 9ull, 10ull, 59ull, 60ull, 65ull, 90ull, 119ull, 120ull, 1000ull, (unsigned long long)SORTED_KEY_MASK}) {
                // thr 0, 9: below every key, a slice of zero words whose first word is already above thr (from any pos)
                // thr 60 from pos 0 with blocks of 1, 2, 3: the slice ends exactly on a block boundary, its head opens the next block
                // thr 120 and above: the slice ends with the file, there is no head word
                char what[96];
                snprintf(what, sizeof what, "block %llu pos %llu thr %llu", (unsigned long long)block_words, (unsigned long long)pos,
                         (unsigned long long)thr);
                check_walk(what, path, file, pos, block_words, thr);
            }
    // a threshold with flag bits set: the keys are compared masked, the threshold as it stands
    check_walk("thr with flag bits", path, file, 0, 4, 50 | CANON);

    // a caller that stops the walk: at the first block, behind the first block, and behind the block that holds the head
    for (uint64_t block_words : {1ull, 2ull, 3ull, 64ull})
        for (uint64_t stop_after : {0ull, 1ull, 2ull}) {
            char what[96];
            snprintf(what, sizeof what, "block %llu stopped at block %llu", (unsigned long long)block_words, (unsigned long long)stop_after);
            check_walk(what, path, file, 0, block_words, 65, stop_after);
            check_walk(what, path, file, 5, block_words, 1000, stop_after);
        }

    // one word
    const std::string one = dir + "/one";
    write_file(one, {7 | CANON});
    for (uint64_t thr : {6ull, 7ull}) check_walk("one word", one, {7 | CANON}, 0, 1, thr);

    // a file that is shorter than it was said to be
    check_throws("short file", KGWAS_ERR_IO, "read error on " + one + ": file got shorter", [&] {
        std::vector<uint64_t> block(4);
        walk_slice(one, 0, 3, 4, 100, [&] { return block.data(); }, [](const uint64_t*, uint64_t) { return true; });
    });

    // the messages of the open helpers
    const std::string missing = dir + "/no_such_file", nowhere = dir + "/no_such_dir/out";
    check_throws("open_input", KGWAS_ERR_FORMAT, "can't open file: " + missing, [&] {
        Fd f;
        open_input(f, missing);
    });
    check_throws("walk_slice on a missing file", KGWAS_ERR_FORMAT, "can't open file: " + missing, [&] {
        std::vector<uint64_t> block(4);
        walk_slice(missing, 0, 3, 4, 100, [&] { return block.data(); }, [](const uint64_t*, uint64_t) { return true; });
    });
    check_throws("open_output", KGWAS_ERR_IO, "can't open output file " + nowhere + ": " + std::strerror(ENOENT), [&] {
        Fd f;
        open_output(f, nowhere);
    });

    // the window helpers, against their definitions
    CHECK(kmers_step_to_threshold(5000, 31) == ((1ull << 62) - 1) / 5000 + 1, "kmers_step_to_threshold(5000, 31)");
    CHECK(kmers_step_to_threshold(5000, 1) == 1, "kmers_step_to_threshold(5000, 1)");
    for (uint64_t step : {1ull, 7ull})
        for (uint64_t x = 0; x < 30; x++) CHECK(window_of(x, step) == std::max<uint64_t>(1, (x + step - 1) / step), "window_of(%llu, %llu)", (unsigned long long)x, (unsigned long long)step);

    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    printf("slice walk OK\n");
    return 0;
}
