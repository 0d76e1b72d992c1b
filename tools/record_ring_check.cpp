// record_ring_check.cpp - the record ring's offsets and policy (csrc/record_ring.h) against a plain model, the list of live
// intervals, under the sanitizers: seeded random sequences of fetches (give_back + place), publications, replays, feed
// boundaries and resets, as the feed loop (scan_replay.cpp) and fetch_records (scan_gpu.cpp) issue them, and the edges by hand.
// build: g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I kmersgwas_amd/csrc
//        tools/record_ring_check.cpp -o tools/bin/record_ring_check
// (a host-only program: run it on the CPU, on its own)
#include <cstdio>
#include <random>
#include <vector>

#include "record_ring.h"

using namespace kgwas;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond);      \
            failures++;                                                    \
        }                                                                  \
    } while (0)

static size_t need_of(size_t n) { return (n * 20 + 63) / 64 * 64; }

// A session as the ring sees it: chunks of the current feed are fetched, published and replayed in order, a slot keeps the
// ring_end of the chunk it holds (seq % n_slots), and the model keeps every interval somebody may still read.
struct Session {
    struct Live {
        size_t at, end;
        uint64_t feed, seq;
    };
    RecordRing rr;
    std::vector<size_t> ring_end;  // per slot
    std::vector<Live> live;
    uint64_t feed = 0, fetched = 0, published = 0, replayed = 0;
    size_t last_at = 0;
    uint64_t placements = 0;

    Session(size_t bytes, size_t n_slots, bool keep) : ring_end(n_slots, 0) {
        rr.set_size(bytes);
        rr.reset(keep);
        rr.begin_feed();
    }
    size_t& end_of(uint64_t seq) { return ring_end[(size_t)(seq % ring_end.size())]; }
    bool may_fetch() const { return fetched - replayed < ring_end.size(); }
    // what nobody reads any more: recycling - the chunks replayed; keep - nothing (the logs refer to every record)
    void drop_replayed() {
        if (rr.keep()) return;
        std::vector<Live> still;
        for (const Live& l : live)
            if (l.feed == feed && l.seq >= replayed) still.push_back(l);
        live.swap(still);
    }
    // fetch_records: false = no room (nothing was taken)
    bool fetch(size_t n) {
        const bool keep = rr.keep();
        const size_t tail_before = rr.tail();
        rr.give_back(replayed, [this](uint64_t q) { return end_of(q); });
        if (keep) CHECK(rr.tail() == tail_before && rr.tail() == 0);  // nothing is given back
        drop_replayed();
        const size_t head_before = rr.head();
        const size_t at = rr.place(n, fetched);
        if (at == RecordRing::NO_ROOM) {
            CHECK(n > 0);
            CHECK(rr.head() == head_before || (rr.head() == 0 && rr.tail() == 0));
            return false;
        }
        if (n) {
            const size_t end = at + need_of(n);
            CHECK(at % 64 == 0);
            CHECK(end <= rr.size());
            CHECK(rr.head() == end);
            for (const Live& l : live) CHECK(end <= l.at || l.end <= at);
            if (keep) CHECK(live.empty() || at >= last_at);  // offsets only grow
            last_at = at;
            live.push_back(Live{at, end, feed, fetched});
            placements++;
        }
        end_of(fetched) = rr.head();
        fetched++;
        return true;
    }
    void publish() {
        if (published < fetched) published++;
    }
    void replay() {
        if (replayed < published) replayed++;
    }
    // the ring ran full in keep mode and everything published is replayed: the logs take copies
    void to_recycling() {
        CHECK(replayed == published);
        rr.to_recycling(replayed, replayed ? end_of(replayed - 1) : 0);
        CHECK(!rr.keep());
        if (replayed) CHECK(rr.tail() == end_of(replayed - 1));
        drop_replayed();
    }
    // what the feed loop does when a fetch finds no room; false: nothing is left to wait for
    bool make_room() {
        if (published < fetched) {
            publish();
        } else if (rr.keep()) {
            replayed = published;
            to_recycling();
        } else if (replayed < published) {
            replay();
        } else {
            return false;
        }
        return true;
    }
    void end_feed() {
        published = fetched;
        replayed = fetched;
        drop_replayed();
        feed++;
        fetched = published = replayed = 0;
        rr.begin_feed();
        if (!rr.keep()) live.clear();
    }
    void reset(bool keep) {
        end_feed();
        live.clear();
        last_at = 0;
        rr.reset(keep);
        rr.begin_feed();
    }
};

static uint64_t random_sequences(uint32_t seed, uint64_t* placements) {
    std::mt19937_64 rng(seed);
    uint64_t sequences = 0;
    for (int round = 0; round < 400; round++, sequences++) {
        const size_t n_slots = 1 + rng() % 12;
        const size_t key_slots = 1 + rng() % 3000;  // a chunk's worst case
        const uint64_t slot_bytes = key_slots * 20;
        // the smallest ring the sizing function returns, a ring of a few chunks, or what it plans by itself (at least two chunks)
        const uint64_t forced = round % 3 == 0 ? 1 : round % 3 == 1 ? slot_bytes * (1 + rng() % 6) + rng() % 64 : 0;
        const size_t bytes = record_ring_bytes(n_slots, slot_bytes, forced);
        CHECK(bytes >= slot_bytes + 4096);
        if (!forced) CHECK(bytes >= 2 * slot_bytes + 4096);
        Session se(bytes, n_slots, rng() % 2 == 0);
        for (int step = 0; step < 600; step++) {
            const unsigned what = (unsigned)(rng() % 100);
            if (what < 50) {
                if (!se.may_fetch()) {
                    se.publish();
                    se.replay();
                    continue;
                }
                // no records (or an overflowed list: nothing is copied), a few, or up to the worst case
                const unsigned kind = (unsigned)(rng() % 10);
                const size_t n = kind < 2 ? 0 : kind < 7 ? 1 + rng() % (key_slots / 4 + 1) : 1 + rng() % key_slots;
                while (!se.fetch(n)) {
                    if (!se.make_room()) {
                        CHECK(false);  // everything placed is freed, and a chunk's worst case fits the smallest ring
                        break;
                    }
                }
            } else if (what < 70) {
                se.publish();
            } else if (what < 94) {
                se.replay();
            } else if (what < 98) {
                se.end_feed();
            } else if (what < 99) {
                se.reset(rng() % 2 == 0);
            } else {  // between feeds every column is materialised (an export, an import): the next feed recycles
                se.end_feed();
                se.rr.logs_released();
                se.live.clear();
                se.rr.begin_feed();
            }
        }
        // once everything placed is freed, a request of at most `size` bytes succeeds
        if (se.rr.keep()) {
            se.end_feed();
            se.rr.logs_released();
            se.live.clear();
            se.rr.begin_feed();
        } else {
            se.published = se.replayed = se.fetched;
        }
        const size_t n_max = se.rr.size() / 64 * 64 / 20;
        CHECK(need_of(n_max) <= se.rr.size());
        CHECK(se.fetch(n_max));
        *placements += se.placements;
    }
    return sequences;
}

// the rule in RecordRing::place: a chunk that shipped no records carries a ring_end taken from the old head
static void empty_chunk_keeps_the_tail() {
    Session se(8192, 8, false);
    CHECK(se.fetch(10));  // A: [0, 256)
    CHECK(se.fetch(0));   // B: no records, ring_end = 256
    CHECK(se.end_of(1) == 256);
    se.publish();
    se.replay();  // A is replayed, B is not
    // C: the ring is empty (tail == head == 256), but B is still to be freed: no starting over at the bottom
    CHECK(se.fetch(100));
    CHECK(se.live.back().at == 256);
    CHECK(se.fetch(40));  // D behind C
    se.published = se.replayed = 2;  // B is replayed: the tail stays where C begins
    CHECK(se.fetch(0));
    CHECK(se.rr.tail() == 256);
    se.published = se.replayed = se.fetched;
    CHECK(se.fetch(1));  // everything before it is freed: at the bottom again
    CHECK(se.live.back().at == 0);
}

static void edges() {
    {  // exactly the free space, and one byte over
        Session a(1280, 4, false), b(1279, 4, false);
        CHECK(a.fetch(64));   // 1280 bytes
        CHECK(!b.fetch(64));  // one byte over
        CHECK(!b.fetch(63));  // (1260 bytes take 1280 as well)
        CHECK(b.fetch(60));
    }
    {  // the wrapped ring is full at head == tail: exactly the gap is refused, a line less fits
        Session se(4096, 8, false);
        CHECK(se.fetch(51));   // A [0, 1024)
        CHECK(se.fetch(103));  // B [1024, 3136)
        se.publish();
        se.replay();           // A freed at the next fetch: tail 1024, 960 bytes behind the head
        CHECK(!se.fetch(51));  // wrap with tail == need: refused
        CHECK(se.rr.tail() == 1024 && se.rr.head() == 3136);
        CHECK(se.fetch(48));   // 960 bytes: exactly the room behind the head
        CHECK(se.live.back().at == 3136 && se.rr.head() == 4096);
        CHECK(se.fetch(47));   // wraps: 960 < tail 1024
        CHECK(se.live.back().at == 0);
        CHECK(!se.fetch(3));   // [960, 1024) is 64 bytes: head + need == tail is "full", refused
        CHECK(!se.fetch(4));
    }
    {  // the smallest ring: one slot's worst case + 4096 bytes holds a worst-case chunk, and the next once that is replayed
        const size_t key_slots = 1000;
        Session se(record_ring_bytes(4, key_slots * 20, 1), 4, true);
        CHECK(se.rr.size() == key_slots * 20 + 4096);
        CHECK(se.fetch(key_slots));
        CHECK(!se.fetch(key_slots));  // keep: linear, full
        CHECK(se.make_room());        // publish
        CHECK(se.make_room());        // replayed, logs detached: recycling
        CHECK(!se.rr.keep() && se.rr.tail() == se.end_of(0));
        CHECK(se.fetch(key_slots));
        CHECK(se.live.back().at == 0);
    }
    // the sizing: 8 worst-case chunks between 64 MiB and 1 GiB, never more than the slots hold, never less than two chunks
    CHECK(record_ring_bytes(48, 1 << 20, 0) == (48u << 20));
    CHECK(record_ring_bytes(48, 4 << 20, 0) == (64u << 20));
    CHECK(record_ring_bytes(48, 40 << 20, 0) == (320u << 20));
    CHECK(record_ring_bytes(8, 400ull << 20, 0) == (1ull << 30));
    CHECK(record_ring_bytes(4, 600ull << 20, 0) == (1200ull << 20) + 4096);
    CHECK(record_ring_bytes(48, 1 << 20, 5ull << 20) == (5u << 20));
}

int main() {
    uint64_t placements = 0, sequences = 0;
    for (uint32_t seed = 1; seed <= 5; seed++) sequences += random_sequences(seed, &placements);
    empty_chunk_keeps_the_tail();
    edges();
    printf("record_ring_check: %llu random sequences, %llu placements, %d failures\n", (unsigned long long)sequences, (unsigned long long)placements, failures);
    return failures ? 1 : 0;
}
