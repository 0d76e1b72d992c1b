// record_ring.h — the offsets and the policy of the session's pinned record ring: where a sparse chunk's candidate records
// (20 B each: score f64 | kmer u64 | row u32, three arrays) go in host memory, and when that room is free again. Host-only and
// free of HIP: the pinned buffer and its device address live beside it in the session (scan_internal.h), this class works on
// offsets, and tools/record_ring_check.cpp drives it on a CPU.
//
// ONE pinned ring: a chunk takes exactly its 20 B x candidates when its counts are known and gives them back when it is
// replayed (FIFO). Slots used to own worst-case buffers (cap x P records each), which capped the chunks in flight at 12 for
// 201 columns: with host and GPU level the GPU then idled while the host digested the ramp.
//
// Threads: everything here belongs to the control thread (the caller of a feed) - except `keep`, which the replay workers read
// (acquire, replay_group) to know whether a chunk's records may be referred to where they lie.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdint>

namespace kgwas {

// Pinning memory is slow - 1 GiB takes 0.21-0.25 s, two thirds of a session's creation (KGWAS_TRACE), and every other
// allocation of the process queues behind it, so a thread of its own does not hide it: the ring is sized for what the scan
// plans to have in flight instead of the cap. A chunk is planned to fill 40 % of the key list (next_sparse_chunk) and the GPU
// runs up to ~16 chunks ahead of the replay: 20 planned chunks' records (8 x a slot's worst case), at least 64 MiB and two
// worst-case chunks, at most 1 GiB - 390 MB at 101 columns (top-10001), 775 MB at 201. A ring that fills up only makes the GPU
// wait for the replay (fetch_records).
// slot_bytes: a chunk's worst case (20 B x the key list); forced (KGWAS_RING_BYTES, 0: unset): tests ask for a ring barely
// larger than one chunk's worst case, so that it wraps and fills up.
inline size_t record_ring_bytes(uint64_t n_slots, uint64_t slot_bytes, uint64_t forced) {
    if (forced) return (size_t)std::max<uint64_t>(forced, slot_bytes + 4096);
    return (size_t)std::max<uint64_t>(std::min<uint64_t>(1ull << 30, std::min<uint64_t>(n_slots * slot_bytes, std::max<uint64_t>(64ull << 20, 8 * slot_bytes))),
                                      2 * slot_bytes + 4096);
}

// The three arrays of n records placed at `at` in a ring that begins at `base` (the host address or the mapped device address)
struct RecordPtrs {
    double* score;
    uint64_t* kmer;
    uint32_t* row;
};
inline RecordPtrs record_ptrs(uint8_t* base, size_t at, size_t n) {
    return RecordPtrs{reinterpret_cast<double*>(base + at), reinterpret_cast<uint64_t*>(base + at + n * 8), reinterpret_cast<uint32_t*>(base + at + n * 16)};
}

class RecordRing {
   public:
    static constexpr size_t NO_ROOM = ~(size_t)0;
    void set_size(size_t bytes) { size_ = bytes; }
    size_t size() const { return size_; }
    size_t head() const { return head_; }  // behind the chunk placed last: that chunk's `ring_end`
    size_t tail() const { return tail_; }
    // Columns in select mode keep their sparse chunks' records where the GPU wrote them (LazyCol::Seg): while this is set the
    // ring is filled linearly and nothing is given back - from one reset() to the next, across feeds. Should it run full
    // (to_recycling), the logs take copies of what they refer to and the ring recycles as it does for sessions that replay
    // every column; from then on the workers copy each chunk's records into the logs.
    bool keep(std::memory_order o = std::memory_order_relaxed) const { return keep_.load(o); }

    // A new scan: nothing refers to the ring any more; a session in select mode fills it linearly.
    void reset(bool keep) {
        head_ = tail_ = 0;
        keep_.store(keep, std::memory_order_release);
    }
    // No log is left (every column was materialised between two feeds): the next feed recycles the ring.
    void logs_released() { keep_.store(false, std::memory_order_release); }
    // Chunk sequence numbers restart with every feed: nothing is in flight between feeds.
    void begin_feed() {
        if (keep())
            tail_ = 0;  // (the records of earlier feeds stay: the columns' logs refer to them)
        else
            head_ = tail_ = 0;
        feed_start_ = head_;
        freed_ = 0;
    }
    // Give back what the replay has finished with: the chunks [0, replayed) of this feed (chunks are replayed, hence freed, in
    // order). end_of(seq): the head as it stood behind chunk seq's place() - its slot's ring_end; call this before that slot's
    // value is overwritten by the chunk being fetched.
    template <class EndOf>
    void give_back(uint64_t replayed, EndOf&& end_of) {
        if (keep()) freed_ = replayed;  // (the logs refer to the records: nothing is given back)
        while (freed_ < replayed) {
            tail_ = end_of(freed_);
            freed_++;
        }
    }
    // Room for chunk seq's n records (rounded up to 64 bytes; 0 records take none and always fit): their offset, or NO_ROOM
    // (nothing is taken: retry after more chunks are replayed and given back).
    size_t place(size_t n_records, uint64_t seq) {
        // empty: start over at the bottom - but only when every chunk fetched before this one has been freed: a fetched,
        // not yet replayed chunk without records (or one that overflowed) carries a ring_end taken from the old head,
        // and freeing it later would move the tail back over records placed at the bottom in the meantime
        if (!keep() && tail_ == head_ && freed_ == seq) head_ = tail_ = 0;
        const size_t need = (n_records * 20 + 63) / 64 * 64;
        size_t at;
        if (keep()) {  // linear: [0, head) is referred to by the columns' logs
            if (size_ - head_ < need) return NO_ROOM;  // (the caller lets the replay catch up, then to_recycling)
            at = head_;
        } else if (head_ >= tail_) {  // used part does not wrap (or the ring is empty)
            if (size_ - head_ >= need)
                at = head_;
            else if (tail_ > need)  // wrap: the bytes up to the end stay unused until this chunk is freed
                at = 0;
            else
                return NO_ROOM;
        } else {
            if (tail_ - head_ > need)
                at = head_;
            else
                return NO_ROOM;
        }
        head_ = at + need;
        return at;
    }
    // The ring has run full while the columns' logs refer to its records. Called when every published chunk is replayed (no
    // worker is inside a column) and the logs have taken their copies: the ring is recycled from here on - free up to the end
    // of the last replayed chunk (end_of_last_replayed; none replayed: up to where the feed began); chunks that are fetched
    // but not yet published keep their records where they are and are copied into the logs when their turn comes.
    void to_recycling(uint64_t replayed, size_t end_of_last_replayed) {
        keep_.store(false, std::memory_order_release);
        tail_ = replayed ? end_of_last_replayed : feed_start_;
        freed_ = replayed;
    }

   private:
    size_t size_ = 0, head_ = 0, tail_ = 0;  // used: [tail, head) circularly; head == tail: empty
    size_t feed_start_ = 0;                  // head when the current feed began
    uint64_t freed_ = 0;                     // chunks (of this feed) whose records have been given back
    std::atomic<bool> keep_{false};
};

}  // namespace kgwas
