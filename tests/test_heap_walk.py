"""CPU tests of BestHeap's hole walks (csrc/heap.h) at the capacities where the walk changes its path: while a hole has all
four grandchildren (4 c + 6 < len) the push of a full heap of totally ordered scores resolves two levels per load, then it
goes on one level at a time and ends with the inner node that has a left child only. The capacities cover: no grandchildren
at all (N < 8), the first N with a full set (8), sets that exist for the left child only, len even and odd, walks that end
after an odd and after an even number of levels, and the headline's 10001. Each heap goes through kgwas_heap_new /
kgwas_heap_add_many / kgwas_heap_pop_all and is held against the oracle's literal std::priority_queue: identities and rows
in pop order, score bytes, and the count of effective pushes (ours: a record is one if the heap is not full or the record
beats the minimum the library reports before it; the oracle's: its own counter)."""
import ctypes as C

import numpy as np
import pytest

import kmersgwas_amd as kg
from kmersgwas_amd import capi
from oracle import binding as ob

CAPACITIES = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 14, 15, 16, 17, 22, 23, 30, 31, 32, 33, 62, 63, 64, 10001]
STREAMS = ["all_equal", "two_values", "ascending", "descending", "duplicates", "late_tie", "turns_negative", "turns_nan"]


def make_stream(kind, N, n, rng):
    if kind == "all_equal":
        return np.full(n, 2.5)
    if kind == "two_values":
        return np.where(rng.random(n) < 0.5, 1.0, 3.0)
    if kind == "ascending":
        return 1.0 + np.arange(n) * 0.125
    if kind == "descending":
        return 1.0 + np.arange(n, 0, -1) * 0.125
    if kind == "duplicates":  # 30 % of the records repeat an earlier record's score
        s = 10.0 + rng.random(n)
        dup = np.flatnonzero(rng.random(n) < 0.3)
        dup = dup[dup > 0]
        s[dup] = s[(rng.random(len(dup)) * dup).astype(np.int64)]
        return s
    if kind == "late_tie":  # all different, but for one of the N largest that comes again in the last 2 % of the stream
        s = 10.0 + rng.permutation(n) * 1e-3 + rng.random(n) * 1e-4
        tail = n // 50 + 1
        best = np.sort(s[: n - tail])[-min(N, n - tail):]
        s[n - 1 - rng.integers(0, tail)] = best[rng.integers(0, len(best))]
        return s
    # the heap is built with int64 compares; halfway the stream leaves +0 .. +inf and the double compares take over for good
    s = rng.integers(0, 64, n) * 0.25
    late = np.arange(n) >= n // 2
    s[late & (rng.random(n) < 0.25)] += 100.0
    odd = late & (rng.random(n) < 0.125)
    s[odd] = -rng.integers(0, 5, int(odd.sum())) * 0.5 if kind == "turns_negative" else np.nan
    return s


def feed_counting_pushes(h, N, k, s, r):
    """Record by record through kgwas_heap_add_many; the minimum is read again after every record that was a push."""
    lib, hp = capi.lib, h._h
    kp, sp, rp = k.ctypes.data, s.ctypes.data, r.ctypes.data
    size, low = C.c_uint64(0), C.c_double(0.0)
    ps, pl = C.byref(size), C.byref(low)
    pushes, lowest, filled = 0, 0.0, 0
    for i, x in enumerate(s.tolist()):
        push = filled < N or x > lowest
        assert lib.kgwas_heap_add_many(hp, kp + 8 * i, sp + 8 * i, rp + 8 * i, 1) == capi.KGWAS_OK
        if push:
            pushes += 1
            assert lib.kgwas_heap_size(hp, ps, None, pl) == capi.KGWAS_OK
            filled, lowest = size.value, low.value
    return pushes


@pytest.mark.parametrize("kind", STREAMS)
@pytest.mark.parametrize("N", CAPACITIES)
def test_hole_walks_equal_the_oracle_heap_at_the_walk_boundaries(N, kind):
    n = 20 * N + 7
    rng = np.random.default_rng(1000 * N + STREAMS.index(kind))
    s = np.ascontiguousarray(make_stream(kind, N, n, rng), np.float64)
    k = np.arange(n, dtype=np.uint64) + 1000
    r = np.arange(n, dtype=np.uint64) * 3
    h = kg.BestAssociationsHeap(N)
    pushes = feed_counting_pushes(h, N, k, s, r)
    o = ob.Heap(N)
    o.add_many(k, s, r)
    o_pops, o_pushes = C.c_uint64(), C.c_uint64()
    ob.lib().orc_heap_stats(C.c_void_p(o.h), C.byref(o_pops), C.byref(o_pushes))
    assert pushes == o_pushes.value
    assert len(h) == min(N, n) and np.float64(h.lowest_score).tobytes() == np.float64(o.lowest).tobytes()
    # pop_all: sorted where the scores alone decide, popped for real up to the last tie (int64 compares) or throughout
    # (pop_all_classic: a tie among the largest, a NaN or a negative score) - whichever this stream reaches
    for a, b in zip(h.pop_all(), o.pop_all()):
        assert a.tobytes() == b.tobytes()
