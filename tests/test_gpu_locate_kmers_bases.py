"""kgwas_locate_kmers_bases, the array level of locate_kmers, against locate_np: the records must be the model's, byte for byte.

The grid is k in {2, 15, 16, 31} (the least, an odd and an even split into halves, the most) x d in {0, 1}. Streams are a few tiles
of 4096 positions long, 4096 t + {-1, 0, 1, k - 1, k}, so windows end on, straddle and follow a tile's end; they carry separators
at and next to tile and piece boundaries and lower case. KGWAS_LOCATE_PIECE_BYTES is set so that planted hits straddle piece
boundaries, KGWAS_LOCATE_RECORDS so that a piece drains in several rounds, and cap lies below the count of all records. The
queries are planted ones (exact, one mismatch in either half, reverse-complemented, palindromes, many sharing one half) and random
ones that hit nothing. Beside the grid: 2^16 queries (lists longer than one block of splitters), a two-letter stream where most
windows hit something, a stream shorter than k, and the bases taken from a torch tensor on the device."""
import ctypes as C

import numpy as np
import pytest

import kmersgwas_amd as kg
from kmersgwas_amd import capi

import locate_np as LN

pytestmark = pytest.mark.gpu
TILE = 4096
_model = {}  # (stream, queries, d) -> the model's records, computed once


def model(stream, queries, d):
    key = (bytes(stream), tuple(queries), d)
    if key not in _model:
        _model[key] = LN.locate(stream, queries, d)[0]
    return _model[key]


def word(rng, k, letters="ACGT"):
    return "".join(rng.choice(list(letters), k))


def make_stream(rng, n, k, piece):
    """n bytes: random bases, some lower case, separators at and next to the tile and piece boundaries - but for the first boundary
    of either kind and its surroundings, which stay clean so that windows straddle them"""
    s = rng.choice(np.frombuffer(b"ACGT", np.uint8), n)
    low = rng.random(n) < 0.1
    s[low] |= 0x20
    clean = (TILE, piece)
    others = sorted({e for m in (TILE, piece) for e in range(2 * m, n + 2, m)})
    for no, edge in enumerate(others):
        at = edge + (-1, 0, 1)[no % 3]
        if 0 <= at < n and all(abs(at - c) > k + 1 for c in clean):
            s[at] = (ord("N"), ord("\n"), ord("n"), 0)[no % 4]
    for at in rng.integers(0, n, 3):
        if all(abs(at - c) > k + 1 for c in clean):
            s[at] = ord("N")
    return s


def plant(rng, s, k, piece, n_random=60):
    """queries for the stream s (changed in place where a palindrome is planted)"""
    n = len(s)
    text = lambda p: bytes(s[p:p + k]).decode("latin-1").upper()
    ok = lambda w: len(w) == k and not set(w) - set("ACGT")
    queries, seen = [], set()

    def add(w):
        if ok(w) and LN.canonical(w) not in seen:
            seen.add(LN.canonical(w))
            queries.append(w)

    def change(w, j):
        return w[:j] + rng.choice([c for c in "ACGT" if c != w[j]]) + w[j + 1:]

    if k % 2 == 0 and k >= 4:  # palindromes: a half and its reverse complement, planted across a tile's end and elsewhere
        for p in (TILE - k // 2, 1000):
            half = word(rng, k // 2)
            pal = half + LN.revcomp(half)
            if p + k <= n:
                s[p:p + k] = np.frombuffer(pal.encode(), np.uint8)
                add(pal)
    # windows that end on, straddle and follow the tile and piece boundaries, and random ones
    starts = [e + o for m in (TILE, piece) for e in range(m, n, m) for o in (-k, -k + 1, -(k // 2), -1, 0, 1)]
    starts += rng.integers(0, max(1, n - k), 40).tolist()
    for no, p in enumerate(starts):
        if p < 0 or p + k > n or not ok(text(p)):
            continue
        w = text(p)
        kind = no % 6
        if kind == 1:
            w = change(w, int(rng.integers(0, (k + 1) // 2)))  # one mismatch in the first half
        elif kind == 2 and k > 1:
            w = change(w, int(rng.integers((k + 1) // 2, k)))  # ... in the last half
        elif kind == 3:
            w = LN.revcomp(w)
        elif kind == 4:
            w = LN.revcomp(change(w, int(rng.integers(0, k))))
        add(w)
    if k >= 15:  # many queries that share one half with a window of the stream, and so lie in one range of equal half keys
        base = next(text(p) for p in range(50, n) if ok(text(p)))
        hh = (k + 1) // 2
        add(base)
        for _ in range(60):
            add(base[:hh] + word(rng, k - hh))
            add(word(rng, hh) + base[hh:])
            add(LN.revcomp(base[:hh] + word(rng, k - hh)))
        for j in range(k):  # its neighbours at every base: the window of `base` hits all of them with d = 1
            add(change(base, j))
    for _ in range(n_random if k >= 15 else 2):
        add(word(rng, k))
    return queries


def call(stream, queries, k, d, cap=None):
    codes = kg.kmer_codes(queries, k)
    return kg.locate_kmers_bases(stream, codes, k, d, cap=cap)


def same(rec, exp):
    assert rec.dtype == exp.dtype == kg.LOCATE_RECORD == LN.RECORD
    assert len(rec) == len(exp), (len(rec), len(exp))
    assert rec.tobytes() == exp.tobytes(), "first difference at record %d" % next(i for i in range(len(rec)) if rec[i] != exp[i])


@pytest.mark.parametrize("d", [0, 1])
@pytest.mark.parametrize("k,tiles,piece,records", [(2, 3, 3000, 1000), (15, 3, 2500, 7), (16, 3, 2048, 50), (31, 3, 1371, 11)])
def test_grid(monkeypatch, k, d, tiles, piece, records):
    monkeypatch.setenv("KGWAS_LOCATE_PIECE_BYTES", str(piece))
    monkeypatch.setenv("KGWAS_LOCATE_RECORDS", str(records))
    total = 0
    for delta in (-1, 0, 1, k - 1, k):
        rng = np.random.default_rng(1000 * k + 10 * d + delta)
        n = TILE * tiles + delta
        s = make_stream(rng, n, k, piece)
        queries = plant(rng, s, k, piece)
        exp = model(s, queries, d)
        rec, count = call(s, queries, k, d)
        assert count == len(exp)
        same(rec, exp)
        total += count
        if delta == 0 and count > 3:  # cap below the count: the first cap records, nothing behind them
            cap = count // 2
            out = np.zeros(cap + 3, kg.LOCATE_RECORD)
            out["pad"] = 0xEE
            n_out = C.c_uint64(0)
            codes = kg.kmer_codes(queries, k)
            capi.check(capi.lib.kgwas_locate_kmers_bases(capi.ptr(s), len(s), 0, capi.ptr(codes), len(codes), k, d, 0, capi.ptr(out), cap, C.byref(n_out)))
            assert n_out.value == count and out[:cap].tobytes() == exp[:cap].tobytes() and (out["pad"][cap:] == 0xEE).all()
    assert total > (50 if k > 2 else 1000), "the fixture plants nothing"
    if k >= 15:
        kinds = model(s, queries, d)
        assert (kinds["strand"] == 1).any() and (d == 0 or (kinds["mismatches"] == 1).any())


def test_hits_straddle_tiles_and_pieces():
    """what the grid's fixture is for, stated on its own: at d = 1 and k = 31 there are records whose window crosses a tile's end and
    a piece's end, and a window with more than one record"""
    k, piece = 31, 1371
    rng = np.random.default_rng(1000 * k + 10)
    s = make_stream(rng, 3 * TILE, k, piece)
    exp = model(s, plant(rng, s, k, piece), 1)
    pos = exp["pos"].astype(np.int64)
    assert ((pos < TILE) & (pos + k > TILE)).any() and ((pos < piece) & (pos + k > piece)).any()
    assert (np.unique(pos, return_counts=True)[1] > 1).any()


def test_many_queries(monkeypatch):
    """2^16 queries: 2^17 patterns, 64 entries per splitter"""
    k, d = 16, 1
    monkeypatch.setenv("KGWAS_LOCATE_PIECE_BYTES", "3000")
    monkeypatch.setenv("KGWAS_LOCATE_RECORDS", "100")
    rng = np.random.default_rng(65536)
    s = make_stream(rng, TILE + k, k, 3000)
    queries = plant(rng, s, k, 3000, n_random=0)
    seen = {LN.canonical(q) for q in queries}
    codes = rng.integers(0, 1 << (2 * k), 70000, dtype=np.uint64)
    for c in codes.tolist():
        w = "".join("ACGT"[(c >> (2 * (k - 1 - j))) & 3] for j in range(k))
        if len(queries) < 1 << 16 and LN.canonical(w) not in seen:
            seen.add(LN.canonical(w))
            queries.append(w)
    assert len(queries) == 1 << 16
    order = rng.permutation(len(queries))  # the planted ones anywhere among the others
    queries = [queries[i] for i in order]
    exp = model(s, queries, d)
    # not vacuous: the window `base` alone hits itself and its k neighbours, and the boundary windows add theirs; the hits' queries lie
    # all over the shuffled list, so their patterns lie in many blocks of the sorted lists
    assert len(exp) > k + 1 and len(np.unique(exp["kmer"] // 2048)) > 16
    rec, count = call(s, queries, k, d)
    assert count == len(exp)
    same(rec, exp)


def test_two_letter_stream(monkeypatch):
    """k = 8 over A and C alone: most windows hit something and many hit several queries"""
    k = 8
    monkeypatch.setenv("KGWAS_LOCATE_PIECE_BYTES", "5000")
    monkeypatch.setenv("KGWAS_LOCATE_RECORDS", "1000")
    rng = np.random.default_rng(8)
    s = rng.choice(np.frombuffer(b"ACac", np.uint8), 2 * TILE + 5, p=[0.45, 0.45, 0.05, 0.05])
    s[[TILE - 1, 5000, 7000]] = ord("N")
    queries = sorted({word(rng, k, "AC") for _ in range(100)})
    for d in (0, 1):
        exp = model(s, queries, d)
        rec, count = call(s, queries, k, d)
        assert count == len(exp)
        same(rec, exp)
    windows = len(s) - k + 1
    assert len(np.unique(exp["pos"])) > windows // 2 and len(exp) > 2 * windows


def test_a_stream_shorter_than_k():
    for s in (b"", b"ACG", b"ACGTACGTACGTAC"):
        rec, count = call(s, ["ACGTACGTACGTACG"], 15, 1)
        assert count == 0 and len(rec) == 0


def test_bases_on_the_device(monkeypatch):
    """the stream in a torch tensor on the GPU: no copy of the pieces; a piece size that is no multiple of 16 leaves every other piece
    unaligned for the 16-byte loads"""
    import torch
    k, d, piece = 31, 1, 1371
    monkeypatch.setenv("KGWAS_LOCATE_PIECE_BYTES", str(piece))
    monkeypatch.setenv("KGWAS_LOCATE_RECORDS", "11")
    rng = np.random.default_rng(1000 * k + 10 * d)
    s = make_stream(rng, 3 * TILE, k, piece)
    queries = plant(rng, s, k, piece)
    exp = model(s, queries, d)
    t = torch.from_numpy(s).cuda()
    rec, count = call(t, queries, k, d)
    assert count == len(exp) and len(exp) > 100
    same(rec, exp)
    rec, count = call(t[3:], queries, k, d)  # a base pointer that is itself unaligned
    exp3 = model(s[3:], queries, d)
    assert count == len(exp3)
    same(rec, exp3)
    rec, _ = call(torch.from_numpy(s), queries, k, d)  # a tensor on the host
    same(rec, exp)
