"""kgwas_fetch_reads_bases against fetch_np: the records and kmer_windows must be the model's, byte for byte.

The streams are 4096 t + {-1, 0, 1, k - 1, k} bytes long, t <= 3 (the kernels' tile is 4096 positions), and built from reads of
the lengths 0, 1, k - 1, k, k + 1 and 150, one of 4096 + k, one of about 9000 that spans three tiles, and reads that start and end
at a tile's edge and one byte either side of it; they carry N and lower case at and next to tile edges, planted hits that straddle
a tile's end on both strands, runs of hits for min_hits 2 and 5, and a palindrome where k is even. Each stream is a few KB, the
model runs once per stream and serves every min_hits."""
import numpy as np
import pytest

import kmersgwas_amd as kg
from kmersgwas_amd import capi

import fetch_np as FN

pytestmark = pytest.mark.gpu
TILE = 4096


def words_for(k, rng, n=40):
    if k == 1:
        return ["C"]
    if k == 2:
        return ["AC", "AT", "GG"]  # AT is a palindrome
    words, seen = [], set()
    half = "".join(rng.choice(list("ACGT"), k // 2))
    if k % 2 == 0:
        words.append(half + FN.revcomp(half))  # a palindrome
        seen.add(FN.canonical(words[0]))
    while len(words) < n:
        w = "".join(rng.choice(list("ACGT"), k))
        if FN.canonical(w) not in seen:
            seen.add(FN.canonical(w))
            words.append(w)
    return words


def make_stream(k, n, variant, rng, words, final_newline=True):
    """n bytes. variant 0: reads of at most 150 and newlines around every tile edge; 1: a read of 4096 + k behind the short ones;
    2: one of about 9000."""
    s = bytearray(rng.choice(np.frombuffer(b"ACGT", np.uint8), n).tobytes())
    newlines, at = [], 0
    for length in (0, 1, k - 1, k, k + 1, 150):
        at += length
        newlines.append(at)
        at += 1
    if variant == 1 and at + TILE + k < n:
        at += TILE + k
        newlines.append(at)
        at += 1
    if variant == 2 and at + 9000 < n:
        at += 9000 + k
        newlines.append(at)
        at += 1
    while at + 150 < n:
        at += int(rng.choice([150, 150, 150, 100, 151, k, 0]))
        newlines.append(at)
        at += 1
    edges = list(range(TILE, n, TILE))
    if variant == 0:
        for e in edges:  # reads that start and end at the edge, and one byte either side
            newlines += [e - 2, e - 1, e, e + 1 + 150 + (e // TILE)]
    plants = []
    if variant:
        for j, e in enumerate(edges):  # hits that straddle a tile's end, on both strands
            w = words[j % len(words)]
            plants.append((e - (k + 1) // 2 - (j & 1), w if j % 2 == 0 else FN.revcomp(w)))
        for e in edges[:1]:
            plants.append((e + 40, FN.revcomp(words[-1]).lower()))  # lower case next to the edge
    for i in range(30):  # hits anywhere, some in runs
        w = words[int(rng.integers(0, len(words)))]
        p = int(rng.integers(0, max(1, n - 7 * k)))
        for r in range(1 if i % 3 else 6):
            plants.append((p + r * k, w if i % 2 else FN.revcomp(w)))
    for p, w in plants:
        if 0 <= p and p + len(w) <= n:
            s[p:p + len(w)] = w.encode()
    for e in edges[1:2]:
        for p, b in ((e - 1, b"N"), (e, b"n"), (e + 1, b"N"), (e - 30, b"acgtacgt"), (e + 8, b"\r")):
            if p + len(b) <= n:
                s[p:p + len(b)] = b
    if variant:  # the long reads keep their planted hits: no newline inside them there
        newlines = [p for p in newlines if not any(q <= p < q + len(w) for q, w in plants[:len(edges) + 1])]
    for p in newlines:
        if 0 <= p < n:
            s[p] = 10
    s[n - 1] = 10 if final_newline else ord("A")
    return bytes(s)


def lengths_for(k):
    seen, out = set(), []
    for t in (1, 2, 3):
        for extra in (-1, 0, 1, k - 1, k):
            if t * TILE + extra not in seen:
                seen.add(t * TILE + extra)
                out.append(t * TILE + extra)
    return out


def same(got, exp, what):
    rec, n, win = got
    erec, ewin = exp
    assert n == len(erec), (what, n, len(erec))
    assert rec.tobytes() == erec[:len(rec)].tobytes(), (what, rec[:5], erec[:5])
    assert win.tolist() == ewin.tolist(), what


@pytest.mark.parametrize("k", [1, 2, 15, 16, 31])
def test_grid(k):
    rng = np.random.default_rng(100 + k)
    words = words_for(k, rng)
    codes = kg.kmer_codes(words, k)
    longest = 0
    for no, n in enumerate(lengths_for(k)):
        stream = make_stream(k, n, no % 3, rng, words)
        assert len(stream) == n
        reads = FN.per_read(stream, words)
        longest = max(longest, max(len(r) for r in FN.reads_of(stream)))
        for min_hits in (1, 2, 5):
            same(kg.fetch_reads_bases(stream, codes, k, min_hits), FN.fetch(stream, words, min_hits, reads), (k, n, min_hits))
    assert longest >= 9000


@pytest.fixture(scope="module")
def case31():
    k = 31
    rng = np.random.default_rng(7)
    words = words_for(k, rng)
    stream = make_stream(k, 3 * TILE + k, 0, rng, words)
    return {"k": k, "words": words, "codes": kg.kmer_codes(words, k), "stream": stream, "reads": FN.per_read(stream, words)}


def test_the_model_keeps_reads_in_the_shared_case(case31):
    rec, win = FN.fetch(case31["stream"], case31["words"], 1, case31["reads"])
    assert len(rec) > 20 and 2 <= len(FN.fetch(case31["stream"], case31["words"], 2, case31["reads"])[0]) < len(rec) and int(win.sum()) > 40
    assert set(rec["strand"].tolist()) == {0, 1}


@pytest.mark.parametrize("piece", [5000, 1000, 152])
def test_pieces_end_at_many_different_reads(monkeypatch, case31, piece):
    monkeypatch.setenv("KGWAS_FETCH_PIECE_BYTES", str(piece))
    for min_hits in (1, 2):
        same(kg.fetch_reads_bases(case31["stream"], case31["codes"], 31, min_hits), FN.fetch(case31["stream"], case31["words"], min_hits, case31["reads"]), piece)


def test_a_read_longer_than_a_piece_is_refused_with_its_length(monkeypatch, case31):
    monkeypatch.setenv("KGWAS_FETCH_PIECE_BYTES", "120")
    with pytest.raises(kg.KgwasError) as e:
        kg.fetch_reads_bases(case31["stream"], case31["codes"], 31)
    assert e.value.code == capi.KGWAS_ERR_ARG and "a read of 150 bytes does not fit a piece of 120 bytes" in e.value.msg, e.value.msg


def test_a_piece_drains_in_several_rounds(monkeypatch, case31):
    monkeypatch.setenv("KGWAS_FETCH_RECORDS", "7")
    same(kg.fetch_reads_bases(case31["stream"], case31["codes"], 31), FN.fetch(case31["stream"], case31["words"], 1, case31["reads"]), "rounds")
    monkeypatch.setenv("KGWAS_FETCH_PIECE_BYTES", "5000")
    same(kg.fetch_reads_bases(case31["stream"], case31["codes"], 31), FN.fetch(case31["stream"], case31["words"], 1, case31["reads"]), "rounds and pieces")


def test_cap_below_the_count(case31):
    erec, ewin = FN.fetch(case31["stream"], case31["words"], 1, case31["reads"])
    for cap in (0, 1, len(erec) - 1):
        rec, n, win = kg.fetch_reads_bases(case31["stream"], case31["codes"], 31, cap=cap)
        assert n == len(erec) and len(rec) == cap and rec.tobytes() == erec[:cap].tobytes() and win.tolist() == ewin.tolist()


def test_without_the_prefilter(monkeypatch, case31):
    monkeypatch.setenv("KGWAS_FETCH_PREFILTER", "0")
    for min_hits in (1, 2):
        same(kg.fetch_reads_bases(case31["stream"], case31["codes"], 31, min_hits), FN.fetch(case31["stream"], case31["words"], min_hits, case31["reads"]), "off")
    monkeypatch.setenv("KGWAS_FETCH_PREFILTER", "1")
    same(kg.fetch_reads_bases(case31["stream"], case31["codes"], 31), FN.fetch(case31["stream"], case31["words"], 1, case31["reads"]), "on")


def test_many_queries(monkeypatch):
    """2^16 queries: more than one list entry per splitter."""
    k = 31
    rng = np.random.default_rng(65536)
    raw = rng.integers(0, 4, (1 << 16, k))
    words = sorted({"".join("ACGT"[c] for c in row) for row in raw})
    canon = {}
    for w in words:
        canon.setdefault(FN.canonical(w), w)
    words = list(canon.values())
    rng.shuffle(words)
    assert len(words) > 65000
    stream = make_stream(k, 2 * TILE + k, 1, rng, words[:50] + words[-50:])
    monkeypatch.setenv("KGWAS_FETCH_PIECE_BYTES", "6000")
    for pre in ("1", "0"):
        monkeypatch.setenv("KGWAS_FETCH_PREFILTER", pre)
        same(kg.fetch_reads_bases(stream, kg.kmer_codes(words, k), k, 1), FN.fetch(stream, words, 1), "2^16 " + pre)


def test_two_letter_stream(monkeypatch):
    """Most windows hit: the prefilter passes nearly everything."""
    k = 3
    rng = np.random.default_rng(3)
    words = ["AAA", "AAC", "ACA", "ACC", "CAA", "CAC", "CCA"]  # every word over {A, C} but CCC
    s = bytearray(rng.choice(np.frombuffer(b"AC", np.uint8), 2 * TILE + 1).tobytes())
    for p in range(97, len(s), 101):
        s[p] = 10
    s[-1] = 10
    monkeypatch.setenv("KGWAS_FETCH_RECORDS", "16")
    for min_hits in (1, 90):
        exp = FN.fetch(bytes(s), words, min_hits)
        assert len(exp[0]) > 3
        same(kg.fetch_reads_bases(bytes(s), kg.kmer_codes(words, k), k, min_hits), exp, min_hits)


def test_a_stream_no_query_hits(case31):
    stream = (b"A" * 150 + b"\n") * 40 + b"NNNN\n\n"
    rec, n, win = kg.fetch_reads_bases(stream, case31["codes"], 31)
    assert n == 0 and len(rec) == 0 and win.tolist() == [0] * len(case31["words"])
    rec, n, win = kg.fetch_reads_bases(b"", case31["codes"], 31)
    assert n == 0 and win.tolist() == [0] * len(case31["words"])
    rec, n, win = kg.fetch_reads_bases(b"\n", case31["codes"], 31)
    assert n == 0


def test_a_stream_without_a_final_newline(monkeypatch, case31):
    k, words = 31, case31["words"]
    rng = np.random.default_rng(11)
    for n in (TILE, TILE + 1, 2 * TILE - 1):
        stream = make_stream(k, n, 0, rng, words, final_newline=False)
        tail = words[3] if n != TILE + 1 else FN.revcomp(words[4])
        stream = stream[:n - k] + tail.encode()  # the last read ends with a hit and no newline
        assert not stream.endswith(b"\n") and len(stream) == n
        same(kg.fetch_reads_bases(stream, case31["codes"], k), FN.fetch(stream, words), n)
    monkeypatch.setenv("KGWAS_FETCH_PIECE_BYTES", "1000")
    same(kg.fetch_reads_bases(stream, case31["codes"], k), FN.fetch(stream, words), "pieces")
