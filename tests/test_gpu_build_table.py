"""build_kmers_table on the GPU (build_kernels.hip, build_table.cpp, bin/build_kmers_table) against the restatement
(build_table_np.py): <o>.table and <o>.names of the library call and of the tool, byte for byte.

KGWAS_BUILD_PIECE_ROWS forces small pieces (runs of whole windows), KGWAS_BUILD_BLOCK_WORDS small read blocks, so that slices,
duplicates, empty slices and descents meet piece and block boundaries. Small cases are checked against the literal form as well as
the closed form (which test_build_table.py pins to it)."""
import os
import re
import subprocess

import numpy as np
import pytest

import kmersgwas_amd as kg
import build_table_np as bt
import filter_kmers_np as fk
from test_build_table import random_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "kmersgwas_amd", "bin", "build_kmers_table")
U = np.uint64


def write_inputs(d, all_words, acc):
    os.makedirs(d, exist_ok=True)
    allk = os.path.join(d, "all.kmers")
    np.asarray(all_words, "<u8").tofile(allk)
    paths, names = [], []
    for c, w in enumerate(acc):
        p = os.path.join(d, "a%d.sorted" % c)
        np.asarray(w, "<u8").tofile(p)
        paths.append(p)
        names.append("acc_%d" % c)
    lst = os.path.join(d, "list.txt")
    with open(lst, "w") as f:
        for p, nm in zip(paths, names):
            f.write("%s\t%s\n" % (p, nm))
    return allk, paths, names, lst


def check(tmp_path, all_words, acc, k, piece_rows=None, block_words=None, cli=True, tag="x", literal=None):
    """The library and the tool on these inputs against the restatement; returns the expected rows."""
    all_words = np.asarray(all_words, U)
    acc = [np.asarray(a, U) for a in acc]
    d = str(tmp_path / tag)
    allk, paths, names, lst = write_inputs(d, all_words, acc)
    rows = bt.closed_rows(all_words, acc, k)
    if literal is None:
        literal = len(all_words) + sum(len(a) for a in acc) <= 30000 and len(acc) <= 130  # (5001 windows x S calls in Python)
    if literal:
        assert bt.literal_rows(all_words, acc, k).tolist() == rows.tolist(), "the closed form differs from the literal form"
    want_table = bt.table_bytes(rows, len(acc), k)
    want_names = "".join(n + "\n" for n in names).encode()
    env = {}
    if piece_rows:
        env["KGWAS_BUILD_PIECE_ROWS"] = str(piece_rows)
    if block_words:
        env["KGWAS_BUILD_BLOCK_WORDS"] = str(block_words)
    old = {v: os.environ.get(v) for v in ("KGWAS_BUILD_PIECE_ROWS", "KGWAS_BUILD_BLOCK_WORDS")}
    try:
        for v in old:
            os.environ.pop(v, None)
        os.environ.update(env)
        out = os.path.join(d, "lib")
        assert kg.build_kmers_table(allk, paths, names, k, out) == len(rows)
    finally:
        for v, val in old.items():
            os.environ.pop(v, None)
            if val is not None:
                os.environ[v] = val
    with open(out + ".table", "rb") as f:
        got = f.read()
    assert len(got) == len(want_table) and got == want_table, "library .table differs (%s, pieces %s, blocks %s)" % (tag, piece_rows, block_words)
    with open(out + ".names", "rb") as f:
        assert f.read() == want_names
    if cli:
        out = os.path.join(d, "cli")
        e2 = {v: val for v, val in os.environ.items() if v not in old}
        e2.update(env)
        r = subprocess.run([BIN, "-l", lst, "-k", str(k), "-a", allk, "-o", out], capture_output=True, timeout=900, env=e2)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout == b""
        err = r.stderr.decode()
        assert err.startswith("".join(bt.MILESTONES) + "[kgwas] seconds:") and len(err.splitlines()) == 4
        assert re.search(r" rows=%d$" % len(rows), err.splitlines()[-1])
        with open(out + ".table", "rb") as f:
            got = f.read()
        assert len(got) == len(want_table) and got == want_table, "tool .table differs (%s)" % tag
        with open(out + ".names", "rb") as f:
            assert f.read() == want_names
    return rows


def ascending_case(rng, S, k, n, per_acc, dup=0.1):
    """n all-k-mers keys spread over the 2k-bit key space (some repeated), S accessions of about per_acc keys: members of the
    list, other keys, some files wholly inside a few windows (so many of their slices are empty)."""
    top = (1 << (2 * k)) - 1
    a = np.sort(rng.integers(0, top, size=n, dtype=U, endpoint=True))
    rep = rng.random(n) < dup
    a[1:][rep[1:]] = a[:-1][rep[1:]]
    a = np.sort(a)
    acc = []
    for c in range(S):
        m = max(1, int(rng.integers(1, 2 * per_acc)))
        pick = rng.choice(a, size=m)
        other = rng.integers(0, top, size=max(1, m // 4), dtype=U, endpoint=True)
        w = np.sort(np.concatenate([pick, other]))
        if c % 7 == 3:  # a narrow file: keys of a short stretch of the list only
            i = int(rng.integers(0, n))
            w = np.sort(rng.choice(a[i:i + 5], size=m))
        acc.append(w | (rng.integers(0, 4, size=len(w), dtype=U) << U(62)))
    return a | (rng.integers(0, 4, size=n, dtype=U) << U(62)), acc


@pytest.mark.parametrize("k", [10, 17, 31])
@pytest.mark.parametrize("S", [1, 63, 64, 65, 1135, 4097])
def test_widths_and_lengths_small_pieces(S, k, tmp_path):
    rng = np.random.default_rng(1000 * k + S)
    n = 300 if S < 1000 else 200
    all_words, acc = ascending_case(rng, S, k, n, 60 if S < 1000 else 12)
    if k == 10:  # keys above the last threshold end a file's use (k = 10: step * 5001 = 1 050 210)
        all_words = np.concatenate([all_words, np.array([1050211, 1050300], U)])
        acc[0] = np.concatenate([acc[0], np.array([1050211, 1050300], U)])
    rows = check(tmp_path, all_words, acc, k, piece_rows=37, block_words=16, tag="small")
    assert rows[:, 1:].any()
    if S <= 65:
        check(tmp_path, all_words, acc, k, tag="default", cli=False)
        check(tmp_path, all_words, acc, k, piece_rows=1, block_words=1, tag="one", cli=False)


def test_accessions_wholly_above_or_below_the_list(tmp_path):
    rng = np.random.default_rng(4)
    a = np.sort(rng.integers(1 << 40, 1 << 50, size=500, dtype=U))
    acc = [np.sort(rng.integers(0, 1 << 39, size=300, dtype=U)),        # wholly below
           np.sort(rng.integers(1 << 51, 1 << 61, size=300, dtype=U)),  # wholly above
           a[::3].copy(), np.array([a[0]], U), np.array([a[-1]], U), np.array([0], U), np.array([bt.MASK], U)]
    for pr, bw in ((None, None), (64, 32), (7, 5)):
        rows = check(tmp_path, a, acc, 31, piece_rows=pr, block_words=bw, tag="ab_%s" % pr)
        assert not (rows[:, 1] & U(0b1100011)).any() and int(rows[0, 1]) == 0b01100 and int(rows[-1, 1]) == 0b10000


def test_duplicates_in_the_all_kmers_file(tmp_path):
    rng = np.random.default_rng(6)
    vals = np.sort(rng.integers(0, 1 << 62, size=80, dtype=U))
    a = np.repeat(vals, rng.integers(1, 9, size=80))  # runs of up to 8 equal keys, crossing piece boundaries
    acc = [vals[::2].copy(), vals[1::2].copy(), np.repeat(vals, 3), vals[:1].copy()]
    for pr in (None, 16, 3):
        rows = check(tmp_path, a, acc, 31, piece_rows=pr, block_words=8, tag="dup_%s" % pr)
        first = np.concatenate([[True], a[1:] != a[:-1]])
        assert (rows[~first, 1] == 0).all() and (rows[first, 1] != 0).all()


# k = 10: step 210; windows 1 = 0..210, 2 = 211..420, 3 = 421..630, 4 = 631..840
DESCENTS = {
    "same_window_bit_set": ([7], [[5, 100, 7]]),
    "at_word_1_accession": ([3, 9, 250], [[9, 3, 250]]),
    "at_word_1_all": ([9, 3, 250], [[3, 9, 250], [9]]),
    "all_alone": ([10, 20, 15, 220, 230, 225, 430], [[10, 15, 20, 220, 225, 230, 430], [15, 225]]),
    "accession_alone": ([10, 15, 20, 220, 225, 230, 430], [[10, 20, 15, 220, 230, 225, 430], [10, 230]]),
    "both": ([10, 20, 15, 220, 230, 225, 430], [[20, 10, 15, 230, 220, 225, 430], [430, 15]]),
    "several_per_file": ([10, 30, 20, 40, 35, 220, 210, 230, 225, 640, 430], [[40, 30, 20, 10, 230, 225, 220, 640, 35, 430], [35, 30, 640, 210]]),
    "back_to_an_earlier_window_no_bit": ([7, 300, 500], [[300, 7], [7, 500, 300], [500, 7, 300]]),
    # pieces of 4 rows: windows 1-2, then 3-4; a descent in the last window of the first piece / the first window of the next
    "last_window_of_a_piece": ([10, 20, 220, 230, 430, 440, 650, 660], [[10, 230, 220, 430], [230, 220, 20]]),
    "first_window_of_the_next_piece": ([10, 20, 220, 230, 430, 440, 650, 660], [[10, 220, 440, 430, 650], [440, 430, 230]]),
    "all_kmers_in_both_places": ([10, 20, 230, 220, 440, 430, 650, 660], [[10, 220, 230, 430, 440, 650], [230, 220, 440, 430]]),
}


@pytest.mark.parametrize("name", sorted(DESCENTS))
def test_descents_by_hand(name, tmp_path):
    all_words, acc = DESCENTS[name]
    for pr, bw in ((None, None), (4, 2), (1, 1), (2, 3)):
        rows = check(tmp_path, all_words, acc, 10, piece_rows=pr, block_words=bw, tag="%s_%s" % (name, pr), cli=pr in (None, 4))
    if name == "same_window_bit_set":
        assert rows.tolist() == [[7, 1]]
    if name == "back_to_an_earlier_window_no_bit":
        # accession 0's 7 and accession 1's and 2's 300 come after a larger key: they count for its window, where the list has no such key
        assert rows.tolist() == [[7, 0b010], [300, 0b001], [500, 0b110]]


def test_random_cases_with_descents(tmp_path):
    rng = np.random.default_rng(77)
    for i in range(60):
        k = int(rng.choice([10, 11, 15, 31]))
        all_words, acc = random_case(rng, k)
        pr = [None, 1, 2, 3, 5, 8, 50][int(rng.integers(0, 7))]
        bw = [None, 1, 2, 7, 64][int(rng.integers(0, 5))]
        check(tmp_path, all_words, acc, k, piece_rows=pr, block_words=bw, tag="r%d" % i, cli=i % 10 == 0)


@pytest.mark.parametrize("piece_rows", [None, 64])
def test_crowded_and_spread_keys(piece_rows, tmp_path):
    """Keys 1..n at k = 31 all lie in window 1 (larger than a forced piece: the host's loop makes it); spread keys beside them."""
    rng = np.random.default_rng(9)
    n = 1500
    crowded = np.arange(1, n + 1, dtype=U)
    acc_c = [crowded[rng.random(n) < 0.25] for _ in range(70)]
    acc_c[5] = crowded[::-1].copy()  # (and one descending file)
    rows = check(tmp_path, crowded, acc_c, 31, piece_rows=piece_rows, block_words=100, tag="crowded")
    assert (rows[:, 1] >> U(5) & U(1)).all()
    spread = np.sort(rng.integers(0, 1 << 62, size=n, dtype=U))
    acc_s = [spread[rng.random(n) < 0.25] for _ in range(70)]
    check(tmp_path, spread, acc_s, 31, piece_rows=piece_rows, block_words=100, tag="spread")
    both = np.concatenate([crowded, spread[spread > n]])
    check(tmp_path, both, [np.concatenate([x, y[y > n]]) for x, y in zip(acc_c[:5], acc_s)], 31, piece_rows=piece_rows, block_words=100,
          tag="both")


def test_large_case_default_pieces_and_round_trip(tmp_path):
    """About 10^5 rows x 1135 accessions at bit density 0.25, default pieces; then the built table is read back."""
    rng = np.random.default_rng(2024)
    n, S, k = 100000, 1135, 31
    a = np.unique(rng.integers(0, 1 << 62, size=n, dtype=U))
    n = len(a)
    bits = rng.random((S, n)) < 0.25
    acc = []
    for c in range(S):
        extra = rng.integers(0, 1 << 62, size=50, dtype=U)  # keys that are not in the list
        acc.append(np.sort(np.concatenate([a[bits[c]], extra])))
    rows = check(tmp_path, a, acc, k, tag="large", literal=False)
    packed = np.packbits(bits.T, axis=1, bitorder="little")
    packed = np.concatenate([packed, np.zeros((n, 8 * ((S + 63) // 64) - packed.shape[1]), np.uint8)], axis=1)
    assert np.array_equal(rows[:, 1:], packed.view("<u8").reshape(n, -1)) and np.array_equal(rows[:, 0], a)
    # round trip: the table opens, and filter_kmers over it returns the rows that were put in
    base = str(tmp_path / "large" / "cli")
    tbl = kg.KmersTable(base, k)
    assert tbl.n_rows == n and tbl.words_per_row == (S + 63) // 64 and list(tbl.names) == ["acc_%d" % c for c in range(S)]
    sel = np.sort(rng.choice(n, size=2000, replace=False))
    fr, rr = kg.filter_kmers(tbl, a[sel])
    tbl.close()
    assert np.array_equal(fr, sel.astype(U)) and np.array_equal(rr, rows[sel])
    assert fk.lines_bytes(rr[:3], k, S) == fk.lines_bytes(rows[sel[:3]], k, S)
