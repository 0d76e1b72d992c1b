"""filter_kmers on the GPU (filter_kernels.hip, filter_kmers.cpp, bin/filter_kmers) against the restatement (filter_kmers_np.py).

Every case checks the library's rows (file_rows and the raw rows), the library's output file and - where the list is given as
words - the tool's output file, byte for byte. KGWAS_INGEST_PIECE_ROWS=128 cuts tables into many pieces, so runs of equal
keys cross piece boundaries and descents fall on row 1, inside a piece, on a piece's first row, and more than once."""
import os
import subprocess

import numpy as np
import pytest

import kmersgwas_amd as kg
from oracle import oracle_np as onp
import filter_kmers_np as fk

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "kmersgwas_amd", "bin", "filter_kmers")
M64 = (1 << 64) - 1


def canonical(codes, k):
    """kmer2bits of bits2kmer31(code, k), vectorised: min(code, reverse complement) of the low 2k bits."""
    x = np.asarray(codes, np.uint64) & np.uint64((1 << (2 * k)) - 1 if k < 32 else M64)
    b = x.copy()
    for sh, m in ((32, 0xFFFFFFFF00000000), (16, 0xFFFF0000FFFF0000), (8, 0xFF00FF00FF00FF00), (4, 0xF0F0F0F0F0F0F0F0),
                  (2, 0xCCCCCCCCCCCCCCCC)):
        x = ((x & np.uint64(m)) >> np.uint64(sh)) | ((x & np.uint64(~m & M64)) << np.uint64(sh))
    rc = (~x) >> np.uint64(64 - 2 * k)
    return np.minimum(b, rc)


def test_canonical_helper_matches_the_restatement():
    rng = np.random.default_rng(5)
    for k in (1, 10, 31, 32):
        c = rng.integers(0, 1 << 63, size=200, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
        words = [fk.bits2kmer31(int(v), k) for v in c]
        assert [int(v) for v in canonical(c, k)] == [fk.kmer2bits(w) for w in words]


def table_rows(keys, S_f, seed):
    rng = np.random.default_rng(seed)
    W = (S_f + 63) // 64
    rows = np.empty((len(keys), 1 + W), np.uint64)
    rows[:, 0] = keys
    rows[:, 1:] = rng.integers(0, 1 << 63, size=(len(keys), W), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(len(keys), W), dtype=np.uint64)
    if S_f % 64:
        rows[:, W] &= np.uint64((1 << (S_f % 64)) - 1)
    return rows


def check(tmp_path, rows, S_f, k, codes=None, words=None, cli=True, tag="x"):
    """Library (rows and file) on `codes`, or on the codes of `words`, and the tool on `words`, against the restatement."""
    names = ["acc%d" % i for i in range(S_f)]
    base = str(tmp_path / ("tab_" + tag))
    onp.write_table(base, names, k, rows[:, 0], rows[:, 1:])
    if codes is None:
        codes = canonical(words, k)  # (words are given as codes; their text is bits2kmer31)
    codes = np.asarray(codes, np.uint64)
    emitted, want = fk.expected_output(names, k, rows, sorted(int(c) for c in codes))
    tbl = kg.KmersTable(base, k)
    fr, rr = kg.filter_kmers(tbl, codes)
    assert fr.dtype == np.uint64 and np.array_equal(fr, emitted)
    assert np.array_equal(rr, rows[emitted.astype(np.int64)].reshape(-1, rows.shape[1]))
    out = str(tmp_path / ("lib_%s.tsv" % tag))
    assert kg.filter_kmers_write(out, tbl, codes) == len(emitted)
    tbl.close()
    with open(out, "rb") as f:
        got = f.read()
    assert len(got) == len(want) and got == want, "library output differs"
    if cli and words is not None:
        lst = str(tmp_path / ("list_%s.txt" % tag))
        w = np.asarray(words, np.uint64)
        with open(lst, "wb") as f:
            f.write(fk.lines_bytes(w.reshape(-1, 1), k, 0))  # one bits2kmer31 word per line
        out = str(tmp_path / ("cli_%s.tsv" % tag))
        r = subprocess.run([BIN, "-t", base, "-k", lst, "-o", out], capture_output=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout == b""
        err = r.stderr.decode().splitlines()
        assert err[0] == "We have %d" % len(rows) and err[-1].startswith("[kgwas] seconds:") and len(err) == 2
        with open(out, "rb") as f:
            got = f.read()
        assert len(got) == len(want) and got == want, "tool output differs"
    return emitted


def runs_table(n_rows, S_f, k, seed, descents=()):
    """Ascending canonical keys in runs of 1..300 equal keys, with the rows at `descents` set below their predecessor."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 300, size=n_rows)
    lens[rng.random(n_rows) < 0.6] = 1
    vals = np.unique(canonical(rng.integers(0, 1 << 62, size=n_rows, dtype=np.uint64), k))
    keys = np.repeat(vals, lens[:len(vals)])[:n_rows]
    if len(keys) < n_rows:
        keys = np.concatenate([keys, np.full(n_rows - len(keys), keys[-1], np.uint64)])
    keys = keys.copy()
    for d in descents:
        keys[d] = keys[d - 1] - np.uint64(1) if keys[d - 1] > 0 else keys[d - 1]
        assert keys[d] < keys[d - 1]
    return table_rows(keys, S_f, seed + 1)


def list_from(rows, rng, n, present=0.7):
    """n codes: keys of the table (each possibly repeated) and codes absent from it."""
    keys = np.unique(rows[:, 0])
    pick = keys[rng.integers(0, len(keys), size=int(n * present))]
    absent = rng.integers(0, 1 << 62, size=n - len(pick), dtype=np.uint64)
    return np.concatenate([pick, absent])[rng.permutation(n)]


# ---- panel widths and k -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S_f", [1, 63, 64, 65, 1135, 4097, 12000])
def test_panel_widths(S_f, tmp_path, monkeypatch):
    monkeypatch.setenv("KGWAS_INGEST_PIECE_ROWS", "1024")
    rng = np.random.default_rng(S_f)
    rows = runs_table(3000, S_f, 31, seed=S_f)
    words = canonical(list_from(rows, rng, 1500), 31)
    assert len(check(tmp_path, rows, S_f, 31, words=words)) > 0


@pytest.mark.parametrize("k", [10, 31, 32])
def test_kmer_lengths(k, tmp_path, monkeypatch):
    monkeypatch.setenv("KGWAS_INGEST_PIECE_ROWS", "512")
    rng = np.random.default_rng(k)
    rows = runs_table(4000, 70, k, seed=100 + k)
    words = list_from(rows, rng, 3000)
    words = canonical(words, k)
    assert len(check(tmp_path, rows, 70, k, words=words)) > 0


# ---- list sizes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 1000, 20000, (1 << 21) + 3])
def test_list_sizes(n, tmp_path):
    rng = np.random.default_rng(n)
    rows = runs_table(12000, 130, 31, seed=7)
    words = canonical(list_from(rows, rng, n, present=0.5 if n < (1 << 20) else 0.01), 31)
    if n == 1:
        words = rows[[5000], 0].copy()
    emitted = check(tmp_path, rows, 130, 31, words=words)
    assert len(emitted) > 0


# ---- pieces of 128 rows: runs across boundaries, descents ---------------------------------------------------------------------
@pytest.mark.parametrize("descents", [(), (1,), (300,), (256,), (128, 129), (1, 200, 384, 900), tuple(range(130, 1500, 97))])
def test_descents_across_pieces(descents, tmp_path, monkeypatch):
    monkeypatch.setenv("KGWAS_INGEST_PIECE_ROWS", "128")
    rng = np.random.default_rng(len(descents) * 31 + (descents[0] if descents else 0))
    rows = runs_table(2000, 65, 31, seed=17, descents=descents)
    keys = np.unique(rows[:, 0])
    # duplicates in the list: every key present 0 to 4 times, against runs of up to 300 equal rows
    reps = rng.integers(0, 5, size=len(keys))
    words = np.concatenate([np.repeat(keys, reps), rng.integers(0, 1 << 62, size=200, dtype=np.uint64)])
    words = canonical(words[rng.permutation(len(words))], 31)
    check(tmp_path, rows, 65, 31, words=words)


def test_a_descent_changes_the_answer(tmp_path, monkeypatch):
    """Rows 5, 9 x 127 | 3, 3, 5, 5, 11 ... against the list {3, 5, 11}, the descent on a piece's first row: the reference emits
    rows 0 and 132 only (set intersection would add rows 128 to 131 and every other 11)."""
    monkeypatch.setenv("KGWAS_INGEST_PIECE_ROWS", "128")
    keys = np.array([5] + [9] * 127 + [3, 3, 5, 5] + [11] * 200, np.uint64)
    rows = table_rows(keys, 3, 1)
    assert list(check(tmp_path, rows, 3, 4, words=np.array([3, 5, 11], np.uint64))) == [0, 132]


def test_list_used_up_then_descent(tmp_path, monkeypatch):
    monkeypatch.setenv("KGWAS_INGEST_PIECE_ROWS", "128")
    keys = np.concatenate([np.arange(10, 300, dtype=np.uint64), np.arange(5, 400, dtype=np.uint64)])
    rows = table_rows(keys, 64, 2)
    emitted = check(tmp_path, rows, 64, 10, codes=np.array([20, 20, 299, 7, 8], np.uint64))
    assert list(emitted) == [10, 289]


# ---- keys ---------------------------------------------------------------------------------------------------------------------
def test_non_canonical_keys_and_high_bits(tmp_path, monkeypatch):
    """Keys that are not canonical and keys with bits above 2k: the library matches the codes it is given exactly; the tool's
    words are canonical, and a key's printed text is its low 2k bits."""
    monkeypatch.setenv("KGWAS_INGEST_PIECE_ROWS", "256")
    rng = np.random.default_rng(23)
    k = 10
    raw = np.sort(rng.integers(0, 1 << (2 * k), size=3000, dtype=np.uint64))
    high = np.sort(rng.integers(1 << (2 * k), 1 << 40, size=500, dtype=np.uint64))
    keys = np.concatenate([raw, high])
    rows = table_rows(keys, 100, 3)
    assert (canonical(raw, k) != raw).any()
    codes = np.concatenate([raw[::3], high[::5], canonical(raw[1::7], k)])
    emitted = check(tmp_path, rows, 100, k, codes=codes, tag="lib")
    assert (keys[emitted.astype(np.int64)] != canonical(keys[emitted.astype(np.int64)], k)).any()
    assert (keys[emitted.astype(np.int64)] >= np.uint64(1 << (2 * k))).any()
    check(tmp_path, rows, 100, k, words=canonical(raw[::2], k), tag="cli")


def test_no_match_gives_a_header_only_file(tmp_path):
    rows = runs_table(5000, 65, 31, seed=29)
    keys = set(int(x) for x in rows[:, 0])
    words = np.array([c for c in range(1, 4000, 3) if c not in keys], np.uint64)
    assert len(check(tmp_path, rows, 65, 31, words=words)) == 0
    with open(str(tmp_path / "cli_x.tsv"), "rb") as f:
        assert f.read() == fk.header(["acc%d" % i for i in range(65)])


def test_every_row_matches(tmp_path, monkeypatch):
    monkeypatch.setenv("KGWAS_INGEST_PIECE_ROWS", "384")
    rows = runs_table(6000, 200, 31, seed=31)
    assert len(check(tmp_path, rows, 200, 31, words=rows[:, 0].copy())) == 6000


def test_every_row_matches_past_the_text_budget(tmp_path):
    """12 500 rows x 12 000 accessions, all emitted: 300 MB of text, more than one piece's text budget (256 MiB)."""
    rng = np.random.default_rng(37)
    keys = np.sort(rng.choice(1 << 40, size=12500, replace=False)).astype(np.uint64)
    rows = table_rows(keys, 12000, 37)
    assert len(check(tmp_path, rows, 12000, 31, codes=keys, cli=False)) == 12500


# ---- a table of more than 2^21 rows at the default piece size -------------------------------------------------------------------
def test_large_table_default_piece(tmp_path):
    rng = np.random.default_rng(41)
    n = (1 << 21) + 4321
    keys = np.sort(canonical(rng.integers(0, 1 << 62, size=n, dtype=np.uint64), 31))
    keys[1::9] = keys[0::9][:len(keys[1::9])]  # runs of two
    keys = np.sort(keys)
    rows = table_rows(keys, 1, 41)
    words = canonical(list_from(rows, rng, 100000, present=0.8), 31)
    emitted = check(tmp_path, rows, 1, 31, words=words)
    assert len(emitted) > 50000
