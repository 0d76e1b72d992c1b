"""The numpy model of the dead-pattern skip (lmm_skip_np.simulate) on hand-made lrt arrays, and the geometry of the fixture the GPU
tests of kgwas_lmm_test_table_multi_skip rely on. No GPU."""
import numpy as np
import pytest

import lmm_skip_np as K


def run(pattern, lrt, piece, chunk, N, rows=None, **kw):
    pattern = np.asarray(pattern)
    rows = np.arange(len(pattern)) if rows is None else rows
    trace = []
    out = K.simulate(pattern, rows, np.atleast_2d(np.asarray(lrt, float)), piece, chunk, N, trace=trace, **kw)
    assert out["rows_rotated"] + out["rows_skipped"] == len(pattern) and out["rows_rotated"] == len(trace)
    return out, trace


def test_nothing_dies_while_a_heap_is_open():
    # two patterns, the weak one first and often; N = 100 is never reached
    pattern = [0, 0, 1, 0, 0, 1, 0, 0]
    lrt = np.array([[0.1, 9.0][p] for p in pattern])
    out, trace = run(pattern, lrt, piece=2, chunk=1, N=100)
    assert out["patterns_dead"] == 0 and out["rows_skipped"] == 0 and out["pairs_shipped"] == 8 and all(s for _, s, _ in trace)
    # one open column among closed ones keeps every pattern alive: column 1 is NaN everywhere and N = 2 closes both after two rows,
    # with select off both count as open for ever
    both = np.stack([lrt, lrt])
    out, _ = run(pattern, both, piece=2, chunk=1, N=2, select=False)
    assert out["patterns_dead"] == 0 and out["rows_skipped"] == 0 and out["pairs_shipped"] == 16
    # with N = the number of rows no heap ever closes
    out, _ = run(pattern, both, piece=2, chunk=1, N=8)
    assert out["patterns_dead"] == 0 and out["rows_skipped"] == 0 and out["pairs_shipped"] == 16


def test_a_pattern_that_shipped_is_recomputed_and_may_die_later():
    # N = 1, pieces of 2 rows, one row per sub-chunk. Pattern 0 (lrt 5) ships at row 0 (open heap); at row 2 it is computed again
    # and ships nothing (5 > 5 is false): dead. Row 4 is skipped. Pattern 1 (lrt 7) ships at row 1, is computed at row 3: dead.
    pattern = [0, 1, 0, 1, 0, 1, 2]
    lrt = [5.0, 7.0, 5.0, 7.0, 5.0, 7.0, 1.0]
    out, trace = run(pattern, lrt, piece=2, chunk=1, N=1)
    assert trace == [(0, True, True), (1, True, False), (2, False, False), (3, False, False), (6, False, False)]
    assert out["rows_skipped"] == 2 and out["patterns_dead"] == 3 and out["patterns_cached"] == 3 and out["pairs_shipped"] == 2
    assert out["kept"] == [[1]]
    # the same rows in one piece: every row is computed (a row is skipped only in a later piece), the same heap
    one, _ = run(pattern, lrt, piece=100, chunk=1, N=1)
    assert one["rows_skipped"] == 0 and one["rows_rotated"] == 7 and one["kept"] == [[1]] and one["pairs_shipped"] == 2
    # a stale threshold: with the whole table in one sub-chunk the snapshot is the open heap's, and every pair ships
    stale, _ = run(pattern, lrt, piece=100, chunk=100, N=1)
    assert stale["pairs_shipped"] == 7 and stale["patterns_dead"] == 0 and stale["kept"] == [[1]]


def test_dead_is_absorbing():
    # pattern 0 dies in piece 1 (rows 2, 3) and is then skipped in every later piece, although a late threshold could not be lower
    pattern = [1, 1, 0, 0, 0, 1, 0, 0, 0, 0]
    lrt = [[9.0, 9.0, 1.0, 1.0, 1.0, 9.0, 1.0, 1.0, 1.0, 1.0]]
    out, trace = run(pattern, lrt, piece=2, chunk=2, N=2)
    assert [r for r, _, _ in trace] == [0, 1, 2, 3, 5] and out["rows_skipped"] == 5
    assert out["patterns_dead"] == 2 and out["kept"] == [[0, 1]]  # (pattern 1 dies at row 5: 9 > 9 is false)
    # the kept rows are those of a run that computes everything
    full, _ = run(pattern, lrt, piece=100, chunk=2, N=2)
    assert full["kept"] == out["kept"] and full["rows_skipped"] == 0


def test_the_block_edge():
    # 33 columns, N = 1: pattern 0 beats the threshold in column 32 alone - the second block of columns keeps it alive
    P = 33
    pattern = [1, 0, 0, 0]
    lrt = np.zeros((P, 4))
    lrt[:, 0] = 5.0            # pattern 1 closes every heap
    lrt[:32, 1:] = 1.0
    lrt[32, :] = [5.0, 6.0, 6.0, 6.0]
    out, trace = run(pattern, lrt, piece=1, chunk=1, N=1)
    # row 1 ships in column 32 (6 > 5); rows 2 and 3 then ship nothing (6 > 6 is false), row 2 marks, row 3 is skipped
    assert trace == [(0, True, True), (1, True, False), (2, False, False)] and out["rows_skipped"] == 1
    assert out["pairs_shipped"] == P + 1 and out["kept"][32] == [1] and out["kept"][0] == [0]
    # a flag taken after the first block of columns alone would kill pattern 0 at row 1
    wrong, _ = run(pattern, lrt, piece=1, chunk=1, N=1, flag_blocks=1)
    assert wrong["rows_skipped"] == 2 and wrong["pairs_shipped"] == P + 1 and wrong["rows_skipped"] != out["rows_skipped"]


def test_a_nan_lrt_ships_only_into_an_open_heap():
    out, trace = run([0, 1, 1, 1], [np.nan, np.nan, np.nan, np.nan], piece=1, chunk=1, N=1)
    assert trace == [(0, True, True), (1, False, False)] and out["rows_skipped"] == 2 and out["kept"] == [[0]]


@pytest.mark.parametrize("S,S_f", K.PANELS + [K.WIDE])
def test_fixture_geometry(S, S_f):
    """what the GPU tests rely on: fewer distinct tested patterns than half the tested rows, copies in the owner's piece and in
    later pieces, and - with hand-made lrts, one chi-square draw per (column, pattern) - at least one skipped row in every
    parametrisation that claims skipping"""
    f = K.fixture(S, S_f)
    n, distinct = len(f["rows"]), int(f["pattern"].max()) + 1
    assert 0 < distinct < n / 2
    first = {}
    for i, p in enumerate(f["pattern"]):
        first.setdefault(p, i)
    owner_row = f["rows"][[first[p] for p in f["pattern"]]]
    copy = np.arange(n) != np.array([first[p] for p in f["pattern"]])
    lrt = K.synthetic_lrt(f["pattern"], K.MAX_P, 5)
    for g, (forced, chunk) in enumerate(K.GEOMETRIES):
        piece = K.piece_of_geometry(f, g)
        assert (copy & (owner_row // piece == f["rows"] // piece)).any(), "no copy in its owner's piece"
        if forced:
            assert (f["rows"] // piece).max() >= 2 and (copy & (owner_row // piece < f["rows"] // piece)).any()
        for P, N in K.CASES[g]:
            out = K.simulate(f["pattern"], f["rows"], lrt[:P], piece, chunk, N)
            assert out["patterns_cached"] == distinct and out["rows_rotated"] + out["rows_skipped"] == n
            assert out["rows_skipped"] <= K.skip_bound(f["pattern"], f["rows"], piece, N)
            plain = K.simulate(np.arange(n), f["rows"], lrt[:P], piece, chunk, N)  # no pattern repeats: nothing is skipped
            assert plain["rows_skipped"] == 0 and plain["pairs_shipped"] == out["pairs_shipped"] and plain["kept"] == out["kept"]
            if K.claims_skipping(g, S):
                assert out["rows_skipped"] > 0 and out["patterns_dead"] > 0, (S, forced, chunk, P, N, out)
            if not forced:
                assert out["rows_skipped"] == 0
