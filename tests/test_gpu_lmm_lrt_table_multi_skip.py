"""lmm_lrt --pattern_skip (kgwas_lmm_test_table_multi_skip, the lmm_pattern_* and lmm_skip_* kernels of lmm_table_kernels.hip): in the multi-phenotype
table pass a pattern of which a fully computed row shipped no pair is dead, and later pieces leave its rows out.

The yardstick everywhere is kgwas_lmm_test_table_multi on the same handle and table, at the same piece and chunk_variants: the
kept rows of every column, their k-mers, lrt, lambda, p and af, logl0 and lambda0 are compared by their raw bytes, rows_read,
rows_tested and pairs_shipped as numbers. There is no tolerance. The counters are compared with lmm_skip_np.simulate, which walks
the pieces, sub-chunks and column blocks in numpy on the lrts of a yardstick run with N = the number of rows (which keeps every
tested row), wherever nothing is rejected and no tag collides."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kmersgwas_amd as kg
from kmersgwas_amd import capi
from oracle import oracle_np as onp

import lmm_skip_np as K
import lmm_table_np as T
import lmm_unique_np as Q

pytestmark = pytest.mark.gpu
BINDIR = os.path.join(os.path.dirname(os.path.abspath(capi.__file__)), "bin")
FIELDS = ("lrt", "lambda", "p", "af")
COUNTERS = ("slots", "patterns_cached", "patterns_dead", "rows_skipped", "rows_collided", "rows_rejected", "rows_rotated")
MODELLED = ("patterns_cached", "patterns_dead", "rows_skipped", "rows_rotated")


def columns(y, P, seed=11):
    """y and P - 1 seeded permutations of it"""
    rng = np.random.default_rng(seed)
    return np.stack([y] + [rng.permutation(y) for _ in range(P - 1)])


def set_piece(monkeypatch, piece):
    if piece is None:
        monkeypatch.delenv("KGWAS_LMM_PIECE_ROWS", raising=False)
    else:
        monkeypatch.setenv("KGWAS_LMM_PIECE_ROWS", str(piece))


def assert_same(res, yard, what):
    assert len(res["columns"]) == len(yard["columns"])
    for j, (got, exp) in enumerate(zip(res["columns"], yard["columns"])):
        assert got["row"].tolist() == exp["row"].tolist(), "%s column %d: other rows (n_kept %d, %d)" % (what, j, len(got["row"]), len(exp["row"]))
        assert got["kmer"].tolist() == exp["kmer"].tolist(), "%s column %d: other k-mers" % (what, j)
        for k in FIELDS:
            assert got[k].tobytes() == exp[k].tobytes(), "%s column %d: %s differs in its bytes" % (what, j, k)
    for k in ("logl0", "lambda0"):
        assert res[k].tobytes() == yard[k].tobytes(), "%s: %s differs in its bytes" % (what, k)
    for k in ("rows_read", "rows_tested", "pairs_shipped"):
        assert res[k] == yard[k], "%s: %s is %d, kgwas_lmm_test_table_multi's %d" % (what, k, res[k], yard[k])
    u = res["skip"]
    assert u["rows_rotated"] + u["rows_skipped"] == res["rows_tested"], (what, u)
    assert u["patterns_dead"] <= u["patterns_cached"] <= u["slots"], (what, u)


class Case:
    """A table on disk, open, with one handle per chunk_variants, and the lrt of every (column, tested row) from the yardstick."""

    def __init__(self, tmp_path, table, S_f, pick, K_, Y, mc, name="tab"):
        names = ["acc%d" % i for i in range(S_f)]
        self.base = str(tmp_path / name)
        onp.write_table(self.base, names, T.K_LEN, table[:, 0], table[:, 1:])
        self.acc = [names[i] for i in pick]
        self.table, self.pick, self.K, self.Y, self.mc = table, np.asarray(pick, np.uint64), K_, Y, mc
        self.tbl = kg.KmersTable(self.base, T.K_LEN)
        self.handles = {}
        self._full = None

    def handle(self, chunk):
        if chunk not in self.handles:
            self.handles[chunk] = kg.LmmLrt(self.K, chunk_variants=chunk)
        return self.handles[chunk]

    def yard(self, P, N, chunk, Y=None):
        return self.handle(chunk).test_table_multi(self.tbl, self.pick, (self.Y if Y is None else Y)[:P], self.mc, Q.MAF, N)

    def skip(self, P, N, chunk, slots=4096, Y=None):
        return self.handle(chunk).test_table_multi_skip(self.tbl, self.pick, (self.Y if Y is None else Y)[:P], self.mc, Q.MAF, N, slots)

    def full(self):
        """(rows, lrt [P][tested rows]) of all columns: N = the number of rows keeps every tested row, in row order"""
        if self._full is None:
            res = self.yard(len(self.Y), len(self.table), 10240)
            rows = res["columns"][0]["row"].astype(np.int64)
            assert len(rows) == res["rows_tested"] and all(c["row"].tolist() == rows.tolist() for c in res["columns"])
            self._full = (rows, np.stack([c["lrt"] for c in res["columns"]]))
        return self._full

    def close(self):
        for m in self.handles.values():
            m.close()
        self.tbl.close()


def fixture_case(tmp_path, monkeypatch, S, S_f, P=K.MAX_P):
    f = K.fixture(S, S_f)
    K_, y = T.kinship_and_phenotype(S)
    c = Case(tmp_path, f["table"], S_f, f["pick"], K_, columns(y, P), f["mc"])
    set_piece(monkeypatch, None)
    rows, lrt = c.full()
    assert rows.tolist() == f["rows"].tolist(), "the tested rows are not those of the numpy rule"
    for a, b in zip(*np.nonzero(f["pattern"][:, None] == f["pattern"][None, :200])):  # equal patterns, equal bits in every column
        assert lrt[:, a].tobytes() == lrt[:, b].tobytes()
    return f, c, lrt


def check_against_model(c, f, lrt, monkeypatch, g, P, N, what, claims, slots=4096, runs=1):
    forced, chunk = K.GEOMETRIES[g]
    piece = K.piece_of_geometry(f, g)
    model = K.simulate(f["pattern"], f["rows"], lrt[:P], piece, chunk, N)
    if claims:
        assert model["rows_skipped"] > 0 and model["patterns_dead"] > 0, "%s: the model expects no skipped row" % what
    set_piece(monkeypatch, forced)
    yard = c.yard(P, N, chunk)
    assert yard["pairs_shipped"] == model["pairs_shipped"], "%s: the model's walk is not the host's" % what
    out = [c.skip(P, N, chunk, slots) for _ in range(runs)]
    for res in out:
        assert_same(res, yard, what)
        u = res["skip"]
        print(what, u, "shipped", res["pairs_shipped"])
        assert u["slots"] == slots and u["rows_rejected"] == 0 and u["rows_collided"] == 0, (what, u)
        assert {k: u[k] for k in MODELLED} == {k: model[k] for k in MODELLED}, (what, u, model)
    assert all(r["skip"] == out[0]["skip"] for r in out), "%s: the counters of two runs differ" % what
    return model


# ---- 1. panels, pieces, chunks, P and N ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,S_f", K.PANELS)
def test_equals_test_table_multi(tmp_path, monkeypatch, S, S_f):
    monkeypatch.delenv("KGWAS_LMM_PATTERN_TAG_BITS", raising=False)
    monkeypatch.delenv("KGWAS_LMM_TABLE_SELECT", raising=False)
    f, c, lrt = fixture_case(tmp_path, monkeypatch, S, S_f)
    try:
        for g in range(len(K.GEOMETRIES)):
            for i, (P, N) in enumerate(K.CASES[g]):
                what = "S=%d S_f=%d piece %s chunk %d P %d N %d" % ((S, S_f) + K.GEOMETRIES[g] + (P, N))
                before = c.handle(K.GEOMETRIES[g][1]).stats()
                check_against_model(c, f, lrt, monkeypatch, g, P, N, what, K.claims_skipping(g, S), runs=2 if i == 0 else 1)
                after = c.handle(K.GEOMETRIES[g][1]).stats()
                calls = 3 if i == 0 else 2  # the yardstick and the runs with the table: a tested row counts once per column in each
                assert after["variants_tested"] - before["variants_tested"] == calls * P * len(f["rows"]), what
    finally:
        c.close()


def test_code_rows_wider_than_a_wave(tmp_path, monkeypatch):
    """1135 accessions: a code row of 71 dwords, so the hash and the compare take a second round of lanes"""
    monkeypatch.delenv("KGWAS_LMM_PATTERN_TAG_BITS", raising=False)
    monkeypatch.delenv("KGWAS_LMM_TABLE_SELECT", raising=False)
    f, c, lrt = fixture_case(tmp_path, monkeypatch, *K.WIDE, P=3)
    try:
        check_against_model(c, f, lrt, monkeypatch, 1, 3, 7, "S=1135 piece 1000 chunk 64 P 3 N 7", True)
    finally:
        c.close()


# ---- 2. the edge between two blocks of columns ---------------------------------------------------------------------------------
@pytest.fixture
def repeated67(tmp_path, monkeypatch):
    monkeypatch.delenv("KGWAS_LMM_PATTERN_TAG_BITS", raising=False)
    monkeypatch.delenv("KGWAS_LMM_TABLE_SELECT", raising=False)
    f, c, lrt = fixture_case(tmp_path, monkeypatch, 67, 70)
    yield f, c, lrt
    c.close()


def test_the_only_shipped_pair_is_in_column_33(repeated67, monkeypatch):
    """P = 33: for some row computed with every heap closed the only pair that ships is the one of the last column, the second
    block's only one. The column order that makes it so is searched in numpy on the yardstick's lrts. Its pattern must stay live:
    a flag read after the first block alone would kill it, and the model says what that would show."""
    f, c, lrt = repeated67
    g, N = 0, 7
    forced, chunk = K.GEOMETRIES[g]
    piece = K.piece_of_geometry(f, g)
    found = None
    for last in range(K.MAX_P):
        order = [k for k in range(K.MAX_P) if k != last] + [last]
        blocks = []
        model = K.simulate(f["pattern"], f["rows"], lrt[order], piece, chunk, N, block_trace=blocks)
        edge = [r for r, was_open, per_block in blocks if not was_open and tuple(per_block) == (False, True)]
        wrong = K.simulate(f["pattern"], f["rows"], lrt[order], piece, chunk, N, flag_blocks=1)
        if edge and wrong["rows_skipped"] != model["rows_skipped"]:
            found = (order, model, wrong, edge)
            break
    assert found is not None, "no column order ships a row's only pair in column 33"
    order, model, wrong, edge = found
    print("column %d last: %d rows ship in column 33 alone; rows_skipped %d, %d with the flag of the first block alone"
          % (order[-1], len(edge), model["rows_skipped"], wrong["rows_skipped"]))
    set_piece(monkeypatch, forced)
    Y = c.Y[order]
    yard = c.yard(K.MAX_P, N, chunk, Y=Y)
    res = c.skip(K.MAX_P, N, chunk, Y=Y)
    assert_same(res, yard, "the block edge")
    assert yard["pairs_shipped"] == model["pairs_shipped"]
    assert {k: res["skip"][k] for k in MODELLED} == {k: model[k] for k in MODELLED}, (res["skip"], model)


# ---- 3. open heaps: nothing dies -----------------------------------------------------------------------------------------------
def test_no_heap_ever_closes(repeated67, monkeypatch):
    f, c, lrt = repeated67
    set_piece(monkeypatch, 1024)
    n = len(f["rows"])
    for P, N, select in ((33, Q.ROWS, "1"), (33, n, "1"), (3, 7, "0")):
        monkeypatch.setenv("KGWAS_LMM_TABLE_SELECT", select)
        yard, res = c.yard(P, N, 32), c.skip(P, N, 32)
        assert_same(res, yard, "N %d select %s" % (N, select))
        u = res["skip"]
        assert u["rows_skipped"] == 0 and u["patterns_dead"] == 0 and u["rows_rotated"] == n, u
        assert res["pairs_shipped"] == P * n and u["patterns_cached"] == int(f["pattern"].max()) + 1


def test_a_zero_lrt_under_an_open_heap_does_not_kill(tmp_path, monkeypatch):
    """An open heap ships every pair, also one whose lrt is not above the 0.0 the host uploads as its threshold. The fixture makes
    such pairs: 64 accessions in 32 pairs, a kinship matrix that does not change when the two of a pair are swapped, patterns that
    are constant on every pair and phenotypes that change sign under the swap. Then the pattern is orthogonal to the phenotype at
    every lambda, the likelihoods with and without it are one number, and lrt = fmax(0, 2 (l - l0)) is 0.0. With N = the number of
    rows nothing may die; a mark that looked at lrt > thr alone would kill these patterns in the first piece."""
    monkeypatch.delenv("KGWAS_LMM_PATTERN_TAG_BITS", raising=False)
    monkeypatch.delenv("KGWAS_LMM_TABLE_SELECT", raising=False)
    S, n_rows, P = 64, 1500, 3
    rng = np.random.default_rng(64)
    G = rng.standard_normal((S // 2, 80))
    K_ = np.kron(G @ G.T / 80.0, np.ones((2, 2))) + np.eye(S)
    half = rng.standard_normal((P, S // 2))
    Y = np.stack([half, -half], axis=2).reshape(P, S)            # y[2i] = -y[2i + 1]
    pair_patterns = np.repeat(rng.random((40, S // 2)) < 0.5, 2, axis=1)
    bits = pair_patterns[rng.integers(0, 40, n_rows)]
    tested = Q.tested_of(bits, S)
    assert tested.sum() > 1000
    pick = np.arange(S)
    c = Case(tmp_path, T.table_from_bits(bits, S, pick, 3), S, pick, K_, Y, Q.min_count_of(S))
    try:
        set_piece(monkeypatch, None)
        rows, lrt = c.full()
        zero = (lrt == 0.0).all(axis=0)
        print("%d of %d tested rows have lrt 0.0 in all %d columns; the largest lrt is %g" % (zero.sum(), len(rows), P, lrt.max()))
        pattern = K.patterns_of(bits, tested)
        piece = 256
        later = [i for i in np.flatnonzero(zero) if (pattern[:i][rows[:i] // piece < rows[i] // piece] == pattern[i]).any()]
        assert len(later) > 0, "no row with lrt 0.0 in every column repeats a pattern of an earlier piece"
        set_piece(monkeypatch, piece)
        yard, res = c.yard(P, n_rows, 32), c.skip(P, n_rows, 32)
        assert_same(res, yard, "lrt 0.0 under open heaps")
        assert res["skip"]["rows_skipped"] == 0 and res["skip"]["patterns_dead"] == 0, res["skip"]
        assert res["pairs_shipped"] == P * len(rows)
    finally:
        c.close()


# ---- 4. a tie at the cut -------------------------------------------------------------------------------------------------------
def test_tie_at_the_cut(repeated67, monkeypatch):
    """two copies of a pattern in different pieces, next to each other in a column's ranking: N cuts between them"""
    f, c, lrt = repeated67
    P, piece, chunk = 3, 1024, 32
    rows = f["rows"]
    found = None
    for k in range(P):
        order = np.lexsort((rows, -lrt[k]))
        cuts = [i + 1 for i in range(len(order) - 1)
                if f["pattern"][order[i]] == f["pattern"][order[i + 1]] and rows[order[i]] // piece != rows[order[i + 1]] // piece]
        if len(cuts) >= 10 and found is None:
            cut = cuts[len(cuts) // 2]
            found = (k, cut, order[cut - 1], order[cut])
    assert found is not None, "no cut between two copies in different pieces"
    k, cut, first, second = found
    assert lrt[k, first].tobytes() == lrt[k, second].tobytes() and rows[first] < rows[second], "no tie at the cut"
    for g in (0, 1):
        model = check_against_model(c, f, lrt, monkeypatch, g, P, cut, "N %d geometry %d" % (cut, g), False)
        assert rows[first] in model["kept"][k] and rows[second] not in model["kept"][k]
    res = c.skip(P, cut, K.GEOMETRIES[1][1])
    kept = res["columns"][k]["row"].tolist()
    assert rows[first] in kept and rows[second] not in kept, "the later of two tied rows was kept"


# ---- 5. a full table, colliding tags -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [0, 1])
def test_full_table(repeated67, monkeypatch, g):
    f, c, lrt = repeated67
    distinct = int(f["pattern"].max()) + 1
    assert distinct > 3 * 64
    forced, chunk = K.GEOMETRIES[g]
    set_piece(monkeypatch, forced)
    P, N = 33, 7
    yard, res = c.yard(P, N, chunk), c.skip(P, N, chunk, slots=64)
    assert_same(res, yard, "64 slots")
    u = res["skip"]
    print(u, "distinct", distinct)
    assert u["slots"] == 64 and u["patterns_cached"] <= 64 and u["rows_rejected"] > 0
    assert u["rows_skipped"] <= K.skip_bound(f["pattern"], f["rows"], K.piece_of_geometry(f, g), N)


@pytest.mark.parametrize("g", [0, 1])
def test_colliding_tags(repeated67, monkeypatch, g):
    f, c, lrt = repeated67
    monkeypatch.setenv("KGWAS_LMM_PATTERN_TAG_BITS", "4")
    forced, chunk = K.GEOMETRIES[g]
    set_piece(monkeypatch, forced)
    P, N = 3, 7
    yard = c.yard(P, N, chunk)
    a, b = c.skip(P, N, chunk), c.skip(P, N, chunk)
    for res in (a, b):
        assert_same(res, yard, "4-bit tags")
    u = a["skip"]
    print(u)
    assert u["rows_collided"] > 0 and u["patterns_cached"] <= 15 and u["rows_rejected"] == 0
    assert u["rows_skipped"] <= K.skip_bound(f["pattern"], f["rows"], K.piece_of_geometry(f, g), N)
    assert b["skip"] == u, "the counters of two runs differ"


# ---- 6. one pattern, no duplicate, no tested row -------------------------------------------------------------------------------
def degenerate_case(tmp_path, bits, S, P):
    K_, y = T.kinship_and_phenotype(S)
    pick = np.arange(S)
    return Case(tmp_path, T.table_from_bits(bits, S, pick, 5), S, pick, K_, columns(y, P), 5)


def test_every_tested_row_the_same_pattern(tmp_path, monkeypatch):
    monkeypatch.delenv("KGWAS_LMM_PATTERN_TAG_BITS", raising=False)
    monkeypatch.delenv("KGWAS_LMM_TABLE_SELECT", raising=False)
    S, P, N, piece, chunk = 67, 3, 10, 256, 32
    one = T.bits_with_counts([20], S, 3)[0]
    out = T.bits_with_counts([0, 1, 4, S, S - 1, S - 4], S, 4)
    which = np.random.default_rng(8).integers(0, 8, 1500)  # 6, 7: the tested pattern; 0 .. 5: a row that is not tested
    bits = np.where((which >= 6)[:, None], one[None, :], out[np.minimum(which, 5)])
    tested = T.tested_rule(bits.sum(axis=1), S, 5, Q.MAF)
    assert (tested == (which >= 6)).all() and tested.sum() > 300
    c = degenerate_case(tmp_path, bits, S, P)
    try:
        set_piece(monkeypatch, None)
        rows, lrt = c.full()
        model = K.simulate(np.zeros(len(rows), int), rows, lrt, piece, chunk, N)
        assert model["rows_skipped"] > 0 and model["patterns_dead"] == 1 == model["patterns_cached"]
        set_piece(monkeypatch, piece)
        yard, res = c.yard(P, N, chunk), c.skip(P, N, chunk, slots=64)
        assert_same(res, yard, "one pattern")
        assert {k: res["skip"][k] for k in MODELLED} == {k: model[k] for k in MODELLED}, (res["skip"], model)
        assert all(col["row"].tolist() == rows[:N].tolist() for col in res["columns"]), "the best 10 of rows with one lrt: the first ten"
    finally:
        c.close()


def test_no_duplicate(tmp_path, monkeypatch):
    monkeypatch.delenv("KGWAS_LMM_PATTERN_TAG_BITS", raising=False)
    monkeypatch.delenv("KGWAS_LMM_TABLE_SELECT", raising=False)
    S, P, N = 67, 3, 7
    bits = T.random_bits(Q.ROWS, S, 21)
    tested = T.tested_rule(bits.sum(axis=1), S, 5, Q.MAF)
    n = int(tested.sum())
    assert len(np.unique(np.packbits(bits[tested], axis=1), axis=0)) == n > 1000, "the fixture repeats a tested pattern"
    c = degenerate_case(tmp_path, bits, S, P)
    try:
        set_piece(monkeypatch, 1024)
        # 65536 slots for fewer than 3000 patterns: 16 taken slots in a row do not happen, so nothing is rejected
        yard, res = c.yard(P, N, 64), c.skip(P, N, 64, slots=65536)
        assert_same(res, yard, "no duplicate")
        u = res["skip"]
        print(u)
        assert u["rows_skipped"] == 0 and u["rows_rotated"] == n == u["patterns_cached"] and u["rows_collided"] == 0 == u["rows_rejected"]
        assert 0 < u["patterns_dead"] <= n - N, "patterns die although no row repeats them"
    finally:
        c.close()


def test_no_row_tested(tmp_path, monkeypatch):
    S = 67
    bits = T.bits_with_counts([0, 1, 2, 4, S, S - 4, S - 1] * 40, S, 1)
    c = degenerate_case(tmp_path, bits, S, 3)
    try:
        set_piece(monkeypatch, 64)
        yard, res = c.yard(3, 100, 64), c.skip(3, 100, 64, slots=64)
        assert_same(res, yard, "no tested row")
        assert res["rows_read"] == len(bits) and res["rows_tested"] == 0 and res["pairs_shipped"] == 0
        assert res["skip"] == dict(zip(COUNTERS, (64, 0, 0, 0, 0, 0, 0)))
    finally:
        c.close()


# ---- 7. a handle used again, the refusals --------------------------------------------------------------------------------------
def test_a_second_call_starts_with_an_empty_table(repeated67, monkeypatch):
    f, c, lrt = repeated67
    set_piece(monkeypatch, 1024)
    P, N, chunk = 3, 7, 64
    Y2 = columns(np.random.default_rng(9).permutation(c.Y[0]), P, seed=5)
    yard1, yard2 = c.yard(P, N, chunk), c.yard(P, N, chunk, Y=Y2)
    assert yard1["columns"][0]["row"].tolist() != yard2["columns"][0]["row"].tolist()
    seen = []
    for Y, yard in ((c.Y, yard1), (Y2, yard2), (c.Y, yard1), (Y2, yard2)):
        res = c.skip(P, N, chunk, Y=Y)
        assert_same(res, yard, "another phenotype on one handle")
        assert res["skip"]["rows_skipped"] > 0 and res["skip"]["rows_rejected"] == 0
        seen.append(res["skip"])
    assert seen[0] == seen[2] and seen[1] == seen[3], "two runs give other counters"


def test_refusals(repeated67):
    f, c, lrt = repeated67
    m = c.handle(64)
    Y = np.ascontiguousarray(c.Y[:3])

    def raw(handle, max_patterns, ks, kept):
        return capi.lib.kgwas_lmm_test_table_multi_skip(handle._h, 3, capi.ptr(Y), c.tbl._h, capi.ptr(c.pick), len(c.pick), c.mc, Q.MAF, 10,
                                                        None, None, None, None, None, None, capi.ptr(kept), None, None, None, None, None,
                                                        max_patterns, C.byref(ks))

    before = m.stats()
    ks, kept = capi.LmmSkipStats(*([77] * 7)), np.full(3, 99, np.uint64)
    assert raw(m, 63, ks, kept) == capi.KGWAS_ERR_ARG and b"max_patterns is below 64" in capi.lib.kgwas_last_error()
    assert ks.as_dict() == dict(zip(COUNTERS, [77] * 7)) and kept.tolist() == [99] * 3 and m.stats() == before
    with pytest.raises(kg.KgwasError) as e:
        c.skip(3, 10, 64, slots=0)
    assert e.value.code == capi.KGWAS_ERR_ARG
    assert c.skip(3, 10, 64, slots=127)["skip"]["slots"] == 64  # 127 slots asked for: 64 taken
    W = np.c_[np.ones(f["S"]), np.random.default_rng(2).standard_normal(f["S"])]
    cov = kg.LmmLrt(c.K, chunk_variants=64, covariates=W)
    try:
        before = cov.stats()
        assert raw(cov, 4096, ks, kept) == capi.KGWAS_ERR_ARG
        assert b"covariates are not built for the multi-phenotype passes" in capi.lib.kgwas_last_error()
        assert ks.as_dict() == dict(zip(COUNTERS, [77] * 7)) and kept.tolist() == [99] * 3 and cov.stats() == before
    finally:
        cov.close()
    assert_same(c.skip(3, 10, 64), c.yard(3, 10, 64), "the call after the refusals")


# ---- 8. the tool ---------------------------------------------------------------------------------------------------------------
def test_cli_pattern_skip(repeated67, tmp_path):
    f, c, lrt = repeated67
    P = 5
    ft = 60.0 + 12.0 * (c.Y[:P] - c.Y[0].mean()) / c.Y[0].std()  # values that are no short decimals
    ph = tmp_path / "ph.tsv"
    ph.write_text("accession_id\t" + "\t".join("c%d" % k for k in range(P)) + "\n"
                  + "".join(c.acc[i] + "".join("\t%r" % float(ft[k, i] / 7.0) for k in range(P)) + "\n" for i in range(f["S"])))
    kin = tmp_path / "k.txt"
    kin.write_text("\n".join("\t".join("%.17g" % v for v in r) for r in c.K) + "\n")
    order = [3, 1, 5, 2, 4]
    lst = tmp_path / "cols.txt"
    lst.write_text("".join("%d\tperm%d\n" % (i, i) for i in order))
    common = [os.path.join(BINDIR, "lmm_lrt"), "--kmers_table", c.base, "--kmers_len", str(T.K_LEN), "-p", str(ph), "-lmm", "2", "-k", str(kin),
              "--mac", "5", "-maf", "0.05", "--best", "20", "--chunk_variants", "64", "--pheno_columns", str(lst)]
    env = dict(os.environ, KGWAS_LMM_PIECE_ROWS="1000")
    plain, skip = str(tmp_path / "plain"), str(tmp_path / "skip")
    r0 = subprocess.run(common + ["-outdir", plain], capture_output=True, text=True, timeout=300, env=env)
    r1 = subprocess.run(common + ["-outdir", skip, "--pattern_skip", "1"], capture_output=True, text=True, timeout=300, env=env)
    assert r0.returncode == 0 and r1.returncode == 0, r0.stderr[-1000:] + r1.stderr[-1000:]
    assert sorted(os.listdir(skip)) == sorted(os.listdir(plain)) == sorted("perm%d.%s.txt" % (i, e) for i in order for e in ("assoc", "log"))
    extra = ["pattern_skip_slots", "patterns_cached", "patterns_dead", "rows_skipped", "rows_collided", "rows_rejected", "rows_rotated"]
    for i in order:
        a, b = (open(os.path.join(d, "perm%d.assoc.txt" % i), "rb").read() for d in (plain, skip))
        assert a == b and a.count(b"\n") == 21, "column %d: the .assoc.txt differs with --pattern_skip" % i
        l0, l1 = ([l.split("\t")[0].split(" ")[0] for l in open(os.path.join(d, "perm%d.log.txt" % i)).read().split("\n") if l] for d in (plain, skip))
        assert l1[:len(l0)] == l0 and l1[len(l0):] == extra, l1
        log = dict(l.split("\t", 1) for l in open(os.path.join(skip, "perm%d.log.txt" % i)).read().split("\n") if "\t" in l)
        assert int(log["rows_skipped"]) > 0 and int(log["rows_skipped"]) + int(log["rows_rotated"]) == int(log["rows_tested"]) == len(f["rows"])
        assert int(log["patterns_cached"]) == int(f["pattern"].max()) + 1 and int(log["rows_rejected"]) == 0
        slots = int(log["pattern_skip_slots"])
        assert slots & (slots - 1) == 0 and slots * (16 + 80 // 4) <= 1 << 20 < 2 * slots * (16 + 80 // 4)  # a slot: 16 bytes + the code row
    assert "rows_skipped=%s" % log["rows_skipped"] in r1.stderr and "rows_skipped" not in r0.stderr
