"""lmm_lrt --kmers_table --pheno_columns (kgwas_lmm_test_table_multi, lmm_table_select_kernel): the phenotype and its permutations
over one k-mers table in one pass, the best N per column.

The yardstick is the route the project had before: one LmmLrt.test_table call per column. Doubles are compared by their raw
bytes, rows as lists. The piece of table rows (KGWAS_LMM_PIECE_ROWS), chunk_variants, the number of columns (around LMM_PBLOCK =
32) and N are varied: no result may depend on the first two, and none on whether the device's selection runs
(KGWAS_LMM_TABLE_SELECT=0 ships every pair)."""
import os
import subprocess

import numpy as np
import pytest

import kmersgwas_amd as kg
from kmersgwas_amd import capi

import lmm_table_np as T
from test_gpu_lmm_lrt_table import write_case

pytestmark = pytest.mark.gpu
BINDIR = os.path.join(os.path.dirname(os.path.abspath(capi.__file__)), "bin")
FIELDS = ("lrt", "lambda", "p", "af")
CONFIGS = ((None, 10240), (1024, 32), (1000, 64))  # (KGWAS_LMM_PIECE_ROWS, chunk_variants)


def columns(y, P, seed=11):
    """y and P - 1 seeded permutations of it"""
    rng = np.random.default_rng(seed)
    return np.stack([y] + [rng.permutation(y) for _ in range(P - 1)])


def set_piece(monkeypatch, piece):
    if piece is None:
        monkeypatch.delenv("KGWAS_LMM_PIECE_ROWS", raising=False)
    else:
        monkeypatch.setenv("KGWAS_LMM_PIECE_ROWS", str(piece))


def same_column(got, exp, what):
    assert got["row"].tolist() == exp["row"].tolist(), what + ": other rows"
    assert got["kmer"].tolist() == exp["kmer"].tolist(), what + ": other k-mers"
    for k in FIELDS:
        assert got[k].tobytes() == exp[k].tobytes(), "%s: %s differs in its bits" % (what, k)


class Case:
    """A table on disk, open, with one handle per chunk_variants; the yardstick of a (column, N) is computed once."""

    def __init__(self, tmp_path, rows, S_f, pick, K, Y, mc, maf):
        self.base, _ = write_case(tmp_path, rows, S_f, pick)
        self.rows, self.pick, self.K, self.Y, self.mc, self.maf = rows, np.asarray(pick, np.uint64), K, Y, mc, maf
        self.tbl = kg.KmersTable(self.base, T.K_LEN)
        self.handles, self.yard = {}, {}

    def handle(self, chunk):
        if chunk not in self.handles:
            self.handles[chunk] = kg.LmmLrt(self.K, chunk_variants=chunk)
        return self.handles[chunk]

    def single(self, k, best_n):
        if (k, best_n) not in self.yard:
            self.yard[k, best_n] = self.handle(10240).test_table(self.tbl, self.pick, self.Y[k], self.mc, self.maf, best_n)
        return self.yard[k, best_n]

    def multi(self, cols, best_n, chunk):
        return self.handle(chunk).test_table_multi(self.tbl, self.pick, self.Y[list(cols)], self.mc, self.maf, best_n)

    def close(self):
        for m in self.handles.values():
            m.close()
        self.tbl.close()


def make_case(tmp_path, S, S_f, n_rows, P, bits=None, seed=None):
    K, y = T.kinship_and_phenotype(S)
    pick = np.random.default_rng(S_f).permutation(S_f)[:S] if S_f != S else np.arange(S)
    if bits is None:
        bits = T.random_bits(n_rows, S, S_f if seed is None else seed)
    rows = T.table_from_bits(bits, S_f, pick, S)
    mc, maf = (1, 0.05) if S == 5 else (kg.min_count(S, 0.05, 5), 0.05)
    return Case(tmp_path, rows, S_f, pick, K, columns(y, P), mc, maf)


# ---- 1. equality with one test_table call per column; 7. the stats -------------------------------------------------------------
@pytest.mark.parametrize("S,S_f", [(5, 5), (67, 67), (241, 241), (67, 70)])
def test_equals_single_calls(tmp_path, monkeypatch, S, S_f):
    n_rows = 1200
    c = make_case(tmp_path, S, S_f, n_rows, 33)
    try:
        tested = c.single(0, n_rows)["rows_tested"]
        assert 0 < tested < n_rows
        nulls = [c.handle(10240).null(c.Y[k]) for k in range(33)]
        for piece, chunk in CONFIGS:
            set_piece(monkeypatch, piece)
            for P in (1, 3, 32, 33):
                for best_n in (1, 7, 100, n_rows):
                    what = "piece %s chunk %d P %d N %d" % (piece, chunk, P, best_n)
                    before = c.handle(chunk).stats()
                    res = c.multi(range(P), best_n, chunk)
                    after = c.handle(chunk).stats()
                    assert len(res["columns"]) == P
                    for k in range(P):
                        same_column(res["columns"][k], c.single(k, best_n), "%s column %d" % (what, k))
                        assert len(res["columns"][k]["row"]) == min(best_n, tested)
                    assert res["logl0"].tobytes() == np.array([n[0] for n in nulls[:P]]).tobytes(), what + ": logl0"
                    assert res["lambda0"].tobytes() == np.array([n[1] for n in nulls[:P]]).tobytes(), what + ": lambda0"
                    assert res["rows_read"] == n_rows and res["rows_tested"] == tested
                    assert P * min(best_n, tested) <= res["pairs_shipped"] <= tested * P
                    if best_n == n_rows:
                        assert res["pairs_shipped"] == tested * P, what + ": a pair was dropped although no heap was full"
                    assert after["variants_read"] - before["variants_read"] == n_rows, what
                    assert after["variants_tested"] - before["variants_tested"] == tested * P, what
    finally:
        c.close()


# ---- 2. the order of the columns -----------------------------------------------------------------------------------------------
def test_column_order_and_repeats(tmp_path, monkeypatch):
    set_piece(monkeypatch, 256)
    c = make_case(tmp_path, 67, 70, 900, 5)
    try:
        order = [3, 0, 3, 4, 1, 0, 2] + [1] * 30  # 37 columns: the repeats cross a block of 32
        res = c.multi(order, 20, 64)
        for j, k in enumerate(order):
            same_column(res["columns"][j], c.single(k, 20), "place %d, column %d" % (j, k))
        nulls = [c.handle(10240).null(c.Y[k]) for k in range(5)]
        assert res["logl0"].tolist() == [nulls[k][0] for k in order] and res["lambda0"].tolist() == [nulls[k][1] for k in order]
    finally:
        c.close()


# ---- 3. the filter works and is harmless ---------------------------------------------------------------------------------------
def test_the_filter_works_and_is_harmless(tmp_path, monkeypatch):
    set_piece(monkeypatch, 1024)
    P, best_n = 33, 7
    c = make_case(tmp_path, 67, 70, 1200, P)
    try:
        monkeypatch.delenv("KGWAS_LMM_TABLE_SELECT", raising=False)
        on = c.multi(range(P), best_n, 32)
        monkeypatch.setenv("KGWAS_LMM_TABLE_SELECT", "0")
        off = c.multi(range(P), best_n, 32)
        monkeypatch.setenv("KGWAS_LMM_TABLE_SELECT", "1")
        on1 = c.multi(range(P), best_n, 32)
        tested = on["rows_tested"]
        print("tested %d rows x %d columns: %d pairs shipped with the selection (%.2f %%), %d without"
              % (tested, P, on["pairs_shipped"], 100.0 * on["pairs_shipped"] / (tested * P), off["pairs_shipped"]))
        assert tested > 32 * best_n and off["rows_tested"] == tested
        assert best_n * P <= on["pairs_shipped"] < tested * P
        assert off["pairs_shipped"] == tested * P
        assert on1["pairs_shipped"] == on["pairs_shipped"]
        for k in range(P):
            same_column(on["columns"][k], off["columns"][k], "column %d with and without the selection" % k)
            same_column(on["columns"][k], c.single(k, best_n), "column %d" % k)
    finally:
        c.close()


# ---- 4. ties at the cut --------------------------------------------------------------------------------------------------------
def test_ties_at_the_cut(tmp_path, monkeypatch):
    S, S_f, n_rows, P, piece, chunk = 67, 70, 900, 3, 256, 32
    bits = T.random_bits(n_rows, S, 31, 0.1, 0.9)
    bits[600:650] = bits[10:60]  # identical patterns give identical lrt bits; the copies lie two pieces further on
    c = make_case(tmp_path, S, S_f, n_rows, P, bits=bits)
    try:
        set_piece(monkeypatch, piece)
        # from the yardstick: a column whose N-th and (N+1)-th results are the two copies of one pattern
        found = None
        for k in range(P):
            full = c.single(k, n_rows)
            order = np.lexsort((full["row"], -full["lrt"]))  # by lrt descending, then the table row
            ranked = full["row"][order].astype(np.int64)
            pairs = [i for i in range(len(ranked) - 1) if ranked[i + 1] == ranked[i] + 590]
            if len(pairs) >= 3 and found is None:
                i = pairs[len(pairs) // 2]
                found = (k, i + 1, int(ranked[i]), int(ranked[i + 1]), full["lrt"][order[i]], full["lrt"][order[i + 1]])
        assert found is not None, "no column ranks the two copies of a pattern next to each other"
        k, cut, first, second, lrt_a, lrt_b = found
        assert lrt_a.tobytes() == lrt_b.tobytes() and second == first + 590, "no tie at the cut"
        assert first // piece != second // piece, "the tied rows lie in one piece (and so, possibly, in one sub-chunk)"
        for pc, ch in ((piece, chunk), (333, 64), (None, 10240)):
            set_piece(monkeypatch, pc)
            res = c.multi(range(P), cut, ch)
            for j in range(P):
                same_column(res["columns"][j], c.single(j, cut), "N %d piece %s chunk %d column %d" % (cut, pc, ch, j))
            kept = res["columns"][k]["row"].tolist()
            assert first in kept and second not in kept, "the later of two tied rows was kept"
    finally:
        c.close()


# ---- 5. no tested row; argument errors -----------------------------------------------------------------------------------------
def test_no_row_tested(tmp_path):
    S = 67
    bits = T.bits_with_counts([0, 1, 2, 4, S, S - 4, S - 1] * 40, S, 1)
    c = make_case(tmp_path, S, S, len(bits), 3, bits=bits)
    try:
        assert c.single(0, 100)["rows_tested"] == 0
        before = c.handle(64).stats()
        res = c.multi(range(3), 100, 64)
        after = c.handle(64).stats()
        assert len(res["columns"]) == 3 and all(len(col[f]) == 0 for col in res["columns"] for f in ("row", "kmer") + FIELDS)
        assert res["rows_read"] == len(bits) and res["rows_tested"] == 0 and res["pairs_shipped"] == 0
        assert after["variants_read"] - before["variants_read"] == len(bits) and after["variants_tested"] == before["variants_tested"]
        assert np.isfinite(res["logl0"]).all() and res["logl0"].tolist() == [c.handle(64).null(c.Y[k])[0] for k in range(3)]
    finally:
        c.close()


def test_argument_errors(tmp_path):
    c = make_case(tmp_path, 67, 67, 50, 3)
    try:
        m, Y, S = c.handle(64), c.Y, 67
        bad_value, constant = Y.copy(), Y.copy()
        bad_value[2, 5] = np.inf
        constant[1, :] = 3.0
        for cols, YY, best, msg in ((c.pick, Y, 0, "best_n is 0"), (c.pick[:-1], Y, 10, "n_acc"), (np.r_[c.pick[:-1], S], Y, 10, "out of range"),
                                    (c.pick, bad_value, 10, "(column 2)"), (c.pick, constant, 10, "(column 1)"),
                                    (c.pick, Y[:0], 10, "n_pheno is 0")):
            with pytest.raises(kg.KgwasError) as e:
                m.test_table_multi(c.tbl, np.asarray(cols, np.uint64), YY, c.mc, c.maf, best)
            assert e.value.code == capi.KGWAS_ERR_ARG and msg in str(e.value), e.value
        res = m.test_table_multi(c.tbl, c.pick, Y, c.mc, c.maf, 10)  # the handle is still good
        for k in range(3):
            same_column(res["columns"][k], c.single(k, 10), "after the refusals, column %d" % k)
    finally:
        c.close()


# ---- 6. the tool ---------------------------------------------------------------------------------------------------------------
def test_cli_against_one_run_per_column(tmp_path):
    S, S_f, n_rows, P = 67, 70, 700, 5
    K, y = T.kinship_and_phenotype(S)
    pick = np.random.default_rng(4).permutation(S_f)[:S]
    rows = T.table_from_bits(T.random_bits(n_rows, S, 41), S_f, pick, 41)
    base, acc = write_case(tmp_path, rows, S_f, pick)
    ft = 60.0 + 12.0 * (y - y.mean()) / y.std()  # values that are no short decimals
    Y = columns(ft / 7.0, P)
    ph = tmp_path / "ph.tsv"
    ph.write_text("accession_id\t" + "\t".join("c%d" % k for k in range(P)) + "\n"
                  + "".join(acc[i] + "".join("\t%r" % float(Y[k, i]) for k in range(P)) + "\n" for i in range(S)))
    kin = tmp_path / "ph.kinship"
    kin.write_text("\n".join("\t".join("%.17g" % v for v in r) for r in K) + "\n")
    order = [3, 1, 5, 2, 4]
    lst = tmp_path / "cols.txt"
    lst.write_text("".join("%d\tperm%d\n" % (i, i) for i in order))
    common = [os.path.join(BINDIR, "lmm_lrt"), "--kmers_table", base, "--kmers_len", str(T.K_LEN), "-p", str(ph), "-lmm", "2", "-k", str(kin),
              "--mac", "5", "-maf", "0.05", "--best", "50", "--chunk_variants", "32"]

    def tool(args):
        r = subprocess.run(common + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]

    multi, single = str(tmp_path / "multi"), str(tmp_path / "single")
    tool(["-outdir", multi, "--pheno_columns", str(lst)])
    assert sorted(os.listdir(multi)) == sorted("perm%d.%s.txt" % (i, e) for i in order for e in ("assoc", "log"))
    for i in order:
        tool(["-outdir", single, "-n", str(i), "-o", "perm%d" % i])
        got = open(os.path.join(multi, "perm%d.assoc.txt" % i), "rb").read()
        assert got == open(os.path.join(single, "perm%d.assoc.txt" % i), "rb").read(), "column %d: other bytes" % i
        assert got.count(b"\n") == 51
        lm, ls = (open(os.path.join(d, "perm%d.log.txt" % i)).read().split("\n") for d in (multi, single))
        assert len(lm) == len(ls) and sum(l.startswith("ms: ") for l in lm) == 1
        assert [l for l in lm if not l.startswith("ms: ")] == [l for l in ls if not l.startswith("ms: ")], "column %d: other log" % i
