"""lmm_lrt --kmers_table (kgwas_lmm_test_table, lmm_table_kernels.hip): the exact test of every k-mer of a table.

The yardstick of all but the last test is the route the project had before: kgwas_table_to_bed with one batch and no -u, then
kgwas_lmm_test_bed on the written .bed body with the same kinship, y and maf. Doubles are compared by their raw bytes. The piece
of table rows (KGWAS_LMM_PIECE_ROWS) and chunk_variants are varied: no result may depend on either. The last test checks one
table against model E of lmm_lrt_np.py with the tolerance of test_gpu_lmm_lrt.py (1000 x the models' gap, capped at 1e-8); the
fixture's own model gap is asserted <= 1e-10 in test_lmm_lrt_table_cli.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kmersgwas_amd as kg
from kmersgwas_amd import capi
from oracle import oracle_np as onp

import lmm_lrt_np as M
import lmm_table_np as T
from test_lmm_lrt_model import MEASURED_MODEL_GAP

pytestmark = pytest.mark.gpu
LRT_TOL = min(1e-8, 1000 * MEASURED_MODEL_GAP)
BINDIR = os.path.join(os.path.dirname(os.path.abspath(capi.__file__)), "bin")
FIELDS = ("lrt", "lambda", "p", "af")


def write_case(tmp_path, rows, S_f, pick, name="tab"):
    names = ["acc%d" % i for i in range(S_f)]
    base = str(tmp_path / name)
    onp.write_table(base, names, T.K_LEN, rows[:, 0], rows[:, 1:])
    return base, [names[i] for i in pick]


def bed_route(tmp_path, base, rows, pick, acc, K, y, min_count, maf, lmin=1e-5, lmax=1e5, chunk=10240, m=None):
    """The yardstick: (table rows of the tested variants, dict of their lrt, lambda, p, af), in table order. m: an open LmmLrt of K
    to use instead of a new one of chunk_variants = chunk."""
    out = str(tmp_path / "yard")
    tbl = kg.KmersTable(base, T.K_LEN)
    nb, nw = kg.table_to_bed(out, tbl, np.asarray(pick, np.uint64), acc, y.astype(np.float32), min_count, max(len(rows), 1), False)
    tbl.close()
    assert nb == 1
    body = np.frombuffer(open(out + ".0.bed", "rb").read(), np.uint8)[3:]
    bim = [l.split("\t")[1] for l in open(out + ".0.bim").read().split("\n") if l]
    assert len(bim) == nw
    # the table row of every .bim line, by its k-mer (table_from_bits: the k-mer words are ascending and unique)
    words = T.kmer_words(bim)
    bim_rows = np.searchsorted(rows[:, 0], words).astype(np.uint64)
    assert (bim_rows < len(rows)).all() and (rows[bim_rows.astype(np.int64), 0] == words).all(), "a .bim k-mer that is not in the table"
    own = m is None
    if own:
        m = kg.LmmLrt(K, lmin=lmin, lmax=lmax, chunk_variants=chunk)
    try:
        res = m.test(body, y, maf=maf, miss=1.0) if nw else {k: np.zeros(0) for k in FIELDS + ("tested",)}
    finally:
        if own:
            m.close()
    t = np.asarray(res["tested"], bool)
    return bim_rows[t], {k: res[k][t] for k in FIELDS}


def table_route(base, pick, K, y, min_count, maf, best_n, chunk, lmin=1e-5, lmax=1e5, m=None):
    """m: an open LmmLrt of K to use instead of a new one of chunk_variants = chunk; res["stats"] then counts this call alone too."""
    tbl = kg.KmersTable(base, T.K_LEN)
    own = m is None
    if own:
        m = kg.LmmLrt(K, lmin=lmin, lmax=lmax, chunk_variants=chunk)
    try:
        before = m.stats()
        res = m.test_table(tbl, np.asarray(pick, np.uint64), y, min_count, maf, best_n)
        after = m.stats()
        res["stats"] = {k: after[k] - before[k] for k in ("variants_read", "variants_tested", "chunks")}
    finally:
        if own:
            m.close()
        tbl.close()
    return res


def assert_same(res, rows_exp, exp, what):
    assert res["row"].tolist() == rows_exp.tolist(), what + ": other rows"
    for k in FIELDS:
        assert res[k].tobytes() == exp[k].tobytes(), "%s: %s differs in its bits" % (what, k)


# ---- 1. equality with the .bed route -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,S_f", [(5, 5), (64, 64), (65, 65), (67, 67), (241, 241), (67, 70), (241, 300)])
def test_equals_the_bed_route(tmp_path, monkeypatch, S, S_f):
    n_rows = 3000
    K, y = T.kinship_and_phenotype(S)
    pick = np.random.default_rng(S_f).permutation(S_f)[:S]
    bits = T.random_bits(n_rows, S, S_f)
    rows = T.table_from_bits(bits, S_f, pick, S)
    base, acc = write_case(tmp_path, rows, S_f, pick)
    mc, maf = (1, 0.05) if S == 5 else (kg.min_count(S, 0.05, 5), 0.05)
    rows_exp, exp = bed_route(tmp_path, base, rows, pick, acc, K, y, mc, maf)
    n1 = bits.sum(axis=1)
    rule = T.tested_rule(n1, S, mc, maf)
    print("S=%d S_f=%d: %d of %d rows tested; the MAC rule alone keeps %d, the af rule alone %d"
          % (S, S_f, len(rows_exp), n_rows, ((n1 >= mc) & (n1 <= S - mc)).sum(), T.tested_rule(n1, S, 0, maf).sum()))
    assert 0 < len(rows_exp) < n_rows and rows_exp.tolist() == np.flatnonzero(rule).tolist()
    for piece, chunk in ((None, 10240), (1024, 32), (1000, 64)):
        if piece is None:
            monkeypatch.delenv("KGWAS_LMM_PIECE_ROWS", raising=False)
        else:
            monkeypatch.setenv("KGWAS_LMM_PIECE_ROWS", str(piece))
        res = table_route(base, pick, K, y, mc, maf, n_rows, chunk)
        assert_same(res, rows_exp, exp, "piece %s chunk %d" % (piece, chunk))
        assert (res["kmer"] == rows[rows_exp.astype(np.int64), 0]).all()
        assert res["rows_read"] == n_rows and res["rows_tested"] == len(rows_exp)
        assert res["stats"]["variants_read"] == n_rows and res["stats"]["variants_tested"] == len(rows_exp)


# ---- 2. the edges of the tested set --------------------------------------------------------------------------------------------
def edges_case(tmp_path, S, maf, mac, chunk=64):
    """Presence counts at and beside every edge of both rules, and every count 0 .. S: the table route against the .bed route and
    the numpy rule. Returns (counts, rule)."""
    mc = kg.min_count(S, maf, mac)
    counts = [0, S, 1, S - 1, mc - 1, mc, mc + 1, S - mc - 1, S - mc, S - mc + 1] * 3 + list(range(0, S + 1))
    bits = T.bits_with_counts(counts, S, S)
    K, y = T.kinship_and_phenotype(S)
    pick = np.random.default_rng(S).permutation(S)
    rows = T.table_from_bits(bits, S, pick, 9)
    d = tmp_path / ("S%d_%g" % (S, maf))
    d.mkdir()
    base, acc = write_case(d, rows, S, pick)
    rows_exp, exp = bed_route(d, base, rows, pick, acc, K, y, mc, maf)
    rule = T.tested_rule(counts, S, mc, maf)
    assert rows_exp.tolist() == np.flatnonzero(rule).tolist()
    res = table_route(base, pick, K, y, mc, maf, len(counts), chunk)
    assert_same(res, rows_exp, exp, "S=%d maf=%g" % (S, maf))
    return np.asarray(counts), rule


def test_tested_set_edges(tmp_path, monkeypatch):
    monkeypatch.setenv("KGWAS_LMM_PIECE_ROWS", "64")
    # S = 50, maf = 0.1: ceil(S maf) = 5 carriers pass the MAC rule, but 1 - af = 1 - 0.9 = 0.09999999999999998 < 0.1 at n1 = 5
    # (while af = 0.1 passes at n1 = 45): the two rules disagree by one count at one end
    for S, maf, mac in ((50, 0.1, 1), (67, 0.05, 5), (67, 0.0, 7)):
        counts, rule = edges_case(tmp_path, S, maf, mac)
        if S == 50:
            mc = kg.min_count(S, maf, mac)
            mac_only = (counts >= mc) & (counts <= S - mc)
            assert (mac_only & ~rule).any() and set(counts[mac_only & ~rule]) == {5}, "the fixture's rules do not disagree"


def test_no_row_tested(tmp_path):
    S = 67
    K, y = T.kinship_and_phenotype(S)
    pick = np.arange(S)
    rows = T.table_from_bits(T.bits_with_counts([0, 1, 2, 4, S, S - 4, S - 1] * 40, S, 1), S, pick, 2)
    base, acc = write_case(tmp_path, rows, S, pick)
    rows_exp, _ = bed_route(tmp_path, base, rows, pick, acc, K, y, 5, 0.05)
    assert len(rows_exp) == 0
    res = table_route(base, pick, K, y, 5, 0.05, 100, 64)
    assert len(res["row"]) == 0 and res["rows_read"] == len(rows) and res["rows_tested"] == 0


def test_argument_errors(tmp_path):
    S = 67
    K, y = T.kinship_and_phenotype(S)
    pick = np.arange(S)
    rows = T.table_from_bits(T.random_bits(50, S, 1), S, pick, 2)
    base, _ = write_case(tmp_path, rows, S, pick)
    tbl = kg.KmersTable(base, T.K_LEN)
    m = kg.LmmLrt(K, chunk_variants=64)
    for col, yy, best in ((pick, y, 0), (pick[:-1], y, 10), (np.r_[pick[:-1], S], y, 10)):
        with pytest.raises(kg.KgwasError) as e:
            m.test_table(tbl, np.asarray(col, np.uint64), yy, 5, 0.05, best)
        assert e.value.code == capi.KGWAS_ERR_ARG, e.value
    assert capi.lib.kgwas_lmm_test_table(None, capi.ptr(y), tbl._h, capi.ptr(pick.astype(np.uint64)), S, 5, 0.05, 10, *([None] * 9)) == capi.KGWAS_ERR_ARG
    assert len(m.test_table(tbl, pick.astype(np.uint64), y, 5, 0.05, 10)["row"]) == 10  # the handle is still good
    m.close()
    tbl.close()


# ---- 3. selection --------------------------------------------------------------------------------------------------------------
def test_selection_and_ties(tmp_path, monkeypatch):
    S, S_f, n_rows = 67, 70, 900
    K, y = T.kinship_and_phenotype(S)
    pick = np.random.default_rng(3).permutation(S_f)[:S]
    bits = T.random_bits(n_rows, S, 31, 0.1, 0.9)
    # duplicated patterns: identical bits give identical lrt bits. Copies of rows 10..59 go to rows 600.., far enough for another piece.
    bits[600:650] = bits[10:60]
    rows = T.table_from_bits(bits, S_f, pick, 31)
    base, acc = write_case(tmp_path, rows, S_f, pick)
    mc, maf = 5, 0.05
    rows_all, all_ = bed_route(tmp_path, base, rows, pick, acc, K, y, mc, maf)
    order = np.lexsort((rows_all, -all_["lrt"]))  # by lrt descending, then the table row: a stable order on (-lrt, row)
    ranked = rows_all[order]
    # a pair of duplicates next to each other in the ranking; N = the place of the first one cuts between them
    pairs = [i for i in range(len(ranked) - 1) if ranked[i + 1] == ranked[i] + 590]
    assert len(pairs) >= 10, "the duplicated patterns are not tested"
    for i in pairs:
        assert all_["lrt"][order[i]].tobytes() == all_["lrt"][order[i + 1]].tobytes(), "identical patterns, other lrt bits"
    cut = pairs[len(pairs) // 2] + 1
    for best in (1, 100, cut, len(rows_all) - 1):
        keep = np.sort(order[:best])
        got = []
        for piece, chunk in ((256, 32), (333, 64), (None, 10240)):
            if piece is None:
                monkeypatch.delenv("KGWAS_LMM_PIECE_ROWS", raising=False)
            else:
                monkeypatch.setenv("KGWAS_LMM_PIECE_ROWS", str(piece))
            res = table_route(base, pick, K, y, mc, maf, best, chunk)
            assert_same(res, rows_all[keep], {k: all_[k][keep] for k in FIELDS}, "best %d piece %s chunk %d" % (best, piece, chunk))
            assert res["rows_tested"] == len(rows_all)
            got.append(res["row"].tobytes())
        assert len(set(got)) == 1
    # at the cut the earlier of the two identical rows is kept, the later one is not
    res = table_route(base, pick, K, y, mc, maf, cut, 64)
    assert ranked[cut - 1] in res["row"] and ranked[cut] not in res["row"]


# ---- 4. the tool ---------------------------------------------------------------------------------------------------------------
def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def _log(path):
    return dict(l.split("\t", 1) for l in open(path).read().split("\n") if "\t" in l)


def test_cli_against_the_two_tools(tmp_path):
    S, S_f, n_rows = 67, 70, 700
    K, y = T.kinship_and_phenotype(S)
    pick = np.random.default_rng(4).permutation(S_f)[:S]
    rows = T.table_from_bits(T.random_bits(n_rows, S, 41), S_f, pick, 41)
    base, acc = write_case(tmp_path, rows, S_f, pick)
    # flowering-time-like values that are no short decimals (means of replicates), and a second column
    ft = 60.0 + 12.0 * (y - y.mean()) / y.std()
    v1 = ["%.10f" % (round(v * 3) / 3) for v in ft]
    v2 = ["%r" % float(v) for v in np.random.default_rng(6).permutation(ft) / 7.0]
    ph2 = tmp_path / "two.tsv"
    ph2.write_text("accession_id\tFT10\tFT16\n" + "".join("%s\t%s\t%s\n" % t for t in zip(acc, v1, v2)))
    only2 = tmp_path / "second.tsv"
    only2.write_text("accession_id\tFT16\n" + "".join("%s\t%s\n" % t for t in zip(acc, v2)))
    kin = tmp_path / "pheno.kinship"
    kin.write_text("\n".join("\t".join("%.17g" % v for v in r) for r in K) + "\n")
    lmm, t2b, out = os.path.join(BINDIR, "lmm_lrt"), os.path.join(BINDIR, "kmers_table_to_bed"), str(tmp_path / "out")
    for ph, n_opt, tag in ((ph2, [], "c1"), (only2, ["-n", "2"], "c2")):
        plink = str(tmp_path / ("plink_" + tag))
        _run([t2b, "-t", base, "-k", str(T.K_LEN), "-p", str(ph), "--maf", "0.05", "--mac", "5", "-b", "100000", "-o", plink])
        _run([lmm, "-bfile", plink + ".0", "-lmm", "2", "-k", str(kin), "-outdir", out, "-o", "bed_" + tag, "-maf", "0.05"])
        bed_lines = open(os.path.join(out, "bed_%s.assoc.txt" % tag)).read().split("\n")
        assert len(bed_lines) > 100
        _run([lmm, "--kmers_table", base, "--kmers_len", str(T.K_LEN), "-p", str(ph2), "-lmm", "2", "-k", str(kin), "-outdir", out,
              "-o", "all_" + tag, "--mac", "5", "-maf", "0.05"] + n_opt)
        assert open(os.path.join(out, "all_%s.assoc.txt" % tag)).read().split("\n") == bed_lines, "the whole file differs (%s)" % tag
        # the best 50: ranked with the library on the files the first tool wrote
        yy, keep, cnt = np.zeros(S), np.zeros(S, np.uint8), C.c_uint64()
        capi.check(capi.lib.kgwas_lmm_read_fam((plink + ".0.fam").encode(), 1, S, capi.ptr(yy), capi.ptr(keep), C.byref(cnt)))
        assert keep.all()
        m = kg.LmmLrt(K, chunk_variants=64)
        res = m.test(np.frombuffer(open(plink + ".0.bed", "rb").read(), np.uint8)[3:], yy, maf=0.05, miss=0.05)
        m.close()
        tested = np.flatnonzero(res["tested"])
        assert len(tested) == len(bed_lines) - 2
        top = np.sort(np.lexsort((tested, -res["lrt"][tested]))[:50])
        _run([lmm, "--kmers_table", base, "--kmers_len", str(T.K_LEN), "-p", str(ph2), "-lmm", "2", "-k", str(kin), "-outdir", out,
              "-o", "top_" + tag, "--mac", "5", "-maf", "0.05", "--best", "50", "--chunk_variants", "32"] + n_opt)
        top_lines = open(os.path.join(out, "top_%s.assoc.txt" % tag)).read().split("\n")
        assert top_lines == [bed_lines[0]] + [bed_lines[1 + i] for i in top] + [""], "the best 50 differ (%s)" % tag
        lb, lt = _log(os.path.join(out, "bed_%s.log.txt" % tag)), _log(os.path.join(out, "top_%s.log.txt" % tag))
        assert lt["rows_read"] == str(n_rows) and lt["rows_tested"] == lb["variants_tested"] and lt["rows_kept"] == "50" and lt["best_n"] == "50"
        assert lt["lambda0"] == lb["lambda0"] and lt["logl_H0"] == lb["logl_H0"] and lt["individuals_used"] == "67"


def test_cli_no_row_tested(tmp_path):
    S = 67
    K, y = T.kinship_and_phenotype(S)
    pick = np.arange(S)
    rows = T.table_from_bits(T.bits_with_counts([0, 1, 2, S, S - 1] * 20, S, 1), S, pick, 2)
    base, acc = write_case(tmp_path, rows, S, pick)
    ph = tmp_path / "ph.tsv"
    ph.write_text("accession_id\tv\n" + "".join("%s\t%r\n" % (a, float(v)) for a, v in zip(acc, y)))
    kin = tmp_path / "k.txt"
    kin.write_text("\n".join("\t".join("%.17g" % v for v in r) for r in K) + "\n")
    out = str(tmp_path / "out")
    _run([os.path.join(BINDIR, "lmm_lrt"), "--kmers_table", base, "--kmers_len", str(T.K_LEN), "-p", str(ph), "-lmm", "2", "-k", str(kin),
          "-outdir", out, "-o", "none"])
    assert open(os.path.join(out, "none.assoc.txt")).read() == "chr\trs\tps\tn_miss\tallele1\tallele0\taf\tl_mle\tp_lrt\n"
    assert _log(os.path.join(out, "none.log.txt"))["rows_kept"] == "0"


# ---- 5. against model E, without the .bed route ---------------------------------------------------------------------------------
def test_against_model_E(tmp_path):
    K, y, bits, pick, rows = T.model_fixture()
    base, _ = write_case(tmp_path, rows, T.MODEL_S_F, pick)
    res = table_route(base, pick, K, y, T.MODEL_MIN_COUNT, T.MODEL_MAF, T.MODEL_ROWS, 64, M.LMIN, M.LMAX)
    assert res["row"].tolist() == list(range(T.MODEL_ROWS))
    ref, _ = M.lrt_E(K, y, T.model_dosages(bits))
    err = np.abs(res["lrt"] - ref).max()
    print("table route, S=67: max |LRT - model E| = %.3e (allowed %.1e), LRT range %.3g..%.3g" % (err, LRT_TOL, ref.min(), ref.max()))
    assert err <= LRT_TOL
    np.testing.assert_array_equal(res["af"], T.model_dosages(bits).mean(axis=1) / 2)
