"""lmm_lrt --pattern_cache (kgwas_lmm_test_table_unique, the lmm_pattern_* and lmm_cache_* kernels of lmm_table_kernels.hip): each distinct tested
pattern of a k-mers table goes through rotate, grid and refine once, every other row with it takes the stored result.

The yardstick everywhere is kgwas_lmm_test_table on the same handle and table: row, kmer, lrt, lambda, p and af are compared by
their raw bytes, rows_read and rows_tested as numbers. There is no tolerance. The fixtures come from lmm_unique_np.py, which first
asserts in numpy what they are for. The cache's counters are checked against numpy's count of the distinct tested patterns
wherever nothing is rejected and no tag collides."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kmersgwas_amd as kg
from kmersgwas_amd import capi
from oracle import oracle_np as onp

import lmm_table_np as T
import lmm_unique_np as Q

pytestmark = pytest.mark.gpu
BINDIR = os.path.join(os.path.dirname(os.path.abspath(capi.__file__)), "bin")
FIELDS = ("row", "kmer", "lrt", "lambda", "p", "af")
COUNTERS = ("slots", "patterns_cached", "rows_from_cache", "rows_collided", "rows_rejected", "rows_rotated")


def write_case(tmp_path, rows, S_f, pick, name="tab"):
    names = ["acc%d" % i for i in range(S_f)]
    base = str(tmp_path / name)
    onp.write_table(base, names, T.K_LEN, rows[:, 0], rows[:, 1:])
    return base, [names[i] for i in pick]


def set_piece(monkeypatch, piece):
    if piece is None:
        monkeypatch.delenv("KGWAS_LMM_PIECE_ROWS", raising=False)
    else:
        monkeypatch.setenv("KGWAS_LMM_PIECE_ROWS", str(piece))


def assert_same(res, yard, what):
    for k in FIELDS:
        assert res[k].tobytes() == yard[k].tobytes(), "%s: %s differs from kgwas_lmm_test_table's in its bytes" % (what, k)
    assert res["rows_read"] == yard["rows_read"] and res["rows_tested"] == yard["rows_tested"], what


def assert_identities(res, what):
    u = res["unique"]
    assert res["rows_tested"] == u["patterns_cached"] + u["rows_from_cache"] + u["rows_collided"] + u["rows_rejected"], (what, u)
    assert u["rows_rotated"] == res["rows_tested"] - u["rows_from_cache"], (what, u)


def both(m, tbl, pick, y, mc, best_n, max_patterns, what, runs=1):
    """the yardstick and `runs` calls with the cache on the same handle and table; bytes equal, identities hold, counters repeat"""
    col = np.asarray(pick, np.uint64)
    yard = m.test_table(tbl, col, y, mc, Q.MAF, best_n)
    out = [m.test_table(tbl, col, y, mc, Q.MAF, best_n, max_patterns=max_patterns) for _ in range(runs)]
    for res in out:
        assert_same(res, yard, what)
        assert_identities(res, what)
    return yard, out


def panel_case(tmp_path, monkeypatch, S, S_f, geometries):
    bits = Q.repeated_bits(S)
    tested = Q.tested_of(bits, S)
    pick = Q.pick_of(S, S_f)
    rows = T.table_from_bits(bits, S_f, pick, S)
    distinct = Q.assert_fixture(bits, tested, rows.shape[1], sub_chunks=S != 5)
    K, y = T.kinship_and_phenotype(S)
    base, _ = write_case(tmp_path, rows, S_f, pick)
    mc = Q.min_count_of(S)
    assert mc == (1 if S == 5 else kg.min_count(S, Q.MAF, 5))
    for piece, chunk in geometries:
        set_piece(monkeypatch, piece)
        what = "S=%d S_f=%d piece %s chunk %d" % (S, S_f, piece, chunk)
        tbl, m = kg.KmersTable(base, T.K_LEN), kg.LmmLrt(K, chunk_variants=chunk)
        try:
            before = m.stats()
            yard, (a, b) = both(m, tbl, pick, y, mc, Q.ROWS, 4096, what, runs=2)
            after = m.stats()
        finally:
            m.close()
            tbl.close()
        assert yard["rows_tested"] == int(tested.sum()) and len(yard["row"]) == yard["rows_tested"]
        u = a["unique"]
        print(what, u)
        assert u["slots"] == 4096 and u["rows_rejected"] == 0 and u["rows_collided"] == 0, (what, u)
        assert u["patterns_cached"] == distinct == u["rows_rotated"], (what, u, distinct)
        assert b["unique"] == u, "%s: the counters of two runs differ" % what
        assert after["variants_tested"] - before["variants_tested"] == 3 * yard["rows_tested"], "variants_tested counts tested rows"


# ---- 1. panels and chunking ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,S_f", Q.PANELS)
def test_equals_test_table(tmp_path, monkeypatch, S, S_f):
    monkeypatch.delenv("KGWAS_LMM_PATTERN_TAG_BITS", raising=False)
    panel_case(tmp_path, monkeypatch, S, S_f, Q.GEOMETRIES)


def test_code_rows_wider_than_a_wave(tmp_path, monkeypatch):
    """1135 accessions: a code row of 71 dwords, so the hash and the compare take a second round of lanes"""
    monkeypatch.delenv("KGWAS_LMM_PATTERN_TAG_BITS", raising=False)
    panel_case(tmp_path, monkeypatch, *Q.WIDE, Q.GEOMETRIES[:1])


# ---- 2. a full cache, colliding tags -------------------------------------------------------------------------------------------
@pytest.fixture
def repeated67(tmp_path):
    S, S_f = 67, 70
    bits = Q.repeated_bits(S)
    tested = Q.tested_of(bits, S)
    pick = Q.pick_of(S, S_f)
    rows = T.table_from_bits(bits, S_f, pick, S)
    distinct = Q.assert_fixture(bits, tested, rows.shape[1])
    K, y = T.kinship_and_phenotype(S)
    base, acc = write_case(tmp_path, rows, S_f, pick)
    return {"S": S, "bits": bits, "tested": tested, "pick": pick, "rows": rows, "distinct": distinct, "K": K, "y": y, "base": base,
            "acc": acc, "mc": Q.min_count_of(S)}


@pytest.mark.parametrize("piece,chunk", Q.GEOMETRIES[:2])
def test_full_cache(repeated67, monkeypatch, piece, chunk):
    monkeypatch.delenv("KGWAS_LMM_PATTERN_TAG_BITS", raising=False)
    f = repeated67
    assert f["distinct"] > 3 * 64
    set_piece(monkeypatch, piece)
    tbl, m = kg.KmersTable(f["base"], T.K_LEN), kg.LmmLrt(f["K"], chunk_variants=chunk)
    try:
        yard, (res,) = both(m, tbl, f["pick"], f["y"], f["mc"], Q.ROWS, 64, "64 slots")
    finally:
        m.close()
        tbl.close()
    u = res["unique"]
    print(u, "distinct", f["distinct"])
    assert u["slots"] == 64 and u["patterns_cached"] <= 64 and u["rows_rejected"] > 0
    assert f["distinct"] <= u["rows_rotated"] <= res["rows_tested"]


@pytest.mark.parametrize("piece,chunk", Q.GEOMETRIES[:2])
def test_colliding_tags(repeated67, monkeypatch, piece, chunk):
    f = repeated67
    monkeypatch.setenv("KGWAS_LMM_PATTERN_TAG_BITS", "4")
    set_piece(monkeypatch, piece)
    tbl, m = kg.KmersTable(f["base"], T.K_LEN), kg.LmmLrt(f["K"], chunk_variants=chunk)
    try:
        yard, (a, b) = both(m, tbl, f["pick"], f["y"], f["mc"], Q.ROWS, 4096, "4-bit tags", runs=2)
    finally:
        m.close()
        tbl.close()
    u = a["unique"]
    print(u, "distinct", f["distinct"])
    assert u["rows_collided"] > 0 and u["patterns_cached"] <= 16 and u["rows_rejected"] == 0
    assert u["patterns_cached"] + u["rows_collided"] >= f["distinct"]
    assert b["unique"] == u, "the counters of two runs differ"


# ---- 3. no duplicate, one pattern, no tested row -------------------------------------------------------------------------------
def test_no_duplicate(tmp_path, monkeypatch):
    monkeypatch.delenv("KGWAS_LMM_PATTERN_TAG_BITS", raising=False)
    set_piece(monkeypatch, 1024)
    S, S_f = 67, 70
    bits = T.random_bits(Q.ROWS, S, 21)
    tested = Q.tested_of(bits, S)
    n_tested = int(tested.sum())
    assert len(np.unique(np.packbits(bits[tested], axis=1), axis=0)) == n_tested > 1000, "the fixture repeats a tested pattern"
    pick = Q.pick_of(S, S_f)
    base, _ = write_case(tmp_path, T.table_from_bits(bits, S_f, pick, 21), S_f, pick)
    K, y = T.kinship_and_phenotype(S)
    tbl, m = kg.KmersTable(base, T.K_LEN), kg.LmmLrt(K, chunk_variants=64)
    try:
        # 65536 slots for fewer than 3000 patterns: 16 taken slots in a row do not happen, so nothing is rejected
        yard, (res,) = both(m, tbl, pick, y, Q.min_count_of(S), Q.ROWS, 65536, "no duplicate")
    finally:
        m.close()
        tbl.close()
    u = res["unique"]
    assert res["rows_tested"] == n_tested and u["rows_from_cache"] == 0 and u["rows_rotated"] == n_tested
    assert u["patterns_cached"] == n_tested and u["rows_collided"] == 0 and u["rows_rejected"] == 0


def test_every_tested_row_the_same_pattern(tmp_path, monkeypatch):
    monkeypatch.delenv("KGWAS_LMM_PATTERN_TAG_BITS", raising=False)
    set_piece(monkeypatch, 256)
    S = 67
    one = T.bits_with_counts([20], S, 3)[0]
    out = T.bits_with_counts([0, 1, 4, S, S - 1, S - 4], S, 4)
    rng = np.random.default_rng(8)
    which = rng.integers(0, 8, 1500)  # 6, 7: the tested pattern; 0 .. 5: a row that is not tested
    bits = np.where((which >= 6)[:, None], one[None, :], out[np.minimum(which, 5)])
    tested = Q.tested_of(bits, S)
    assert (tested == (which >= 6)).all() and tested.sum() > 300 and np.flatnonzero(tested).max() // 256 >= 4
    pick = np.arange(S)
    base, _ = write_case(tmp_path, T.table_from_bits(bits, S, pick, 5), S, pick)
    K, y = T.kinship_and_phenotype(S)
    tbl, m = kg.KmersTable(base, T.K_LEN), kg.LmmLrt(K, chunk_variants=32)
    try:
        yard, (res,) = both(m, tbl, pick, y, 5, 10, 64, "one pattern")
    finally:
        m.close()
        tbl.close()
    u = res["unique"]
    assert u["rows_rotated"] == 1 and u["patterns_cached"] == 1 and u["rows_from_cache"] == int(tested.sum()) - 1
    # the best 10 of rows with one lrt: the first ten
    assert res["row"].tolist() == np.flatnonzero(tested)[:10].tolist() and len(set(res["lrt"].tolist())) == 1


def test_no_row_tested(tmp_path, monkeypatch):
    set_piece(monkeypatch, 64)
    S = 67
    K, y = T.kinship_and_phenotype(S)
    pick = np.arange(S)
    rows = T.table_from_bits(T.bits_with_counts([0, 1, 2, 4, S, S - 4, S - 1] * 40, S, 1), S, pick, 2)
    base, _ = write_case(tmp_path, rows, S, pick)
    tbl, m = kg.KmersTable(base, T.K_LEN), kg.LmmLrt(K, chunk_variants=64)
    try:
        yard, (res,) = both(m, tbl, pick, y, 5, 100, 64, "no tested row")
    finally:
        m.close()
        tbl.close()
    assert len(res["row"]) == 0 and res["rows_read"] == len(rows) and res["rows_tested"] == 0
    assert res["unique"] == dict(zip(COUNTERS, (64, 0, 0, 0, 0, 0)))


# ---- 4. the cut at the best N --------------------------------------------------------------------------------------------------
def test_cut_at_best_n(repeated67, monkeypatch):
    monkeypatch.delenv("KGWAS_LMM_PATTERN_TAG_BITS", raising=False)
    f = repeated67
    set_piece(monkeypatch, 1024)
    g = Q.geometry(f["bits"], f["tested"], Q.ROWS, f["rows"].shape[1], 1024, 32)
    tbl, m = kg.KmersTable(f["base"], T.K_LEN), kg.LmmLrt(f["K"], chunk_variants=32)
    try:
        full, _ = both(m, tbl, f["pick"], f["y"], f["mc"], Q.ROWS, 4096, "all rows")
        assert full["row"].tolist() == g["rows"].tolist()
        order = np.lexsort((full["row"], -full["lrt"]))  # the ranking: lrt descending, then the table row
        # two copies of one pattern next to each other in the ranking, in different pieces: N = the place of the first cuts between
        cuts = [i + 1 for i in range(len(order) - 1)
                if g["pattern"][order[i]] == g["pattern"][order[i + 1]] and g["piece"][order[i]] != g["piece"][order[i + 1]]]
        assert len(cuts) >= 10, "no cut between two copies in different pieces"
        cut = cuts[len(cuts) // 2]
        first, second = order[cut - 1], order[cut]
        assert full["lrt"][first].tobytes() == full["lrt"][second].tobytes() and full["row"][first] < full["row"][second]
        for best in (1, 7, 100, cut):
            yard, (res,) = both(m, tbl, f["pick"], f["y"], f["mc"], best, 4096, "best %d" % best)
            assert res["row"].tolist() == np.sort(full["row"][order[:best]]).tolist(), "best %d: not the best by (lrt, row)" % best
        assert full["row"][first] in res["row"] and full["row"][second] not in res["row"], "the earlier of two copies must stay"
    finally:
        m.close()
        tbl.close()


# ---- 5. covariates, repeated calls, the refusal --------------------------------------------------------------------------------
def test_covariates_on_the_handle(repeated67, monkeypatch):
    monkeypatch.delenv("KGWAS_LMM_PATTERN_TAG_BITS", raising=False)
    f = repeated67
    set_piece(monkeypatch, 1000)
    W = np.c_[np.ones(f["S"]), np.random.default_rng(2).standard_normal(f["S"])]
    tbl, m, plain = kg.KmersTable(f["base"], T.K_LEN), kg.LmmLrt(f["K"], chunk_variants=64, covariates=W), kg.LmmLrt(f["K"], chunk_variants=64)
    try:
        yard, (res,) = both(m, tbl, f["pick"], f["y"], f["mc"], Q.ROWS, 4096, "q = 2")
        assert res["unique"]["patterns_cached"] == f["distinct"]
        other = plain.test_table(tbl, np.asarray(f["pick"], np.uint64), f["y"], f["mc"], Q.MAF, Q.ROWS)
        assert other["lrt"].tobytes() != yard["lrt"].tobytes(), "the covariates change nothing: the case shows nothing"
    finally:
        m.close()
        plain.close()
        tbl.close()


def test_repeated_calls_empty_the_cache(repeated67, monkeypatch):
    monkeypatch.delenv("KGWAS_LMM_PATTERN_TAG_BITS", raising=False)
    f = repeated67
    set_piece(monkeypatch, 1024)
    y2 = np.random.default_rng(9).permutation(f["y"])
    tbl, m = kg.KmersTable(f["base"], T.K_LEN), kg.LmmLrt(f["K"], chunk_variants=64)
    col = np.asarray(f["pick"], np.uint64)
    try:
        yard1 = m.test_table(tbl, col, f["y"], f["mc"], Q.MAF, Q.ROWS)
        yard2 = m.test_table(tbl, col, y2, f["mc"], Q.MAF, Q.ROWS)
        assert yard1["lrt"].tobytes() != yard2["lrt"].tobytes()
        for y, yard in ((f["y"], yard1), (y2, yard2), (f["y"], yard1)):
            res = m.test_table(tbl, col, y, f["mc"], Q.MAF, Q.ROWS, max_patterns=4096)
            assert_same(res, yard, "the second phenotype on one handle")
            assert res["unique"]["patterns_cached"] == f["distinct"] and res["unique"]["rows_rejected"] == 0
    finally:
        m.close()
        tbl.close()


def test_small_cache_is_refused(repeated67):
    f = repeated67
    tbl, m = kg.KmersTable(f["base"], T.K_LEN), kg.LmmLrt(f["K"], chunk_variants=64)
    col = np.asarray(f["pick"], np.uint64)
    try:
        before = m.stats()
        us = capi.LmmUniqueStats(*([77] * 6))
        kept = C.c_uint64(99)
        rc = capi.lib.kgwas_lmm_test_table_unique(m._h, capi.ptr(np.ascontiguousarray(f["y"])), tbl._h, capi.ptr(col), len(col), f["mc"], Q.MAF,
                                                  10, None, None, None, None, None, None, C.byref(kept), None, None, 63, C.byref(us))
        assert rc == capi.KGWAS_ERR_ARG and b"max_patterns" in capi.lib.kgwas_last_error()
        assert us.as_dict() == dict(zip(COUNTERS, [77] * 6)) and kept.value == 99 and m.stats() == before
        with pytest.raises(kg.KgwasError) as e:
            m.test_table(tbl, col, f["y"], f["mc"], Q.MAF, 10, max_patterns=0)
        assert e.value.code == capi.KGWAS_ERR_ARG
        both(m, tbl, f["pick"], f["y"], f["mc"], 10, 64, "the call after the refusal")
        # 127 slots asked for: 64 taken
        assert m.test_table(tbl, col, f["y"], f["mc"], Q.MAF, 10, max_patterns=127)["unique"]["slots"] == 64
    finally:
        m.close()
        tbl.close()


# ---- 6. the tool ---------------------------------------------------------------------------------------------------------------
def test_cli_pattern_cache(repeated67, tmp_path):
    f = repeated67
    ph = tmp_path / "ph.tsv"
    ph.write_text("accession_id\tv\n" + "".join("%s\t%r\n" % (a, float(v)) for a, v in zip(f["acc"], f["y"])))
    cov = tmp_path / "cov.txt"
    cov.write_text("".join("1 %r\n" % float(v) for v in np.random.default_rng(2).standard_normal(f["S"])))
    kin = tmp_path / "k.txt"
    kin.write_text("\n".join("\t".join("%.17g" % v for v in r) for r in f["K"]) + "\n")
    out = str(tmp_path / "out")
    common = [os.path.join(BINDIR, "lmm_lrt"), "--kmers_table", f["base"], "--kmers_len", str(T.K_LEN), "-p", str(ph), "-lmm", "2", "-k",
              str(kin), "-outdir", out, "--mac", "5", "-maf", "0.05", "--best", "200", "--chunk_variants", "64"]
    for tag, extra in (("plain", []), ("cov", ["-c", str(cov)])):
        r0 = subprocess.run(common + extra + ["-o", tag], capture_output=True, text=True, timeout=300)
        r1 = subprocess.run(common + extra + ["-o", tag + "_u", "--pattern_cache", "64"], capture_output=True, text=True, timeout=300)
        assert r0.returncode == 0 and r1.returncode == 0, r0.stderr[-1000:] + r1.stderr[-1000:]
        a, b = (open(os.path.join(out, "%s.assoc.txt" % t), "rb").read() for t in (tag, tag + "_u"))
        assert a == b and a.count(b"\n") == 201, "the .assoc.txt differs with --pattern_cache (%s)" % tag
        l0, l1 = ([l.split("\t")[0].split(" ")[0] for l in open(os.path.join(out, "%s.log.txt" % t)).read().split("\n") if l] for t in (tag, tag + "_u"))
        extra_lines = ["pattern_cache_slots", "patterns_cached", "rows_from_cache", "rows_collided", "rows_rejected", "rows_rotated"]
        assert l1[:len(l0)] == l0 and l1[len(l0):] == extra_lines, l1
        log = dict(l.split("\t", 1) for l in open(os.path.join(out, tag + "_u.log.txt")).read().split("\n") if "\t" in l)
        assert int(log["patterns_cached"]) == f["distinct"] == int(log["rows_rotated"]) and int(log["rows_tested"]) == int(f["tested"].sum())
        slots = int(log["pattern_cache_slots"])
        assert slots & (slots - 1) == 0 and slots * (40 + 80 // 4) <= 64 << 20 < 2 * slots * (40 + 80 // 4)  # a slot: 40 bytes + the code row
        assert "rows_rotated=%d" % f["distinct"] in r1.stderr and "rows_rotated" not in r0.stderr
