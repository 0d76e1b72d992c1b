"""What the matrix-pipe filters KEEP, pair by pair, against the exact model of tests/filter_model.py.

Every other GPU test looks at the heaps at the end of a scan; a filter that keeps too much (its survivors are re-scored exactly and
thrown away), or that loses a pair which a later row would have evicted anyway, passes them all. Here a session created under
KGWAS_DEBUG_SURVIVORS=1 reports, for every filtered chunk, the thresholds its filter launches read and the (column, row) pairs
of its key list (kgwas_scan_debug_survivors), and with the session's own quantisation residuals (kgwas_scan_debug_residuals)
the model says which pairs must be there (I), which may (O \\ I: float32 evaluation) and which must not:

    R <= I <= survivors <= O        for every logged chunk and column, against that chunk's thresholds.

The cases, their tables and phenotypes live in tests/filter_model.py; tests/test_filter_model.py qualifies each of them on the
CPU (thin rounding band, enough pairs at the thresholds) before the device sees it, and the same conditions are asserted here
again with the real residuals and thresholds."""
import ctypes as C
import time

import numpy as np
import pytest

import kmersgwas_amd as kg
from kmersgwas_amd import capi
from oracle import binding as ob
import filter_model as fm
from helpers import check_topn

pytestmark = pytest.mark.gpu


def _logged_chunks(scan, P):
    n = C.c_uint64(0)
    assert capi.lib.kgwas_scan_debug_survivors(scan._h, C.byref(n), 0, None, None, None) == 0, capi.lib.kgwas_last_error()
    out = []
    for ci in range(n.value):
        info = (C.c_uint64 * 5)()
        thr = np.zeros(P, np.float64)
        assert capi.lib.kgwas_scan_debug_survivors(scan._h, None, ci, info, thr.ctypes.data, None) == 0, capi.lib.kgwas_last_error()
        pairs = np.zeros((int(info[4]), 2), np.uint32)
        if info[4]:
            assert capi.lib.kgwas_scan_debug_survivors(scan._h, None, ci, None, None, pairs.ctypes.data) == 0, capi.lib.kgwas_last_error()
        out.append(dict(first=int(info[0]), n=int(info[1]), set=int(info[2]), overflow=int(info[3]), thr=thr, pairs=pairs))
    return out


def _describe(what, bad, n1, T, chunk_of, chunks):
    """The first pairs of a failed inclusion, with what locates them in a kernel: chunk, row in chunk (and in its 64-row wave
    pass), column (tile, slot)."""
    rr, pp = np.nonzero(bad)
    lines = ["%s: %d pairs" % (what, len(rr))]
    for r, p in list(zip(rr, pp))[:12]:
        ch = chunks[chunk_of[r]]
        lines.append("  chunk %d (first row %d, %d rows, set %d) row %d (%% 64 = %d) column %d (tile %d slot %d) N1 %d thr %.17g"
                     % (chunk_of[r], ch["first"], ch["n"], ch["set"], r - ch["first"], (r - ch["first"]) % 64, p, p // 16, p % 16, n1[r], T[r, p]))
    return "\n".join(lines)


@pytest.mark.parametrize("case", fm.CASES, ids=[c["name"] for c in fm.CASES])
def test_filter_keeps_its_inner_set_and_nothing_outside_its_outer_set(case, monkeypatch, capsys):
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("KGWAS_DEBUG_RESIDUALS", "1")
    monkeypatch.setenv("KGWAS_DEBUG_SURVIVORS", "1")
    t0 = time.time()
    S_f, S, P, n, topn = case["S_f"], case["S"], case["P"], case["n"], case["topn"]
    rows, col = fm.case_table(case)
    Y = fm.case_phenotypes(case)
    mac = fm.min_count(S)
    g, n1, keep = fm.unpack(rows, col)
    exp = ob.associate(rows, S_f, col, Y, topn, mac, threads=8)
    scores, kept = ob.scores_dense(rows, S_f, col, Y, mac)
    assert (kept == keep).all()

    scan = kg.AssociationScan(S_f, col, Y, topn, mac, chunk_rows=case["chunk_rows"])
    for a, b in fm.case_feeds(case):
        scan.feed_host(rows[a:b], a)
    scan.finish()
    st = scan.stats()
    chunks = _logged_chunks(scan, P)
    resid = {}
    for form in case["forms"].values():
        resid[form] = np.zeros((P, S))
        for j in range(P):
            assert capi.lib.kgwas_scan_debug_residuals(scan._h, fm.FORMS[form][2], j, resid[form][j].ctypes.data) == 0, capi.lib.kgwas_last_error()

    # the intended kernel form ran
    ex = case["expect"]
    assert st["kernel_used"] == (kg.KERNEL_NARROW if ex.get("narrow") else kg.KERNEL_COARSE), st
    for key in ("coarse_mx", "coarse_mx_stream", "coarse_mx_steps", "coarse_mx_s1_fp6"):
        if key in ex:
            assert st[key] == ex[key], (key, st)
    for key, field in (("lgroups1", "coarse_mode_lgroups"), ("tiles1", "coarse_mode_tiles"), ("tile_slices1", "coarse_mode_tile_slices")):
        if key in ex:
            assert st[field][1] == ex[key], (key, st)
    if ex.get("launches0"):
        assert st["coarse_mode_launches"][0] > 0 and st["coarse_mode_launches"][1] == 0, st
    sets_seen = sorted(set(ch["set"] for ch in chunks))
    assert sets_seen == sorted(case["forms"]), (sets_seen, "both operand sets must appear" if ex.get("both_sets") else "")
    assert st["coarse_launches"] == len(chunks)

    # the log itself: chunks inside the feeds, in order, none overflowed; keys in (column, row) order, each once
    assert not any(ch["overflow"] for ch in chunks)
    assert any(ch["n"] % 64 for ch in chunks)
    surv = np.zeros((n, P), bool)
    T = np.full((n, P), np.nan)
    chunk_of = np.full(n, -1)
    set_of = np.full(n, -1)
    end = 0
    for ci, ch in enumerate(chunks):
        assert ch["first"] >= end and ch["first"] + ch["n"] <= n and ch["n"] > 0
        end = ch["first"] + ch["n"]
        pr = ch["pairs"].astype(np.int64)
        assert (pr[:, 0] < P).all() and (pr[:, 1] < ch["n"]).all()
        flat = pr[:, 0] * (1 << 32) + pr[:, 1]
        assert (np.diff(flat) > 0).all(), "chunk %d: keys out of (column, row) order or repeated" % ci
        surv[ch["first"] + pr[:, 1], pr[:, 0]] = True
        T[ch["first"]:end] = ch["thr"][None, :]
        chunk_of[ch["first"]:end] = ci
        set_of[ch["first"]:end] = ch["set"]
        assert np.isfinite(ch["thr"]).all() and (ch["thr"] >= 0).all()
    assert not surv[~keep].any(), "a row outside the MAC rule survived"

    R = np.zeros((n, P), bool)
    I = np.zeros((n, P), bool)
    O = np.zeros((n, P), bool)
    for set_id, form in case["forms"].items():
        m = fm.FilterModel(form, Y, resid=resid[form])
        assert (m.sum == np.array([float(x) for x in fm.chain_sums(Y)])).all()
        rs = np.nonzero(set_of == set_id)[0]
        Rs, Is, Os = m.sets(g[rs], n1[rs], keep[rs], scores[:, rs], T[rs])
        R[rs], I[rs], O[rs] = Rs, Is, Os
    with capsys.disabled():
        print()
        print("  survivors %d (%.2f per required pair)" % (int(surv.sum()), surv.sum() / max(int(R.sum()), 1)), end="")
        try:
            fig = fm.check_conditions(case, n, [(ch["first"], ch["n"], ch["thr"]) for ch in chunks], R, I, O)
        finally:
            print("  %.1f s" % (time.time() - t0))
    assert not (R & ~I).any(), _describe("required pairs outside the bound (R - I)", R & ~I, n1, T, chunk_of, chunks)
    assert not (I & ~surv).any(), _describe("pairs of the inner set the filter dropped (I - survivors)", I & ~surv, n1, T, chunk_of, chunks)
    assert not (surv & ~O).any(), _describe("survivors outside the outer set (survivors - O)", surv & ~O, n1, T, chunk_of, chunks)
    assert not (R & ~surv).any()
    assert fig["R"] >= 500

    assert st["rows_tested"] == exp["tested"]
    check_topn(scan, exp, P)
    scan.close()


# The chunk sizes a resident table is scanned in - the planner's, not a cap of 2048 to 8192 rows as above. Only there a narrow
# chunk spans several 65 536-row segments (blocks of 768 rows straddle their boundaries: the per-block two-segment counters, the
# key kernel's cross-segment offsets) and a wide chunk several 1024-word bitmap blocks (the count scan's carry, the scatter
# kernel's column base). The model's inner and outer sets stay with the 24 k-row cases above; here every pair above its chunk's
# threshold must be listed, each key once and in order, and the heaps must be the oracle's.
_PLANNER_CASES = [
    # name, columns, table rows, narrow, rows a chunk must exceed (narrow: 262 144 rows = four segments and a 768-row block
    # across every boundary between them; wide: more than 131 072 rows = three bitmap blocks)
    ("narrow_241x1_pack1", 1, 600_011, True, 262_144 - 1),
    ("narrow_241x4", 4, 600_011, True, 262_144 - 1),
    ("wide_241x5", 5, 300_011, False, 131_072),
]


@pytest.mark.parametrize("name,P,n,narrow,big", _PLANNER_CASES, ids=[c[0] for c in _PLANNER_CASES])
def test_survivors_at_the_planners_chunk_sizes(name, P, n, narrow, big, monkeypatch):
    import torch
    monkeypatch.setenv("KGWAS_DEBUG_SURVIVORS", "1")
    S, topn, seed = 241, 100, 4711 + P
    W = 1 + (S + 63) // 64  # 40 bytes per row: the staged narrow kernel reads a wave's 64 rows as three KB
    rng = np.random.default_rng(31 + P)
    y0 = rng.standard_normal(S).astype(np.float32)
    Y = np.stack([y0] + [rng.permutation(y0) for _ in range(P - 1)]).astype(np.float32)
    col = np.arange(S, dtype=np.uint64)
    mac = fm.min_count(S)
    stream = torch.cuda.current_stream().cuda_stream
    t = torch.empty(n * W, dtype=torch.int64, device="cuda")
    kg.synth_rows_device(t.data_ptr(), 0, n, S, seed, stream)
    rows = kg.synth_rows_host(0, n, S, seed)
    exp = ob.associate(rows, S, col, Y, topn, mac, threads=8)
    scores, keep = ob.scores_dense(rows, S, col, Y, mac)

    scan = kg.AssociationScan(S, col, Y, topn, mac)  # chunk_rows = 0: the planner's chunks
    scan.feed_device(t.data_ptr(), n, 0, stream)
    scan.finish()
    st = scan.stats()
    chunks = _logged_chunks(scan, P)

    # not vacuous: the intended path, at the sizes the case exists for
    assert st["kernel_used"] == (kg.KERNEL_NARROW if narrow else kg.KERNEL_COARSE) and st["direct_mode"] == 1, st
    assert not any(ch["overflow"] for ch in chunks)
    sizes = [ch["n"] for ch in chunks]
    assert max(sizes) > big, sizes
    assert any(x % 64 for x in sizes), sizes
    if narrow:
        assert max((x + 65535) // 65536 for x in sizes) >= 5, sizes  # n_segs

    surv = np.zeros((n, P), bool)
    must = np.zeros((n, P), bool)
    end = 0
    for ci, ch in enumerate(chunks):
        assert ch["first"] >= end and ch["first"] + ch["n"] <= n and ch["n"] > 0
        end = ch["first"] + ch["n"]
        pr = ch["pairs"].astype(np.int64)
        assert (pr[:, 0] < P).all() and (pr[:, 1] < ch["n"]).all()
        flat = pr[:, 0] * (1 << 32) + pr[:, 1]
        assert (np.diff(flat) > 0).all(), "chunk %d: keys out of (column, row) order or repeated" % ci
        surv[ch["first"] + pr[:, 1], pr[:, 0]] = True
        assert np.isfinite(ch["thr"]).all() and (ch["thr"] >= 0).all()
        must[ch["first"]:end] = (scores[:, ch["first"]:end].T > ch["thr"][None, :]) & keep[ch["first"]:end, None]
    assert not surv[~keep].any(), "a row outside the MAC rule survived"
    lost = must & ~surv
    assert not lost.any(), "%d pairs above their chunk's threshold are not among the survivors, first (row, column) %s" % (
        int(lost.sum()), np.argwhere(lost)[:8].tolist())
    assert must.any()

    assert st["rows_tested"] == exp["tested"]
    check_topn(scan, exp, P)
    scan.close()


def test_survivor_log_needs_its_switch(monkeypatch):
    """Without KGWAS_DEBUG_SURVIVORS a session logs nothing and says so."""
    monkeypatch.delenv("KGWAS_DEBUG_SURVIVORS", raising=False)
    case = dict(n=6000, S_f=241, S=241, P=5, cols="perm", pheno="normal")
    rows, col = fm.case_table(case)
    scan = kg.AssociationScan(241, col, fm.case_phenotypes(case), 100, fm.min_count(241), chunk_rows=2048)
    scan.feed_host(rows)
    scan.finish()
    assert scan.stats()["coarse_launches"] > 0
    n = C.c_uint64(7)
    assert capi.lib.kgwas_scan_debug_survivors(scan._h, C.byref(n), 0, None, None, None) == capi.KGWAS_ERR_STATE
    scan.close()
