"""The multi-phenotype pass of lmm_lrt (kgwas_lmm_test_bed_multi, kgwas_lmm_run_file_multi, lmm_lrt --columns) on the GPU.

Its contract is bit identity with the single-phenotype path: every sum of lmm_grid_xy_kernel is the MFMA chain of
lmm_grid_kernel's xt yt row, the shared rows come from the same kernel, and base sums, null models and the refinement run the
same code per column. So the tests compare raw bytes (NaNs included) against P kgwas_lmm_null / kgwas_lmm_test_bed calls, at the
smallest shapes that cross every boundary: individuals past a 16 and a 64 multiple (5, 67, 241), variants past a 16-row tile and
a 64-variant chunk (17, 130), columns past a phenotype tile (LMM_PTILE = 4) and a phenotype block (LMM_PBLOCK, LMM_PBLOCK + 1).
The comparison with arithmetic uses test_gpu_lmm_lrt.py's tolerances, imported.
"""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from kmersgwas_amd import capi
from kmersgwas_amd.capi import lib, ptr

import lmm_lrt_np as M
from test_gpu_lmm_lrt import BIN, LRT_TOL, ROWS, Handle, check_p

pytestmark = pytest.mark.gpu

_HDR = open(os.path.join(os.path.dirname(os.path.abspath(capi.__file__)), "csrc", "lmm_kernels.h")).read()
LMM_PBLOCK = int(re.search(r"constexpr uint32_t LMM_PBLOCK = (\d+);", _HDR).group(1))
LMM_PTILE = int(re.search(r"constexpr uint32_t LMM_PTILE = (\d+);", _HDR).group(1))
PMAX = LMM_PBLOCK + 1
MAF, MISS = 0.15, 0.25
KEYS = ("lrt", "lam", "p", "af", "n_miss", "tested", "l0", "lam0")


def multi_rc(h, Y, bed, maf=0.0, miss=1.0):
    """(return code, outputs) of kgwas_lmm_test_bed_multi on a test_gpu_lmm_lrt.Handle"""
    Y = np.ascontiguousarray(Y, np.float64).reshape(-1, h.n)
    bed = np.ascontiguousarray(bed, np.uint8)
    P, m = Y.shape[0], bed.size // ((h.n + 3) // 4)
    out = dict(lrt=np.zeros((P, m)), lam=np.zeros((P, m)), p=np.zeros((P, m)), l0=np.zeros(P), lam0=np.zeros(P), af=np.zeros(m),
               n_miss=np.zeros(m, np.uint32), tested=np.zeros(m, np.uint8))
    rc = lib.kgwas_lmm_test_bed_multi(h.h, P, ptr(Y), ptr(bed), m, maf, miss, ptr(out["lrt"]), ptr(out["lam"]), ptr(out["p"]),
                                      ptr(out["l0"]), ptr(out["lam0"]), ptr(out["af"]), ptr(out["n_miss"]), ptr(out["tested"]))
    return rc, out


def multi(h, Y, bed, **kw):
    rc, out = multi_rc(h, Y, bed, **kw)
    capi.check(rc)
    return out


def singles(h, Y, bed, **kw):
    """The same outputs from one kgwas_lmm_test_bed and one kgwas_lmm_null call per column"""
    outs = []
    for y in Y:
        o = h.test(bed, y, **kw)
        o["l0"], o["lam0"] = h.null(y)
        outs.append(o)
    res = {k: np.stack([o[k] for o in outs]) for k in ("lrt", "lam", "p")}
    res["l0"], res["lam0"] = np.array([o["l0"] for o in outs]), np.array([o["lam0"] for o in outs])
    for k in ("af", "n_miss", "tested"):
        assert all(o[k].tobytes() == outs[0][k].tobytes() for o in outs)
        res[k] = outs[0][k]
    return res


def differing(a, b, cols=slice(None)):
    """names of the outputs whose raw bytes differ (per-column ones restricted to cols of b)"""
    bad = []
    for k in KEYS:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k][cols] if k in ("lrt", "lam", "p", "l0", "lam0") else b[k])
        if x.shape != y.shape or x.tobytes() != y.tobytes():
            bad.append(k)
    return bad


@functools.lru_cache(maxsize=None)
def handle(n, chunk=64):
    return Handle(M.fixture(n, ROWS[n], 3.0)[1], chunk)


@pytest.fixture(scope="module", autouse=True)
def close_shared_handles():
    """the handles of handle() are shared by the tests of this module and closed after the last of them"""
    yield
    single_reference.cache_clear()
    for n in (5, 67, 241):
        handle(n).close()
    handle.cache_clear()


@functools.lru_cache(maxsize=None)
def phenotypes(n):
    """PMAX columns: the fixture's phenotype, the hg = 0 fixture's, then permutations of the first"""
    rng = np.random.default_rng([41, n])
    y = M.fixture(n, ROWS[n], 3.0)[2]
    Y = np.stack([y, M.fixture(n, ROWS[n], 0.0)[2]] + [rng.permutation(y) for _ in range(PMAX - 2)])
    Y.setflags(write=False)
    return Y


@functools.lru_cache(maxsize=None)
def panel(n, nv):
    """nv variants with heterozygous and missing calls, a constant one and one under the maf filter, as a .bed body"""
    G = M.fixture(n, ROWS[n], 3.0)[0]
    rng = np.random.default_rng([43, n, nv])
    D = 2 * M.varying(G)[:nv].astype(np.int64)
    assert len(D) == nv
    D[5:12][rng.random((7, n)) < 0.2] = 1
    D[1, 0] = D[2, 0] = D[8, n - 1] = -1  # missing calls (1 / n <= MISS)
    D[9, :(n + 1) // 2] = -1                # too many of them
    D[3] = 2                                # constant
    D[4] = 0
    D[4, 0] = 1                             # af = 1 / 2n < MAF
    return D, M.pack_bed(D)


@functools.lru_cache(maxsize=None)
def single_reference(n, nv):
    """made once per shape, shared by the cases of test_bit_identity and left unchanged"""
    return singles(handle(n), phenotypes(n), panel(n, nv)[1], maf=MAF, miss=MISS)


@pytest.mark.parametrize("P", [1, 3, LMM_PBLOCK, LMM_PBLOCK + 1])
@pytest.mark.parametrize("nv", [17, 130])
@pytest.mark.parametrize("n", [5, 67, 241])
def test_bit_identity(n, nv, P):
    ref = single_reference(n, nv)
    out = multi(handle(n), phenotypes(n)[:P], panel(n, nv)[1], maf=MAF, miss=MISS)
    t = out["tested"].astype(bool)
    assert not t[3] and not t[4] and not t[9] and 4 <= t.sum() < nv and out["n_miss"].any()
    assert np.isnan(out["lrt"][:, ~t]).all() and np.isfinite(out["lrt"][:, t]).all() and np.isfinite(out["l0"]).all()
    assert differing(out, ref, slice(0, P)) == []


def test_against_arithmetic():
    n, nv = 241, 17
    G, K, _ = M.fixture(n, ROWS[n], 3.0)
    V = M.varying(G)[:nv]
    Y = phenotypes(n)
    col = LMM_PBLOCK  # the one column of the second phenotype block
    out = multi(handle(n), Y, M.presence_bed(V))
    ref, l0 = M.lrt_E(K, Y[col], V.astype(np.float64))
    err = np.abs(out["lrt"][col] - ref).max()
    print("n=241 column %d: max |LRT - model E| = %.3e (allowed %.1e), |l0 - model E| = %.3e" % (col, err, LRT_TOL, abs(out["l0"][col] - l0)))
    assert out["tested"].all() and err <= LRT_TOL and abs(out["l0"][col] - l0) <= LRT_TOL
    check_p({"lrt": out["lrt"][col], "p": out["p"][col]})


def test_order_and_blocks():
    n, nv = 67, 130
    Y, bed = phenotypes(n), panel(n, nv)[1]
    a = multi(handle(n), Y, bed, maf=MAF, miss=MISS)
    perm = np.random.default_rng(3).permutation(PMAX)
    assert differing(multi(handle(n), Y[perm], bed, maf=MAF, miss=MISS), a, perm) == [], "a permuted column order changes a column's numbers"
    twice = [2, 7, 2] + [k % PMAX for k in range(8, 8 + LMM_PBLOCK)] + [2]  # the same column in two tiles and two blocks
    b = multi(handle(n), Y[twice], bed, maf=MAF, miss=MISS)
    assert differing(b, a, twice) == []
    for k in ("lrt", "lam", "p"):
        assert b[k][0].tobytes() == b[k][2].tobytes() == b[k][-1].tobytes()
    for chunk in (32, 10240):
        h = Handle(M.fixture(n, ROWS[n], 3.0)[1], chunk)
        try:
            assert differing(multi(h, Y, bed, maf=MAF, miss=MISS), a) == [], "chunk_variants 64 and %d differ" % chunk
        finally:
            h.close()


def test_state():
    n, nv = 67, 130
    Y, bed = phenotypes(n), panel(n, nv)[1]
    h = Handle(M.fixture(n, ROWS[n], 3.0)[1], 64)
    try:
        y0 = Y[5]
        first = h.test(bed, y0, maf=MAF, miss=MISS)
        first_null = h.null(y0)
        ref = multi(h, Y[:6], bed, maf=MAF, miss=MISS)
        last = h.test(bed, y0, maf=MAF, miss=MISS)
        assert all(first[k].tobytes() == last[k].tobytes() for k in first) and h.null(y0) == first_null
        for bad, word in ((np.full(n, 2.5), "constant"), (np.where(np.arange(n) == 3, np.nan, Y[1]), "not finite")):
            Yb = Y[:6].copy()
            Yb[4] = bad
            rc, _ = multi_rc(h, Yb, bed)
            msg = (lib.kgwas_last_error() or b"").decode()
            assert rc == capi.KGWAS_ERR_ARG and word in msg and "column 4" in msg, (rc, msg)
            assert differing(multi(h, Y[:6], bed, maf=MAF, miss=MISS), ref) == [], "the handle is not usable after a refusal"
        rc, _ = multi_rc(h, np.zeros((0, n)), bed)
        assert rc == capi.KGWAS_ERR_ARG and "n_pheno" in (lib.kgwas_last_error() or b"").decode()
        last = h.test(bed, y0, maf=MAF, miss=MISS)
        assert all(first[k].tobytes() == last[k].tobytes() for k in first)
        assert differing(multi(h, Y[:6], bed, maf=MAF, miss=MISS), ref) == []
    finally:
        h.close()


# ---- the command-line tool ----

def _write_files(tmp_path, name, D, pheno):
    """D (variants x individuals, dosages) and pheno (individuals x columns, NaN = missing) as name.bed / .bim / .fam"""
    base = str(tmp_path / name)
    open(base + ".bed", "wb").write(bytes([0x6C, 0x1B, 0x01]) + M.pack_bed(D).tobytes())
    open(base + ".bim", "w").write("".join("%d\trs%d\t0\t%d\tA\tC\n" % (1 + v % 5, v, 100 + v) for v in range(len(D))))
    open(base + ".fam", "w").write("".join("f%d i%d 0 0 0 %s\n" % (i, i, " ".join("-9" if np.isnan(x) else "%.17g" % x for x in row))
                                           for i, row in enumerate(pheno)))
    return base


def test_cli(tmp_path):
    n, nv = 67, 130
    K = M.fixture(n, ROWS[n], 3.0)[1]
    D = panel(n, nv)[0]
    pheno = phenotypes(n)[:5].T.copy()
    pheno[[2, 30, 66]] = np.nan  # three individuals without a phenotype, the same in every column
    base = _write_files(tmp_path, "panel", D, pheno)
    kin = str(tmp_path / "pheno.kinship")
    open(kin, "w").write("\n".join("\t".join("%.17g" % v for v in r) for r in K) + "\n")
    outdir = str(tmp_path / "out")
    lst = str(tmp_path / "columns.txt")
    open(lst, "w").write("".join("%d\tC%d\n" % (c, c) for c in (1, 2, 3, 4, 5)))
    common = ["-lmm", "2", "-k", kin, "-outdir", outdir, "-maf", "0.05", "-miss", "0.5", "--chunk_variants", "64"]
    r = subprocess.run([BIN, "-bfile", base, "--columns", lst] + common, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "eigendecompositions=1 " in r.stderr and "columns=5 " in r.stderr and "individuals=64 " in r.stderr, r.stderr
    for c in (1, 2, 3, 4, 5):
        r = subprocess.run([BIN, "-bfile", base, "-n", str(c), "-o", "S%d" % c] + common, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        single = open(os.path.join(outdir, "S%d.assoc.txt" % c), "rb").read()
        assert open(os.path.join(outdir, "C%d.assoc.txt" % c), "rb").read() == single and 10 < single.count(b"\n") < nv + 1
        log_m, log_s = (open(os.path.join(outdir, "%s%d.log.txt" % (x, c))).read().split("\n") for x in "CS")
        assert log_m[:9] == log_s[:9] and log_m[4] == "individuals_used\t64"  # everything but the line of milliseconds
    # column 3 with another missing set
    pheno[30, 2] = 0.5
    pheno[31, 2] = np.nan
    other = _write_files(tmp_path, "other", D, pheno)
    r = subprocess.run([BIN, "-bfile", other, "--columns", lst] + common, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "column 3" in r.stderr, r.stderr


def test_python_class():
    import kmersgwas_amd as kg
    n, nv = 67, 130
    K = M.fixture(n, ROWS[n], 3.0)[1]
    Y, bed = phenotypes(n)[:7], panel(n, nv)[1]
    m = kg.LmmLrt(K, lmin=M.LMIN, lmax=M.LMAX, chunk_variants=64)
    try:
        r = m.test_bed_multi(Y, bed.tobytes(), maf=MAF, miss=MISS)
        assert r["lrt"].shape == r["lambda"].shape == r["p"].shape == (7, nv)
        assert r["logl0"].shape == r["lambda0"].shape == (7,) and r["af"].shape == r["n_miss"].shape == r["tested"].shape == (nv,)
        assert r["tested"].dtype == bool and m.stats()["variants_read"] == nv and m.stats()["variants_tested"] == 7 * r["tested"].sum()
        c = multi(handle(n), Y, bed, maf=MAF, miss=MISS)
        r.update(lam=r["lambda"], l0=r["logl0"], lam0=r["lambda0"], tested=r["tested"].astype(np.uint8))
        assert differing(r, c) == []
        with pytest.raises(ValueError):
            m.test_bed_multi(Y[:, :-1], bed)
    finally:
        m.close()
