"""lmm_lrt on the GPU, through the C ABI: statistics against the numpy models of lmm_lrt_np.py, the genotype codes, determinism,
shared eigendecompositions, boundary optima and the command-line tool.

Tolerances (lmm_lrt_np.py has the models; -lmin / -lmax = e^-10 / e^10 everywhere so that tool and models search one range):
  LRT     the two models differ by at most 2.7e-12 on this module's CPU fixtures and by at most 7.0e-11 on those of
          test_gpu_lmm_lrt_regimes.py, at LRT 4720 (test_lmm_lrt_model.py, MEASURED_MODEL_GAP = 7.1e-11). The tool is allowed
          1000 x that gap for its different summation order and eigensolver, capped at 1e-8: LRT_TOL = 1e-8 absolute.
  p       against scipy.stats.chi2.sf(LRT_tool, 1). Largest relative error measured on the GPU over these tests: see
          MEASURED_P_RELERR; asserted with a 10 x margin, cap 1e-9.
  lambda  the optimum is flat (log lambda differs by up to 5e-7 between the models), so lambda is checked through the
          likelihood: model R's l at the tool's lambda is within LRT_TOL of model R's own maximum.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
from scipy.stats import chi2

from kmersgwas_amd import capi
from kmersgwas_amd.capi import lib, ptr

import lmm_lrt_np as M
from test_lmm_lrt_model import MEASURED_MODEL_GAP

pytestmark = pytest.mark.gpu

LRT_TOL = min(1e-8, 1000 * MEASURED_MODEL_GAP)
MEASURED_P_RELERR = 5.5e-14  # largest |p / chi2.sf(LRT, 1) - 1| seen on the MI355X over the lmm modules (test_gpu_lmm_lrt_regimes.py, strong, n = 241, effect 40)
P_RTOL = min(1e-9, 10 * MEASURED_P_RELERR)
BIN = os.path.join(os.path.dirname(os.path.abspath(capi.__file__)), "bin", "lmm_lrt")


class Handle:
    def __init__(self, K, chunk=64, lmin=M.LMIN, lmax=M.LMAX):
        K = np.ascontiguousarray(K, np.float64)
        self.n = K.shape[0]
        self.h = C.c_void_p()
        capi.check(lib.kgwas_lmm_create(self.n, ptr(K), 0, lmin, lmax, chunk, C.byref(self.h)))

    def null(self, y):
        l0, lam0 = C.c_double(), C.c_double()
        capi.check(lib.kgwas_lmm_null(self.h, ptr(np.ascontiguousarray(y, np.float64)), C.byref(l0), C.byref(lam0)))
        return l0.value, lam0.value

    def test(self, bed, y, maf=0.0, miss=1.0):
        bed = np.ascontiguousarray(bed, np.uint8)
        m = bed.size // ((self.n + 3) // 4)
        out = dict(lrt=np.zeros(m), lam=np.zeros(m), p=np.zeros(m), af=np.zeros(m), n_miss=np.zeros(m, np.uint32), tested=np.zeros(m, np.uint8))
        capi.check(lib.kgwas_lmm_test_bed(self.h, ptr(np.ascontiguousarray(y, np.float64)), ptr(bed), m, maf, miss, ptr(out["lrt"]),
                                          ptr(out["lam"]), ptr(out["p"]), ptr(out["af"]), ptr(out["n_miss"]), ptr(out["tested"])))
        return out

    def close(self):
        lib.kgwas_lmm_destroy(self.h)


def run_once(K, y, bed, chunk=64, **kw):
    h = Handle(K, chunk)
    try:
        out = h.test(bed, y, **kw)
        out["l0"], out["lam0"] = h.null(y)
    finally:
        h.close()
    return out


def same_bits(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("lrt", "lam", "p", "af", "n_miss", "tested"))


def check_p(out, sel=slice(None)):
    lrt, p = out["lrt"][sel], out["p"][sel]
    ref = chi2.sf(lrt, 1)
    rel = np.abs(p / ref - 1.0)
    print("p: largest relative error against chi2.sf %.3e (allowed %.1e)" % (rel.max(), P_RTOL))
    assert rel.max() <= P_RTOL


def check_lambda(K, y, xs, lams):
    """model R's l at the tool's lambda against model R's own maximum"""
    one = np.ones(y.size)
    worst = 0.0
    for x, lam in zip(xs, lams):
        best, _ = M.fit_R(K, y, np.column_stack([one, x]))
        worst = max(worst, best - M.loglik_R_at(K, y, x, lam))
    print("lambda: model R loses at most %.3e at the tool's lambda (allowed %.1e)" % (worst, LRT_TOL))
    assert worst <= LRT_TOL


ROWS = {5: 400, 63: 400, 64: 400, 65: 400, 67: 400, 241: 600, 1135: 600}


@functools.lru_cache(maxsize=None)
def panel_reference(n, hg):
    """The first 130 varying variants of the fixture and model E's LRT of them (made once per n and hg)."""
    G, K, y = M.fixture(n, ROWS[n], hg)
    V = M.varying(G)[:130]
    assert len(V) == 130
    lrt, l0 = M.lrt_E(K, y, V.astype(np.float64))
    return K, y, V, lrt, l0


@pytest.mark.parametrize("nv", [1, 15, 16, 17, 130])
@pytest.mark.parametrize("n", [5, 63, 64, 65, 67, 241])
def test_panel_widths(n, nv):
    for hg in (0.0, 3.0):
        K, y, V, ref, l0 = panel_reference(n, hg)
        out = run_once(K, y, M.presence_bed(V[:nv]), chunk=64)
        assert out["tested"].all()
        err = np.abs(out["lrt"] - ref[:nv]).max()
        print("n=%d variants=%d hg=%g: max |LRT - model E| = %.3e (allowed %.1e), |l0 - model E| = %.3e"
              % (n, nv, hg, err, LRT_TOL, abs(out["l0"] - l0)))
        assert err <= LRT_TOL
        assert abs(out["l0"] - l0) <= LRT_TOL
        check_p(out)
        check_lambda(K, y, V[:min(nv, 17)].astype(np.float64), out["lam"])
        np.testing.assert_array_equal(out["af"], V[:nv].mean(axis=1))
        assert (out["n_miss"] == 0).all()


@pytest.mark.parametrize("hg", [0.0, 3.0])
def test_real_panel_width(hg):
    n = 1135
    G, K, y = M.fixture(n, ROWS[n], hg)
    V = M.varying(G)[:48]
    ref, l0 = M.lrt_R(K, y, V.astype(np.float64))
    out = run_once(K, y, M.presence_bed(V), chunk=64)
    err = np.abs(out["lrt"] - ref).max()
    print("n=1135 hg=%g: max |LRT - model R| = %.3e (allowed %.1e), |l0 - model R| = %.3e" % (hg, err, LRT_TOL, abs(out["l0"] - l0)))
    assert out["tested"].all() and err <= LRT_TOL and abs(out["l0"] - l0) <= LRT_TOL
    check_p(out)
    check_lambda(K, y, V[:4].astype(np.float64), out["lam"])


def test_genotype_codes_and_filters():
    n = 67
    for hg in (0.0, 3.0):
        G, K, y = M.fixture(n, ROWS[n], hg)
        rng = np.random.default_rng(5)
        D = 2 * M.varying(G)[:16].astype(np.int64)
        D[:12][rng.random((12, n)) < 0.2] = 1    # heterozygous calls
        D[:12][rng.random((12, n)) < 0.05] = -1  # a few missing ones
        D[12] = 2                                # constant
        D[13] = 0
        D[13, :9] = -1                           # constant where it is called
        D[14, rng.permutation(n)[:20]] = -1      # 20 / 67 missing > miss = 0.2
        D[15] = 0
        D[15, :3] = 2                            # af = 3 / 67 < maf = 0.05
        out = run_once(K, y, M.pack_bed(D), chunk=64, maf=0.05, miss=0.2)
        called = D >= 0
        mean = np.where(called, D, 0).sum(axis=1) / np.maximum(called.sum(axis=1), 1)
        exp_tested = np.array([True] * 12 + [False] * 4)
        for v in range(12):  # (the random calls may push one of the first twelve over a filter: say so rather than guess)
            af = mean[v] / 2
            exp_tested[v] = min(af, 1 - af) >= 0.05 and (~called[v]).sum() / n <= 0.2 and len(set(D[v][called[v]])) > 1
        assert exp_tested[:12].sum() >= 10
        assert (out["tested"].astype(bool) == exp_tested).all(), out["tested"]
        assert (out["n_miss"] == (~called).sum(axis=1)).all()
        np.testing.assert_allclose(out["af"], mean / 2, rtol=4e-16, atol=0)
        assert np.isnan(out["lrt"][~exp_tested]).all() and np.isnan(out["p"][~exp_tested]).all()
        X = M.mean_imputed(D[exp_tested])
        ref, _ = M.lrt_E(K, y, X)
        err = np.abs(out["lrt"][exp_tested] - ref).max()
        print("codes hg=%g: max |LRT - model E| = %.3e (allowed %.1e)" % (hg, err, LRT_TOL))
        assert err <= LRT_TOL
        check_p(out, exp_tested)
        # without filters only the constant ones are dropped
        out0 = run_once(K, y, M.pack_bed(D), chunk=64)
        assert list(np.flatnonzero(out0["tested"] == 0)) == [12, 13]


def test_determinism():
    n = 67
    K, y, V, _, _ = panel_reference(n, 3.0)
    bed = M.presence_bed(V)
    a = run_once(K, y, bed, chunk=64)
    assert same_bits(a, run_once(K, y, bed, chunk=64)), "two runs differ"
    assert same_bits(a, run_once(K, y, bed, chunk=4096)), "chunk_variants 64 and 4096 differ"
    perm = np.random.default_rng(3).permutation(len(V))
    b = run_once(K, y, bed[perm], chunk=64)
    assert same_bits({k: v[perm] for k, v in a.items() if k not in ("l0", "lam0")}, b), "a permuted variant order changes a variant's numbers"


def test_shared_kinship():
    n = 67
    K, y, V, _, _ = panel_reference(n, 3.0)
    bed = M.presence_bed(V[:40])
    rng = np.random.default_rng(11)
    ys = [y, rng.permutation(y), M.fixture(n, ROWS[n], 0.0)[2]]
    h = Handle(K, 64)
    shared = []
    for yy in ys:
        o = h.test(bed, yy)
        o["l0"], o["lam0"] = h.null(yy)
        shared.append(o)
    st = capi.LmmStats()
    capi.check(lib.kgwas_lmm_get_stats(h.h, C.byref(st)))
    h.close()
    assert st.eigendecompositions == 1 and st.variants_tested == 120 and st.variants_read == 120
    for yy, o in zip(ys, shared):
        f = run_once(K, yy, bed, chunk=64)
        assert same_bits(o, f) and o["l0"] == f["l0"] and o["lam0"] == f["lam0"]


def test_boundary_optima():
    n = 67
    G, K, y0, = M.fixture(n, ROWS[n], 0.0)
    V = M.varying(G)[:20]
    d, U = np.linalg.eigh(K)
    # no noise: l(lambda) is flat to first order as lambda grows, and the sign of its 1 / lambda term depends on z. This seed is
    # one of those for which l grows up to lmax under H0 and under every variant's H1 (asserted on the models below).
    z = np.random.default_rng(5).standard_normal(n)
    y_max = (U * np.sqrt(np.clip(d, 0, None))) @ z
    one = np.ones(n)
    for y, edge in ((y0, M.LMIN), (y_max, M.LMAX)):
        out = run_once(K, y, M.presence_bed(V), chunk=64)
        _, lam_model = M.fit_R(K, y, one[:, None])
        assert lam_model == pytest.approx(edge, rel=1e-12), "the fixture's null optimum is not at the boundary"
        assert out["lam0"] == edge
        at_edge = np.array([M.fit_R(K, y, np.column_stack([one, x]))[1] == pytest.approx(edge, rel=1e-12) for x in V.astype(np.float64)])
        assert at_edge.sum() >= 10
        assert (out["lam"][at_edge] == edge).all()
        ref, l0 = M.lrt_E(K, y, V.astype(np.float64))
        err = np.abs(out["lrt"] - ref).max()
        print("boundary %.3g: max |LRT - model E| = %.3e (allowed %.1e), %d of %d variants at the boundary" % (edge, err, LRT_TOL, at_edge.sum(), len(V)))
        assert err <= LRT_TOL and abs(out["l0"] - l0) <= LRT_TOL
        check_p(out)


# ---- the command-line tool ----

def _write_plink(tmp_path, name, G, y):
    """G's rows as a .table, then <name>.bed/.bim/.fam through kgwas_write_plink (pass 2 of associate_kmers)."""
    import kmersgwas_amd as kg
    from oracle import oracle_np as onp
    rows, n = G.shape
    names = ["acc%03d" % i for i in range(n)]
    W = (n + 63) // 64
    pad = np.zeros((rows, W * 64), bool)
    pad[:, :n] = G.astype(bool)
    words = np.packbits(pad.reshape(rows, W, 64), axis=2, bitorder="little").view(np.uint64).reshape(rows, W)
    kmers = np.arange(1, rows + 1, dtype=np.uint64) * np.uint64(977)
    base = str(tmp_path / (name + "_table"))
    onp.write_table(base, names, 31, kmers, words)
    t = kg.KmersTable(base, 31)
    out = str(tmp_path / name)
    kg.write_plink(out, t, np.arange(n, dtype=np.uint64), names, y.astype(np.float32), kmers, np.arange(rows, dtype=np.uint64))
    t.close()
    return out


def _fam_y(base, n):
    v, k, cnt = np.zeros(n), np.zeros(n, np.uint8), C.c_uint64()
    capi.check(lib.kgwas_lmm_read_fam((base + ".fam").encode(), 1, n, ptr(v), ptr(k), C.byref(cnt)))
    assert cnt.value == n and k.all()
    return v


def _read_assoc(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and lines[0] == "chr\trs\tps\tn_miss\tallele1\tallele0\taf\tl_mle\tp_lrt"
    return [l.split("\t") for l in lines[1:-1]]


def test_cli(tmp_path):
    n = 67
    G, K, y = M.fixture(n, ROWS[n], 3.0)
    V = G[:60].copy()
    V[3] = 1   # constant: the tool omits it
    V[5] = 0
    V[5, :2] = 1  # af = 2 / 67 < -maf
    kin = str(tmp_path / "pheno.kinship")
    open(kin, "w").write("\n".join("\t".join("%.17g" % v for v in r) for r in K) + "\n")
    rng = np.random.default_rng(8)
    bases = [_write_plink(tmp_path, "P%d" % j, V, yy) for j, yy in enumerate([y, rng.permutation(y), rng.permutation(y)])]
    outdir = str(tmp_path / "out")
    # the pipeline's argument list (kmers_gwas.py:150-165), GEMMA's default search range
    cmd = [BIN, "-bfile", bases[0], "-lmm", "2", "-k", kin, "-outdir", outdir, "-o", "P0", "-maf", "0.05", "-miss", "0.5"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "eigen=" in r.stderr
    rows = _read_assoc(os.path.join(outdir, "P0.assoc.txt"))
    bed = np.frombuffer(open(bases[0] + ".bed", "rb").read(), np.uint8)[3:]
    h = Handle(K, 64, 1e-5, 1e5)
    abi = h.test(bed, _fam_y(bases[0], n), maf=0.05, miss=0.5)
    h.close()
    bim = [l.split("\t") for l in open(bases[0] + ".bim").read().split("\n") if l]
    keep = np.flatnonzero(abi["tested"])
    assert 0 < len(keep) < len(bim) and len(rows) == len(keep)
    for f, v in zip(rows, keep):
        assert len(f) == 9
        assert [f[0], f[1], f[2], f[4], f[5]] == [bim[v][0], bim[v][1], bim[v][3], bim[v][4], bim[v][5]]
        assert f[3] == "0" and f[6] == "%.3f" % abi["af"][v]
        assert float(f[8]) == float("%.6e" % abi["p"][v]) and float(f[7]) == float("%.6e" % abi["lam"][v])
    log = open(os.path.join(outdir, "P0.log.txt")).read()
    assert "individuals_used\t67" in log and "variants_tested\t%d" % len(keep) in log and "lambda0" in log and "logl_H0" in log
    # --bfiles: three files, one eigendecomposition, the outputs of three single runs
    lst = str(tmp_path / "list.txt")
    open(lst, "w").write("".join("%s\tM%d\n" % (b, j) for j, b in enumerate(bases)))
    r = subprocess.run([BIN, "--bfiles", lst, "-lmm", "2", "-k", kin, "-outdir", outdir, "-maf", "0.05", "-miss", "0.5"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "eigendecompositions=1 " in r.stderr, r.stderr
    for j, b in enumerate(bases):
        if j:
            r = subprocess.run([BIN, "-bfile", b, "-lmm", "2", "-k", kin, "-outdir", outdir, "-o", "P%d" % j, "-maf", "0.05", "-miss", "0.5"],
                               capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stderr
        single = open(os.path.join(outdir, "P%d.assoc.txt" % j)).read()
        assert open(os.path.join(outdir, "M%d.assoc.txt" % j)).read() == single and single.count("\n") > 1
    r = subprocess.run([BIN, "-bfile", bases[0], "-lmm", "1", "-k", kin, "-outdir", outdir, "-o", "W"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "only -lmm 2" in r.stderr and not os.path.exists(os.path.join(outdir, "W.assoc.txt"))


def test_python_class():
    import kmersgwas_amd as kg
    n = 67
    K, y, V, ref, l0 = panel_reference(n, 3.0)
    m = kg.LmmLrt(K, lmin=M.LMIN, lmax=M.LMAX, chunk_variants=64)
    r = m.test(M.presence_bed(V[:17]).tobytes(), y)
    assert np.abs(r["lrt"] - ref[:17]).max() <= LRT_TOL and abs(m.null(y)[0] - l0) <= LRT_TOL and r["tested"].all()
    assert m.stats()["variants_tested"] == 17
    m.close()
