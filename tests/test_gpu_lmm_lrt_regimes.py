"""lmm_lrt on the GPU in the regimes its first two modules never reach: strong associations (LRT up to 4700, p down to 0), a
likelihood with two interior maxima, individuals dropped for a missing phenotype, and a few smaller edges (the genotype codes at
n = 241 and 1135, the tool's default search range, the filters at equality, the unit of y).

The fixtures are lmm_lrt_np.py's; what each of them is for (LRT > 100, two peaks and which one wins, what the filters say about
the kept individuals) and the gap between the two models on it (<= 1e-10) are asserted without a GPU in test_lmm_lrt_model.py.
The tolerances are test_gpu_lmm_lrt.py's, imported: LRT and l0 within LRT_TOL of a model, p within P_RTOL of chi2.sf(LRT_tool, 1),
lambda through the likelihood. Model E is the reference up to n = 241, model R at n = 1135.

Largest deviations measured on the MI355X (each test prints its own; DESIGN.md 4.12 has them all): LRT within 6.1e-11 of model E
(n = 241, LRT 1760) and 7.1e-11 of model R (n = 1135, LRT 4720) under strong effects, 5.3e-11 on the two-peaked fixtures, 3.6e-12
elsewhere; l0 within 3.3e-11; model R loses at most 4.5e-13 at the tool's lambda; p within 5.5e-14 of chi2.sf, relative.
"""
import functools
import os
import subprocess

import numpy as np
import pytest
from scipy.stats import chi2

import lmm_lrt_np as M
from test_gpu_lmm_lrt import BIN, LRT_TOL, P_RTOL, Handle, _read_assoc, check_lambda, check_p, run_once, same_bits
from test_gpu_lmm_lrt_multi import multi

pytestmark = pytest.mark.gpu

TINY = 2.3e-308  # below it chi2.sf is subnormal or 0, and a relative error says nothing
EPS = 2.0 ** -52


def check_p_to_zero(out, expect_underflow):
    """check_p where chi2.sf(LRT, 1) is a normal double; 0 <= p <= TINY (so: not NaN) where it is not"""
    normal = chi2.sf(out["lrt"], 1) >= TINY
    check_p(out, normal)
    rest = out["p"][~normal]
    print("p: %d of %d variants below the normal doubles: %s" % (len(rest), len(normal), rest))
    assert ((rest >= 0) & (rest <= TINY)).all()
    assert (len(rest) > 0) == expect_underflow


def column_of(m, c, single):
    """column c of a multi call's outputs, as a single call's"""
    assert m["l0"][c] == single["l0"] and m["lam0"][c] == single["lam0"]
    return dict(lrt=m["lrt"][c], lam=m["lam"][c], p=m["p"][c], af=m["af"], n_miss=m["n_miss"], tested=m["tested"])


def check_multi(K, Y, bed, singles):
    h = Handle(K, 64)
    try:
        m = multi(h, Y, bed)
    finally:
        h.close()
    for c, s in enumerate(singles):
        assert same_bits(column_of(m, c, s), s), "column %d of the multi pass differs from the single call" % c


def check_against(name, out, ref, l0, sel=slice(None)):
    err = np.abs(out["lrt"][sel] - ref).max()
    print("%s: max |LRT - model| = %.3e, |l0 - model| = %.3e (allowed %.1e), LRT up to %.4g" % (name, err, abs(out["l0"] - l0), LRT_TOL, ref.max()))
    assert err <= LRT_TOL and abs(out["l0"] - l0) <= LRT_TOL


def check_lambda0(K, y, lam0, lmin=M.LMIN, lmax=M.LMAX):
    best, _ = M.fit_R(K, y, np.ones((y.size, 1)), lmin, lmax)
    loss = best - M.loglik_R_at(K, y, None, lam0)
    print("lambda0: model R loses %.3e at the tool's lambda0 (allowed %.1e)" % (loss, LRT_TOL))
    assert loss <= LRT_TOL


# ---- 1. strong associations ----

@functools.lru_cache(maxsize=None)
def strong_reference(n, effect):
    K, base, g, V = M.strong_fixture(n, M.STRONG_ROWS[n], nv=16 if n == 1135 else 20)
    y = base + effect * g
    ref, l0 = (M.lrt_R if n == 1135 else M.lrt_E)(K, y, V.astype(np.float64))
    assert ref.max() > 100 and ref.argmax() == 0
    return K, y, V, ref, l0


@pytest.mark.parametrize("n", [67, 241])
def test_strong_associations(n):
    singles = []
    for effect in M.STRONG_EFFECTS:
        K, y, V, ref, l0 = strong_reference(n, effect)
        out = run_once(K, y, M.presence_bed(V))
        assert out["tested"].all()
        check_against("strong n=%d effect=%g" % (n, effect), out, ref, l0)
        check_p_to_zero(out, expect_underflow=(n, effect) == (241, 40.0))  # LRT = 1760 there
        check_lambda(K, y, V[:8].astype(np.float64), out["lam"])
        singles.append(out)
    check_multi(K, np.stack([strong_reference(n, e)[1] for e in M.STRONG_EFFECTS]), M.presence_bed(V), singles)


def test_strong_associations_real_panel_width():
    n = 1135
    K, y, V, ref, l0 = strong_reference(n, 10.0)
    _, base, g, _ = M.strong_fixture(n, M.STRONG_ROWS[n], nv=16)
    bed = M.presence_bed(V)
    h = Handle(K, 64)
    try:
        singles = []
        for effect in M.STRONG_EFFECTS:
            o = h.test(bed, base + effect * g)
            o["l0"], o["lam0"] = h.null(base + effect * g)
            singles.append(o)
        m = multi(h, np.stack([base + e * g for e in M.STRONG_EFFECTS]), bed)
    finally:
        h.close()
    out = singles[1]
    assert out["tested"].all() and (y == base + 10.0 * g).all()
    check_against("strong n=1135 effect=10", out, ref, l0)
    check_p_to_zero(out, expect_underflow=True)  # LRT = 4720
    check_lambda(K, y, V[:4].astype(np.float64), out["lam"])
    for c, s in enumerate(singles):
        assert same_bits(column_of(m, c, s), s), "column %d of the multi pass differs from the single call" % c


# ---- 2. two interior maxima ----

@functools.lru_cache(maxsize=None)
def two_peak_reference(n, seed):
    K, y, X = M.two_peak_fixture(n, seed, M.two_peak_rows(n))
    ref, l0 = M.lrt_E(K, y, X.astype(np.float64))
    return K, y, X, ref, l0


@pytest.mark.parametrize("n,seed", M.TWO_PEAK_CASES)
def test_two_interior_maxima(n, seed):
    """check_lambda is what fails if the refinement returns the wrong peak: model R would lose the peaks' difference in l
    (0.05 .. 42 over these fixtures) at the tool's lambda, not 1e-12."""
    K, y, X, ref, l0 = two_peak_reference(n, seed)
    assert len(X) > (32 if n <= 16 else 15)
    bed = M.presence_bed(X)
    out = run_once(K, y, bed)
    assert out["tested"].all()
    check_against("two-peak n=%d seed=%d (%d variants)" % (n, seed, len(X)), out, ref, l0)
    check_lambda(K, y, X.astype(np.float64), out["lam"])
    check_lambda0(K, y, out["lam0"])
    check_p(out)
    rng = np.random.default_rng([seed, n, 8])
    Y = np.stack([y, rng.permutation(y), rng.permutation(y)])
    check_multi(K, Y, bed, [out] + [run_once(K, yy, bed) for yy in Y[1:]])


# ---- 3. individuals without a phenotype, against a computation that never sees the file layer ----

MAF = MISS = 0.05
DEFAULT_RANGE = (1e-5, 1e5)  # the tool's, GEMMA's


def _write_dropped(tmp_path):
    K, D, pheno = M.dropped_panel()
    base = str(tmp_path / "panel")
    open(base + ".bed", "wb").write(bytes([0x6C, 0x1B, 0x01]) + M.pack_bed(D).tobytes())
    open(base + ".bim", "w").write("".join("%d\trs%d\t0\t%d\tA\tC\n" % (1 + v % 5, v, 100 + v) for v in range(len(D))))
    open(base + ".fam", "w").write("".join("f%d i%d 0 0 0 %s\n" % (i, i, " ".join(("-9", "NA")[(i + c) % 2] if np.isnan(x) else "%.17g" % x
                                                                                  for c, x in enumerate(row))) for i, row in enumerate(pheno)))
    kin = str(tmp_path / "pheno.kinship")
    open(kin, "w").write("\n".join("\t".join("%.17g" % v for v in r) for r in K) + "\n")
    return base, kin


@functools.lru_cache(maxsize=None)
def dropped_reference(col):
    """What the tool must say of phenotype column col (1-based), from K[keep][:, keep], the kept columns of the dosages and model E."""
    K, D, pheno = M.dropped_panel()
    keep = np.flatnonzero(~np.isnan(pheno[:, col - 1]))
    Ds = D[:, keep]
    t = M.expect_tested(Ds, MAF, MISS)
    af, n_miss, _ = M.call_stats(Ds)
    Ks, y = np.ascontiguousarray(K[np.ix_(keep, keep)]), pheno[keep, col - 1]
    ref, l0 = M.lrt_E(Ks, y, M.mean_imputed(Ds[t]), *DEFAULT_RANGE)
    return Ks, y, Ds, t, af, n_miss, ref, l0


def _p_bounds(lrt):
    """The p_lrt field of a variant whose model LRT is lrt. The tool's LRT is within LRT_TOL of it and chi2.sf falls with LRT, so the
    tool's chi2.sf lies between those of lrt + LRT_TOL and lrt - LRT_TOL (for a large LRT that is dp / p = LRT_TOL / 2; taking the
    two ends holds for a small one too, where dp / dLRT grows like LRT^-1/2). Its p is within P_RTOL of that, and '%.6e' rounds by
    at most half a unit of the sixth decimal of a mantissa >= 1: 5e-7, relative."""
    r = 5e-7 + P_RTOL
    return chi2.sf(lrt + LRT_TOL, 1) * (1 - r), chi2.sf(max(0.0, lrt - LRT_TOL), 1) * (1 + r)


def test_dropped_individuals_cli(tmp_path):
    base, kin = _write_dropped(tmp_path)
    outdir = str(tmp_path / "out")
    common = ["-lmm", "2", "-k", kin, "-outdir", outdir, "-maf", str(MAF), "-miss", str(MISS), "--chunk_variants", "64"]
    for col in (1, 2, 3, 4):
        Ks, y, Ds, t, af, n_miss, ref, l0 = dropped_reference(col)
        kept = 63 if col == 2 else 64
        assert len(y) == kept
        r = subprocess.run([BIN, "-bfile", base, "-n", str(col), "-o", "S%d" % col] + common, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        rows = _read_assoc(os.path.join(outdir, "S%d.assoc.txt" % col))
        assert [f[1] for f in rows] == ["rs%d" % v for v in np.flatnonzero(t)], "the tested set is not that of the kept individuals"
        worst = 0.0
        for f, v, lrt in zip(rows, np.flatnonzero(t), ref):
            assert f[3] == "%d" % n_miss[v] and f[6] == "%.3f" % af[v], (v, f)
            lo, hi = _p_bounds(lrt)
            assert lo <= float(f[8]) <= hi, (v, f[8], "%.6e" % chi2.sf(lrt, 1))
            worst = max(worst, abs(float(f[8]) / chi2.sf(lrt, 1) - 1))
        log = open(os.path.join(outdir, "S%d.log.txt" % col)).read().split("\n")
        assert log[3] == "individuals_in_fam\t70" and log[4] == "individuals_used\t%d" % kept and log[6] == "variants_tested\t%d" % t.sum()
        assert log[8].startswith("logl_H0\t") and abs(float(log[8].split("\t")[1]) - l0) <= 5e-7 + LRT_TOL
        print("column %d, %d kept, %d tested: p_lrt of the file within %.2e of chi2.sf(LRT of model E) (printed to 7 digits)" % (col, kept, t.sum(), worst))
    # the C ABI on the subset gives the numbers of the file, and the model's
    for col in (1, 2):
        Ks, y, Ds, t, af, n_miss, ref, l0 = dropped_reference(col)
        h = Handle(Ks, 64, *DEFAULT_RANGE)
        try:
            abi = h.test(M.pack_bed(Ds), y, maf=MAF, miss=MISS)
            abi["l0"], _ = h.null(y)
        finally:
            h.close()
        assert (abi["tested"].astype(bool) == t).all() and (abi["n_miss"] == n_miss).all() and (abi["af"] == af).all()
        check_against("dropped individuals, column %d, C ABI on the subset" % col, abi, ref, l0, t)
        rows = _read_assoc(os.path.join(outdir, "S%d.assoc.txt" % col))
        for f, v in zip(rows, np.flatnonzero(t)):
            assert float(f[8]) == float("%.6e" % abi["p"][v]) and float(f[7]) == float("%.6e" % abi["lam"][v])
    # --columns over the columns that share a missing set: the files of the single runs, which are anchored to the model above
    lst = str(tmp_path / "columns.txt")
    open(lst, "w").write("".join("%d\tC%d\n" % (c, c) for c in (1, 3, 4)))
    r = subprocess.run([BIN, "-bfile", base, "--columns", lst] + common, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "individuals=64 " in r.stderr, r.stderr
    for c in (1, 3, 4):
        single = open(os.path.join(outdir, "S%d.assoc.txt" % c), "rb").read()
        assert open(os.path.join(outdir, "C%d.assoc.txt" % c), "rb").read() == single
        log_m, log_s = (open(os.path.join(outdir, "%s%d.log.txt" % (x, c))).read().split("\n") for x in "CS")
        assert log_m[:9] == log_s[:9]


# ---- 4. smaller edges ----

@pytest.mark.parametrize("n,nv", [(241, 24), (1135, 12)])
def test_genotype_codes_at_other_widths(n, nv):
    K, y, D = M.codes_panel(n, 600, nv)
    af, n_miss, constant = M.call_stats(D)
    assert not constant.any() and n_miss[nv - 2] == 1 and D[nv - 2, n - 1] == -1 and af[nv - 1] == 0.5 * (2 / n)
    ref, l0 = (M.lrt_R if n == 1135 else M.lrt_E)(K, y, M.mean_imputed(D))
    out = run_once(K, y, M.pack_bed(D))
    assert out["tested"].all()
    np.testing.assert_array_equal(out["af"], af)
    np.testing.assert_array_equal(out["n_miss"], n_miss)
    check_against("codes n=%d" % n, out, ref, l0)
    check_p(out)


def test_default_search_range():
    n = 67
    lmin, lmax = DEFAULT_RANGE
    one = np.ones(n)
    for hg in (0.0, 3.0):
        G, K, y = M.fixture(n, 400, hg)
        V = M.varying(G)[:24]
        ref, l0 = M.lrt_E(K, y, V.astype(np.float64), lmin, lmax)
        h = Handle(K, 64, lmin, lmax)
        try:
            out = h.test(M.presence_bed(V), y)
            out["l0"], out["lam0"] = h.null(y)
        finally:
            h.close()
        assert out["tested"].all()
        check_against("default range hg=%g" % hg, out, ref, l0)
        check_p(out)
        check_lambda0(K, y, out["lam0"], lmin, lmax)
        worst = max(M.fit_R(K, y, np.column_stack([one, x]), lmin, lmax)[0] - M.loglik_R_at(K, y, x, lam)
                    for x, lam in zip(V[:8].astype(np.float64), out["lam"]))
        print("lambda: model R loses at most %.3e at the tool's lambda (allowed %.1e)" % (worst, LRT_TOL))
        assert worst <= LRT_TOL
        if hg == 0.0:  # no heritable part: the null optimum is the lower end, returned exactly
            assert out["lam0"] == 1e-5


@pytest.mark.parametrize("n,maf,miss,edge", [(20, 0.05, 1.0, [1, 1, 1, 0]), (21, 0.05, 1.0, [0, 1, 1, 0]), (5, 0.0, 0.2, [1, 1, 0, 0])])
def test_filters_at_equality(n, maf, miss, edge):
    """af = 1 / 20 against -maf 0.05 and 1 / 5 missing against -miss 0.2 are kept (>=, <=); 1 / 21 and 2 / 5 are not; a variant
    called in one individual is constant. edge: whether rows 6..9 of filter_edge_panel are tested."""
    K, y, D = M.filter_edge_panel(n)
    t = M.expect_tested(D, maf, miss)
    assert list(t[6:]) == [bool(e) for e in edge]
    af, n_miss, _ = M.call_stats(D)
    if n == 20:
        assert af[6] == 0.05 == maf
    if n == 5:
        assert n_miss[7] / n == 0.2 == miss
    out = run_once(K, y, M.pack_bed(D), maf=maf, miss=miss)
    assert (out["tested"].astype(bool) == t).all(), out["tested"]
    np.testing.assert_array_equal(out["af"], af)
    np.testing.assert_array_equal(out["n_miss"], n_miss)
    assert n_miss[9] == n - 1 and all(np.isnan(out[k][~t]).all() for k in ("lrt", "lam", "p"))
    ref, l0 = M.lrt_E(K, y, M.mean_imputed(D[t]))
    check_against("filter edges n=%d" % n, out, ref, l0, t)
    check_p(out, t)


@pytest.mark.parametrize("kind", ["strong", "two-peak"])
def test_unit_of_y(kind):
    """y in another unit, 2^20 or 2^-20 times as large: the LRT is the model's of the unscaled y (the models are scale-free, so one
    reference serves), and l0 moves by -n log s. l0 there is about n 20 log 2 = 930 .. 220 in size; the tool takes it from a log, a
    product and two sums at that size, each rounded to half an ulp, so the comparison after the shift is allowed LRT_TOL plus 16 ulps
    of |l0| (3e-12), not a bound relative to l0."""
    K, y, V, ref, l0 = strong_reference(67, 10.0) if kind == "strong" else two_peak_reference(16, 69)
    bed = M.presence_bed(V)
    n = y.size
    for s in (2.0 ** 20, 2.0 ** -20):
        out = run_once(K, y * s, bed)
        err = np.abs(out["lrt"] - ref).max()
        shifted = out["l0"] + n * np.log(s)
        bound = LRT_TOL + 16 * EPS * abs(out["l0"])
        print("%s, y x %g: max |LRT - model of y| = %.3e (allowed %.1e), |l0 + n log s - model| = %.3e (allowed %.3e)"
              % (kind, s, err, LRT_TOL, abs(shifted - l0), bound))
        assert out["tested"].all() and err <= LRT_TOL and abs(shifted - l0) <= bound
        check_lambda(K, y, V[:8].astype(np.float64), out["lam"])
