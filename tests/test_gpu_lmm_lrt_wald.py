"""lmm_lrt -lmm 4 on the GPU, through the C ABI and the tool: beta, se, the Wald and the score test and the REML null model against
the numpy models of lmm_wald_np.py, the bits the -lmm 2 outputs keep, determinism, filters and the 14-column file.

Tolerances (-lmin / -lmax = e^-10 / e^10 throughout; test_lmm_wald_model.py measures the gaps between the models without a GPU):
  beta, se, F   against model G (model R' at n = 1135) AT THE TOOL'S OWN l_remle and lambda0, so that the location error of a flat
                optimum does not enter: 1000 x the models' gap at fixed lambdas, capped at 1e-8, relative. F_wald is recovered as
                (beta / se)^2. The tool has no F_score output: p_score is compared with the tail of the model's F_score at the tool's
                lambda0, allowed P_RTOL plus F_TOL times |d log Q / d log F| there; and where l_remle == lambda0 to the bit (a
                phenotype without a heritable part) the tool's own F_score is n F_wald / (df + F_wald), and P_RTOL alone holds.
  l_remle       through the likelihood: model R''s REML value at the tool's l_remle within REML_TOL (1000 x the gap, cap 1e-8,
                absolute) of model R''s own maximum. On a two-peaked fixture a wrong peak loses 0.05 .. 42.
  p_wald        against 2 t.sf(sqrt(F), df) of the tool's own F: 10 x MEASURED_P_RELERR, cap 1e-9; 0 <= p <= 2.3e-308 where the
                reference is no normal double.
  vg, ve        against the restatement of emma.REMLE at the tool's lambda0_remle: 1000 x MEASURED_VG_VE_GAP.

Largest deviations measured on the MI355X (each test prints its own; DESIGN.md 4.12 has them too): against model G up to n = 241,
beta within 9.4e-12, se within 3.6e-13, F_wald within 1.9e-11; against model R' at n = 1135, 1.1e-10, 4.9e-13 and 2.3e-10. Model R'
loses at most 4.5e-13 at the tool's l_remle (n = 1135), 5.7e-14 on the two-peaked fixtures, where the wrong peak would lose 0.05 .. 42.
p_wald within 1.1e-13 of the tail of the tool's own F; p_score within 6.2e-15 where the tool's own F_score is known, within 7.5e-11 of
the tail of the model's F_score elsewhere (allowed 2.8e-6 there: F_TOL times the tail's slope). The REML null model: the tool's value
within 3.3e-11 of model R' at its lambda (n = 1135; 1.7e-13 up to n = 241), vg and ve within 1.9e-14 of emma.REMLE's.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
from scipy.stats import t as student_t

from kmersgwas_amd import capi
from kmersgwas_amd.capi import lib, ptr

import lmm_lrt_np as M
import lmm_wald_np as W
from test_gpu_lmm_lrt import BIN, ROWS, Handle, _fam_y, _write_plink
from test_lmm_wald_model import MEASURED_BETA_GAP, MEASURED_F_GAP, MEASURED_REML_GAP, MEASURED_SE_GAP, MEASURED_VG_VE_GAP

pytestmark = pytest.mark.gpu

BETA_TOL = min(1e-8, 1000 * MEASURED_BETA_GAP)
SE_TOL = min(1e-8, 1000 * MEASURED_SE_GAP)
F_TOL = min(1e-8, 1000 * MEASURED_F_GAP)
REML_TOL = min(1e-8, 1000 * MEASURED_REML_GAP)
VG_VE_TOL = min(1e-8, 1000 * MEASURED_VG_VE_GAP)
MEASURED_P_RELERR = 1.1e-13  # largest |p_wald / (2 t.sf(sqrt(F), df)) - 1| seen on the MI355X over this module (strong, n = 241, effect 10)
P_RTOL = min(1e-9, 10 * MEASURED_P_RELERR)
TINY = 2.3e-308
STATS = ("lrt", "lam", "p", "beta", "se", "lam_remle", "p_wald", "p_score")
ALL = STATS + ("af", "n_miss", "tested")


class Handle4(Handle):
    def test_all(self, bed, y, maf=0.0, miss=1.0):
        bed = np.ascontiguousarray(bed, np.uint8)
        m = bed.size // ((self.n + 3) // 4)
        out = {k: np.zeros(m) for k in STATS + ("af",)}
        out["n_miss"], out["tested"] = np.zeros(m, np.uint32), np.zeros(m, np.uint8)
        capi.check(lib.kgwas_lmm_test_bed_all(self.h, ptr(np.ascontiguousarray(y, np.float64)), ptr(bed), m, maf, miss, ptr(out["lrt"]), ptr(out["lam"]),
                                              ptr(out["p"]), ptr(out["beta"]), ptr(out["se"]), ptr(out["lam_remle"]), ptr(out["p_wald"]),
                                              ptr(out["p_score"]), ptr(out["af"]), ptr(out["n_miss"]), ptr(out["tested"])))
        return out

    def null_reml(self, y):
        v = [C.c_double() for _ in range(4)]
        capi.check(lib.kgwas_lmm_null_reml(self.h, ptr(np.ascontiguousarray(y, np.float64)), *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)  # lR0, lambda0_remle, vg, ve


def run_all(K, y, bed, chunk=64, lmin=M.LMIN, lmax=M.LMAX, **kw):
    h = Handle4(K, chunk, lmin, lmax)
    try:
        out = h.test_all(bed, y, **kw)
        out["l0"], out["lam0"] = h.null(y)
        out["null_reml"] = h.null_reml(y)
    finally:
        h.close()
    return out


def same_bits(a, b, keys=ALL):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in keys)


def tail_ref(F, df):
    return 2.0 * student_t.sf(np.sqrt(F), df)


def check_tail(name, p, F, df, extra=0.0):
    """p against the t-tail of F where that is a normal double (relative, P_RTOL + extra), 0 <= p <= TINY where it is not"""
    ref = tail_ref(F, df)
    normal = ref >= TINY
    rel = np.abs(p[normal] / ref[normal] - 1.0)
    allowed = P_RTOL + (extra[normal] if np.ndim(extra) else extra)
    print("%s: largest relative error against the t tail %.3e (allowed %.1e), %d of %d below the normal doubles"
          % (name, rel.max() if rel.size else 0.0, np.max(allowed) if rel.size else P_RTOL, (~normal).sum(), len(normal)))
    assert (rel <= allowed).all()
    assert ((p[~normal] >= 0) & (p[~normal] <= TINY)).all()
    return int((~normal).sum())


def tail_sensitivity(F, df):
    """|d log Q / d log F| of the reference, by a central difference"""
    e = 1e-6
    hi, lo = tail_ref(F * (1 + e), df), tail_ref(F * (1 - e), df)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.abs(np.log(hi) - np.log(lo)) / (2 * e)
    return np.where(np.isfinite(s), s, 0.0)


def check_reml_loss(name, K, y, xs, lams):
    worst = 0.0
    for x, lam in zip(xs, lams):
        best, _ = W.fit_reml_R(K, y, x)
        worst = max(worst, best - W.reml_R_at(K, y, x, lam))
    print("%s: model R' loses at most %.3e at the tool's l_remle (allowed %.1e)" % (name, worst, REML_TOL))
    assert worst <= REML_TOL
    return worst


def check_null_reml(name, K, y, out):
    lR0, lam, vg, ve = out["null_reml"]
    best, _ = W.fit_reml_R(K, y, None)
    at_tool = W.reml_R_at(K, y, None, lam)
    evg, eve = W.emma_vg_ve(K, y, lam)
    gap = max(abs(vg / evg - 1), abs(ve / eve - 1))
    print("%s: null by REML: model R' loses %.3e at lambda0_remle = %.6g and differs by %.3e from the tool's value (allowed %.1e); vg, ve within "
          "%.3e of emma.REMLE's (allowed %.1e)" % (name, best - at_tool, lam, abs(lR0 - at_tool), REML_TOL, gap, VG_VE_TOL))
    assert best - at_tool <= REML_TOL and abs(lR0 - at_tool) <= REML_TOL and gap <= VG_VE_TOL
    assert vg == lam * ve


def check_statistics(name, K, y, X, out, sel=None, model="G"):
    """beta, se, F_wald = (beta / se)^2 and p_score against the model at the tool's own l_remle and lambda0; p_wald against the tail"""
    n = y.size
    df = n - 2
    idx = np.arange(len(X)) if sel is None else np.flatnonzero(sel)
    gb = gs = gF = gFs = 0.0
    Fs_model = np.zeros(len(idx))
    for k, v in enumerate(idx):
        if model == "G":
            b, s, F, _ = W.gls_G(K, y, X[k], out["lam_remle"][v])
            Fs_model[k] = W.score_G(K, y, X[k], out["lam0"])
        else:
            b, s, F = W.wald_R(K, y, X[k], out["lam_remle"][v])
            Fs_model[k] = W.score_R(K, y, X[k], out["lam0"])
        gb, gs = max(gb, abs(out["beta"][v] / b - 1)), max(gs, abs(out["se"][v] / s - 1))
        gF = max(gF, abs((out["beta"][v] / out["se"][v]) ** 2 / F - 1))
    print("%s: beta within %.3e (allowed %.1e), se within %.3e (allowed %.1e), F_wald within %.3e (allowed %.1e) of model %s, relative"
          % (name, gb, BETA_TOL, gs, SE_TOL, gF, F_TOL, model))
    assert gb <= BETA_TOL and gs <= SE_TOL and gF <= F_TOL
    Fw = (out["beta"][idx] / out["se"][idx]) ** 2
    below = check_tail(name + ", p_wald", out["p_wald"][idx], Fw, df)
    below += check_tail(name + ", p_score", out["p_score"][idx], Fs_model, df, extra=F_TOL * tail_sensitivity(Fs_model, df))
    assert (Fs_model < n).all()  # (F_score = n r^2)
    return below


# ---- 1. against the models ----

@pytest.mark.parametrize("nv", [17, 130])
@pytest.mark.parametrize("n", [5, 67, 241])
def test_against_models(n, nv):
    for hg in ((0.0, 3.0) if nv == 17 else (3.0,)):
        G, K, y = M.fixture(n, ROWS[n], hg)
        V = M.varying(G)[:nv]
        assert len(V) == nv
        X = 2.0 * V  # the dosages presence_bed's codes decode to
        out = run_all(K, y, M.presence_bed(V))
        name = "n=%d variants=%d hg=%g" % (n, nv, hg)
        assert out["tested"].all() and np.isfinite(np.stack([out[k] for k in STATS])).all()
        check_statistics(name, K, y, X, out)
        check_reml_loss(name, K, y, X[:17], out["lam_remle"])
        check_null_reml(name, K, y, out)
        assert (out["se"] > 0).all() and (out["lam_remle"] >= M.LMIN).all() and (out["lam_remle"] <= M.LMAX).all()


@pytest.mark.parametrize("n", [67, 241])
def test_strong_effects(n):
    """effect 40 at n = 241: F_wald is past 1e4 and p_wald below the normal doubles"""
    K, base, g, V = M.strong_fixture(n, M.STRONG_ROWS[n])
    X = 2.0 * V
    for effect in M.STRONG_EFFECTS:
        y = base + effect * g
        out = run_all(K, y, M.presence_bed(V))
        name = "strong n=%d effect=%g" % (n, effect)
        assert out["tested"].all()
        below = check_statistics(name, K, y, X, out)
        check_reml_loss(name, K, y, X[:4], out["lam_remle"])
        assert out["beta"][0] == pytest.approx(effect / 2, rel=0.2)  # (per unit of the dosage: presence is 2)
        if (n, effect) == (241, 40.0):
            assert below > 0


def test_real_panel_width():
    n = 1135
    K, base, g, V = M.strong_fixture(n, M.STRONG_ROWS[n], nv=20)
    y = base + 10.0 * g
    X = 2.0 * V
    out = run_all(K, y, M.presence_bed(V))
    assert out["tested"].all()
    check_statistics("strong n=1135 effect=10", K, y, X, out, model="R'")
    check_reml_loss("strong n=1135 effect=10", K, y, X[:4], out["lam_remle"])
    check_null_reml("strong n=1135 effect=10", K, y, out)


def test_score_tail_where_l_remle_is_lambda0():
    """Without a heritable part both lambdas are the lower end, to the bit, for most variants: the Wald and the score statistic then
    come from the same sums, F_score = n F_wald / (df + F_wald), and p_score is checked against the tool's own F."""
    n = 67
    G, K, _ = M.fixture(n, ROWS[n], 0.0)
    y = W.noise_phenotype(n)
    V = M.varying(G)[:130]
    out = run_all(K, y, M.presence_bed(V))
    assert out["lam0"] == M.LMIN and out["null_reml"][1] == M.LMIN, "lambda0_remle is not lmin exactly"
    same = out["lam_remle"] == out["lam0"]
    assert same.sum() >= 65, same.sum()
    Fw = (out["beta"][same] / out["se"][same]) ** 2
    check_tail("p_score at l_remle == lambda0 (%d variants)" % same.sum(), out["p_score"][same], n * Fw / (n - 2 + Fw), n - 2)
    check_null_reml("noise n=67", K, y, out)
    vg, ve = out["null_reml"][2:]
    assert vg == M.LMIN * ve and ve == pytest.approx(np.var(y, ddof=1), rel=1e-2)


# ---- 2. two REML peaks ----

@pytest.mark.parametrize("n,seed", [(8, 36), (67, 56), (8, 18), (67, 54)])
def test_two_reml_peaks(n, seed):
    """test_lmm_wald_model.py asserts that these fixtures have models with two interior REML maxima (all of (67, 56)'s and (67, 54)'s,
    all but one of (8, 36)'s, 12 of (8, 18)'s). Had the refinement returned the wrong peak, model R' would lose the peaks' difference."""
    K, y, X = M.two_peak_fixture(n, seed, M.two_peak_rows(n))
    out = run_all(K, y, M.presence_bed(X))
    assert out["tested"].all()
    xs = X.astype(np.float64)
    two = sum(len(W.interior_reml_maxima(K, y, x)) == 2 for x in xs)
    assert two >= {(8, 36): 63, (8, 18): 8}.get((n, seed), 16)
    worst = check_reml_loss("two-peak n=%d seed=%d (%d variants)" % (n, seed, len(xs)), K, y, xs, out["lam_remle"])
    lR0, lam, _, _ = out["null_reml"]
    loss0 = W.fit_reml_R(K, y, None)[0] - W.reml_R_at(K, y, None, lam)
    print("worst REML loss %.3e over the variants, %.3e under H0" % (worst, loss0))
    assert loss0 <= REML_TOL


# ---- 3. bits ----

def test_lmm2_outputs_keep_their_bits_and_all_are_deterministic():
    n = 67
    K, y, D = M.codes_panel(n, ROWS[n], 130)
    bed = M.pack_bed(D)
    kw = dict(maf=0.05, miss=0.05)
    a = run_all(K, y, bed, chunk=64, **kw)
    assert 20 <= a["tested"].sum() < len(D)
    h = Handle(K, 64)
    try:
        two = h.test(bed, y, **kw)
    finally:
        h.close()
    assert same_bits(a, two, ("lrt", "lam", "p", "af", "n_miss", "tested")), "lrt, lambda_mle, p_lrt, af, n_miss or tested differ from kgwas_lmm_test_bed's"
    assert same_bits(a, run_all(K, y, bed, chunk=64, **kw)), "two runs differ"
    for chunk in (32, 10240):
        assert same_bits(a, run_all(K, y, bed, chunk=chunk, **kw)), "chunk_variants 64 and %d differ" % chunk
    perm = np.random.default_rng(3).permutation(len(D))
    b = run_all(K, y, bed[perm], chunk=64, **kw)
    assert same_bits({k: a[k][perm] for k in ALL}, b), "a permuted variant order changes a variant's numbers"
    assert a["null_reml"] == b["null_reml"] and (a["l0"], a["lam0"]) == (b["l0"], b["lam0"])


def test_null_pointers_and_cached_phenotype():
    n = 67
    G, K, y = M.fixture(n, ROWS[n], 3.0)
    bed = M.presence_bed(M.varying(G)[:17])
    h = Handle4(K, 64)
    try:
        full = h.test_all(bed, y)
        beta = np.zeros(17)
        capi.check(lib.kgwas_lmm_test_bed_all(h.h, ptr(y), ptr(bed), 17, 0.0, 1.0, None, None, None, ptr(beta), None, None, None, None, None, None, None))
        assert beta.tobytes() == full["beta"].tobytes()
        capi.check(lib.kgwas_lmm_null_reml(h.h, ptr(y), None, None, None, None))
        first = h.null_reml(y)
        y2 = np.random.default_rng(4).permutation(y)
        other = h.null_reml(y2)
        assert other != first and h.null_reml(y) == first and h.null(y2) != h.null(y)
        assert lib.kgwas_lmm_null_reml(h.h, None, None, None, None, None) == capi.KGWAS_ERR_ARG
    finally:
        h.close()
    # the Python class gives the same numbers
    import kmersgwas_amd as kg
    m = kg.LmmLrt(K, lmin=M.LMIN, lmax=M.LMAX, chunk_variants=64)
    r = m.test_all(bed.tobytes(), y)
    assert all(r[a].tobytes() == full[b].tobytes() for a, b in (("beta", "beta"), ("se", "se"), ("lambda_remle", "lam_remle"), ("p_wald", "p_wald"),
                                                                ("p_score", "p_score"), ("lrt", "lrt"), ("lambda", "lam"), ("p", "p")))
    assert m.null_reml(y) == first and r["tested"].all()
    m.close()


# ---- 4. filters and missing calls ----

def test_filters_and_missing_calls():
    n = 241
    K, y, D = M.codes_panel(n, 600, 24)
    t = M.expect_tested(D, 0.05, 0.05)
    assert 4 <= t.sum() < len(D)
    out = run_all(K, y, M.pack_bed(D), maf=0.05, miss=0.05)
    assert (out["tested"].astype(bool) == t).all()
    for k in STATS:
        assert np.isnan(out[k][~t]).all() and np.isfinite(out[k][t]).all(), k
    af, n_miss, _ = M.call_stats(D)
    np.testing.assert_array_equal(out["af"], af)
    np.testing.assert_array_equal(out["n_miss"], n_miss)
    assert n_miss[t].max() > 0
    check_statistics("codes n=241, mean-imputed calls", K, y, M.mean_imputed(D[t]), out, sel=t)


# ---- 5. the tool ----

NEW_LOG_LINES = ("lambda0_remle", "logl_remle_H0", "vg", "ve")
HEADER4 = "chr\trs\tps\tn_miss\tallele1\tallele0\taf\tbeta\tse\tl_remle\tl_mle\tp_wald\tp_lrt\tp_score"


def _read(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == ""
    return lines[0], [l.split("\t") for l in lines[1:-1]]


def _log_keys(path):
    return [l.split("\t")[0].split(" ")[0] for l in open(path).read().split("\n") if l]  # ("ms:" for the line of times)


def test_cli(tmp_path):
    n = 67
    G, K, y = M.fixture(n, ROWS[n], 3.0)
    V = G[:60].copy()
    V[3] = 1      # constant: the tool omits it
    V[5] = 0
    V[5, :2] = 1  # af = 2 / 67 < -maf
    kin = str(tmp_path / "pheno.kinship")
    open(kin, "w").write("\n".join("\t".join("%.17g" % v for v in r) for r in K) + "\n")
    bases = [_write_plink(tmp_path, "P%d" % j, V, yy) for j, yy in enumerate([y, np.random.default_rng(8).permutation(y)])]
    outdir = str(tmp_path / "out")
    tail = ["-k", kin, "-outdir", outdir, "-maf", "0.05", "-miss", "0.5"]
    for j, b in enumerate(bases):
        for mode in ("2", "4"):
            r = subprocess.run([BIN, "-bfile", b, "-lmm", mode, "-o", "L%s_%d" % (mode, j)] + tail, capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stderr
    head2, rows2 = _read(os.path.join(outdir, "L2_0.assoc.txt"))
    head4, rows4 = _read(os.path.join(outdir, "L4_0.assoc.txt"))
    assert head4 == HEADER4 and head2 == "chr\trs\tps\tn_miss\tallele1\tallele0\taf\tl_mle\tp_lrt"
    bed = np.frombuffer(open(bases[0] + ".bed", "rb").read(), np.uint8)[3:]
    yf = _fam_y(bases[0], n)
    h = Handle4(K, 64, 1e-5, 1e5)
    try:
        abi = h.test_all(bed, yf, maf=0.05, miss=0.5)
        l0, lam0 = h.null(yf)
        lR0, lamR0, vg, ve = h.null_reml(yf)
    finally:
        h.close()
    keep = np.flatnonzero(abi["tested"])
    assert 0 < len(keep) < len(V) and len(rows4) == len(keep) == len(rows2)
    for f4, f2, v in zip(rows4, rows2, keep):
        assert len(f4) == 14 and len(f2) == 9
        assert f4[:7] == f2[:7] and f4[10] == f2[7] and f4[12] == f2[8]
        for col, key in ((7, "beta"), (8, "se"), (9, "lam_remle"), (11, "p_wald"), (13, "p_score")):
            assert float(f4[col]) == float("%.6e" % abi[key][v]), (v, key, f4[col], abi[key][v])
    log2, log4 = (os.path.join(outdir, "L%s_0.log.txt" % m) for m in "24")
    k2, k4 = _log_keys(log2), _log_keys(log4)
    assert not set(NEW_LOG_LINES) & set(k2) and "remle" not in open(log2).read()
    assert [k for k in k4 if k not in NEW_LOG_LINES][1:] == k2[1:] and [k for k in k4 if k in NEW_LOG_LINES] == list(NEW_LOG_LINES)
    assert "-lmm 2" in open(log2).read().split("\n")[0] and "-lmm 4" in open(log4).read().split("\n")[0]
    val = dict(l.split("\t") for l in open(log4).read().split("\n")[1:] if "\t" in l)
    assert float(val["lambda0_remle"]) == float("%.6e" % lamR0) and float(val["vg"]) == float("%.6e" % vg) and float(val["ve"]) == float("%.6e" % ve)
    assert float(val["logl_remle_H0"]) == float("%.6f" % lR0) and float(val["lambda0"]) == float("%.6e" % lam0) and float(val["logl_H0"]) == float("%.6f" % l0)
    # --bfiles over two files: one eigendecomposition, the files of the single runs
    lst = str(tmp_path / "list.txt")
    open(lst, "w").write("".join("%s\tM%d\n" % (b, j) for j, b in enumerate(bases)))
    r = subprocess.run([BIN, "--bfiles", lst, "-lmm", "4"] + tail, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "eigendecompositions=1 " in r.stderr, r.stderr
    for j in range(len(bases)):
        single = open(os.path.join(outdir, "L4_%d.assoc.txt" % j), "rb").read()
        assert open(os.path.join(outdir, "M%d.assoc.txt" % j), "rb").read() == single and single.count(b"\n") > 1
        assert _log_keys(os.path.join(outdir, "M%d.log.txt" % j)) == k4
    # -n picks the phenotype column in -lmm 4 as in -lmm 2
    r = subprocess.run([BIN, "-bfile", bases[0], "-lmm", "4", "-n", "1", "-o", "N1"] + tail, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and open(os.path.join(outdir, "N1.assoc.txt"), "rb").read() == open(os.path.join(outdir, "L4_0.assoc.txt"), "rb").read()
