"""lmm_lrt with covariates (-c) on the GPU, through the C ABI, the Python class and the tool, against the numpy models of
lmm_covar_np.py.

Tolerances (-lmin / -lmax = e^-10 / e^10 unless the tool's defaults are what is tested; test_lmm_covar_model.py measures the gaps
between the models without a GPU): min(1e-8, 1000 x the models' gap) for LRT and l0 (absolute), beta, se, F (relative), the REML
value (absolute), vg and ve (relative); P_RTOL of test_gpu_lmm_lrt.py for the chi-square tail and of test_gpu_lmm_lrt_wald.py for
the F tails. Statistics are compared at the tool's own lambdas; lambda and l_remle through the likelihood.

Largest deviations measured on the MI355X (each test prints its own; DESIGN.md 4.12 has them too): LRT within 6.8e-13 of model R
and 3.8e-12 of model E up to n = 241 (the latter with W = [1, two leading eigenvectors of K]), 1.8e-12 of model R at n = 1135; l0
within 2.8e-13, 2.2e-12 and 1.4e-12; p within 3.1e-14 of chi2.sf; model R loses at most 4.5e-13 at the tool's lambdas. W = [1] against
no covariates: |dLRT| <= 1.7e-13; W against W A: 1.1e-13. -lmm 4: beta within 4.4e-13, se within 1.6e-14, F_wald within 8.9e-13 of
model G; p_wald within 1.2e-13 of the t tail of the tool's own F, p_score within 7.0e-13 of the tail of the model's F_score; model
R' loses at most 1.1e-13 at the tool's l_remle, the tool's REML null value is within 1.4e-12 of model R''s, vg and ve within 7.2e-15
of model G's.
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

import lmm_covar_np as CV
import lmm_lrt_np as M
import lmm_table_np as T
import lmm_wald_np as WN
from test_gpu_lmm_lrt import BIN, P_RTOL, ROWS
from test_gpu_lmm_lrt_table import BINDIR, write_case
from test_gpu_lmm_lrt_wald import Handle4, check_tail, tail_sensitivity
from test_lmm_covar_model import (MEASURED_BETA_GAP, MEASURED_F_GAP, MEASURED_LRT_GAP, MEASURED_REML_GAP, MEASURED_SE_GAP,
                                  MEASURED_VG_VE_GAP)

pytestmark = pytest.mark.gpu

LRT_TOL = min(1e-8, 1000 * MEASURED_LRT_GAP)
BETA_TOL = min(1e-8, 1000 * MEASURED_BETA_GAP)
SE_TOL = min(1e-8, 1000 * MEASURED_SE_GAP)
F_TOL = min(1e-8, 1000 * MEASURED_F_GAP)
REML_TOL = min(1e-8, 1000 * MEASURED_REML_GAP)
VG_VE_TOL = min(1e-8, 1000 * MEASURED_VG_VE_GAP)
LRT_KEYS = ("lrt", "lam", "p", "af", "n_miss", "tested")
ALL_KEYS = ("lrt", "lam", "p", "beta", "se", "lam_remle", "p_wald", "p_score", "af", "n_miss", "tested")
NV = 40  # with chunk_variants 32: a chunk boundary and a last tile of 8


class HandleC(Handle4):
    def __init__(self, K, W=None, chunk=32, lmin=M.LMIN, lmax=M.LMAX):
        super().__init__(K, chunk, lmin, lmax)
        if W is not None:
            self.set_covariates(W)

    def set_covariates(self, W):
        if W is None:
            capi.check(lib.kgwas_lmm_set_covariates(self.h, 0, None))
        else:
            W = np.ascontiguousarray(W, np.float64)
            capi.check(lib.kgwas_lmm_set_covariates(self.h, W.shape[1], ptr(W)))


def run(K, W, y, bed, chunk=32, all_tests=False, **kw):
    h = HandleC(K, W, chunk)
    try:
        out = h.test_all(bed, y, **kw) if all_tests else h.test(bed, y, **kw)
        out["l0"], out["lam0"] = h.null(y)
        if all_tests:
            out["null_reml"] = h.null_reml(y)
    finally:
        h.close()
    return out


def same_bits(a, b, keys=LRT_KEYS):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in keys)


def check_lrt(name, K, W, y, xs, out, model_E):
    ref, l0 = CV.lrt_R(K, y, W, xs)
    err, err0 = np.abs(out["lrt"] - ref).max(), abs(out["l0"] - l0)
    msg = "%s: max |LRT - model R| = %.3e, |l0 - model R| = %.3e" % (name, err, err0)
    if model_E:
        ref_e, l0_e = CV.lrt_E(K, y, W, xs)
        err_e, err0_e = np.abs(out["lrt"] - ref_e).max(), abs(out["l0"] - l0_e)
        msg += ", max |LRT - model E| = %.3e, |l0 - model E| = %.3e" % (err_e, err0_e)
    rel = np.abs(out["p"] / chi2.sf(out["lrt"], 1) - 1.0).max()
    worst = 0.0  # lambda through the likelihood: model R at the tool's lambda against model R's own maximum
    for x, lam in list(zip(xs, out["lam"]))[:8]:
        worst = max(worst, M.fit_R(K, y, CV.design(W, x))[0] - CV.loglik_R_at(K, y, W, x, lam))
    worst = max(worst, M.fit_R(K, y, CV.design(W))[0] - CV.loglik_R_at(K, y, W, None, out["lam0"]))
    print(msg + " (allowed %.1e); p within %.3e of chi2.sf (allowed %.1e); model R loses at most %.3e at the tool's lambdas"
          % (LRT_TOL, rel, P_RTOL, worst))
    assert out["tested"].all() and err <= LRT_TOL and err0 <= LRT_TOL and rel <= P_RTOL and worst <= LRT_TOL
    if model_E:
        assert err_e <= LRT_TOL and err0_e <= LRT_TOL
    return ref


@functools.lru_cache(maxsize=None)
def panel(n):
    G, K, y = M.fixture(n, ROWS[n], 3.0)
    V = M.varying(G)[:NV]
    assert len(V) == NV
    return K, y, V


# ---- 1. against the models ----

@pytest.mark.parametrize("q", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [64, 67, 241])
def test_widths(n, q):
    K, y0, V = panel(n)
    W = CV.width(n, ROWS[n], q)
    y = CV.phenotype(y0, W)
    out = run(K, W, y, M.presence_bed(V))
    check_lrt("n=%d q=%d" % (n, q), K, W, y, 2.0 * V, out, model_E=True)
    np.testing.assert_array_equal(out["af"], V.mean(axis=1))


def test_real_panel_width():
    n, q = 1135, 4
    G, K, y0 = M.fixture(n, ROWS[n], 3.0)
    V = M.varying(G)[:48]
    W = CV.width(n, ROWS[n], q)
    y = CV.phenotype(y0, W)
    out = run(K, W, y, M.presence_bed(V), chunk=64)
    check_lrt("n=1135 q=4", K, W, y, 2.0 * V, out, model_E=False)


@pytest.mark.parametrize("form", ["batch", "eigen"])
def test_forms_of_W(form):
    n = 67
    K, y0, V = panel(n)
    W = CV.covariates(n, ROWS[n], form)
    y = CV.phenotype(y0, W)
    out = run(K, W, y, M.presence_bed(V))
    check_lrt("n=67 %s" % form, K, W, y, 2.0 * V, out, model_E=True)


def test_a_column_of_ones_against_no_covariates():
    n = 67
    K, y, V = panel(n)
    bed = M.presence_bed(V)
    with_ones = run(K, np.ones((n, 1)), y, bed)
    without = run(K, None, y, bed)
    ref = check_lrt("n=67 W=[1]", K, np.ones((n, 1)), y, 2.0 * V, with_ones, model_E=False)
    gap = np.abs(with_ones["lrt"] - without["lrt"]).max()
    print("W = [1] against no covariates: max |dLRT| = %.3e (allowed %.1e), |dl0| = %.3e" % (gap, 2 * LRT_TOL, abs(with_ones["l0"] - without["l0"])))
    assert np.abs(without["lrt"] - ref).max() <= LRT_TOL and gap <= 2 * LRT_TOL and abs(with_ones["l0"] - without["l0"]) <= 2 * LRT_TOL


def test_W_and_W_A():
    n = 67
    K, y0, V = panel(n)
    W, WA = CV.covariates(n, ROWS[n], "normal"), CV.covariates(n, ROWS[n], "recombined")
    y = CV.phenotype(y0, W)
    bed = M.presence_bed(V)
    a, b = run(K, W, y, bed), run(K, WA, y, bed)
    check_lrt("n=67 W", K, W, y, 2.0 * V, a, model_E=False)
    check_lrt("n=67 W A", K, WA, y, 2.0 * V, b, model_E=False)
    print("W against W A: max |dLRT| = %.3e" % np.abs(a["lrt"] - b["lrt"]).max())


# ---- 2. bits ----

def test_bits():
    n, q = 67, 3
    K, y0, D = M.codes_panel(n, ROWS[n], NV)
    W = CV.width(n, ROWS[n], q)
    y = CV.phenotype(y0, W)
    bed = M.pack_bed(D)
    kw = dict(maf=0.05, miss=0.05)
    for all_tests, keys in ((False, LRT_KEYS), (True, ALL_KEYS)):
        a = run(K, W, y, bed, chunk=32, all_tests=all_tests, **kw)
        assert 10 <= a["tested"].sum() < NV
        assert same_bits(a, run(K, W, y, bed, chunk=32, all_tests=all_tests, **kw), keys), "two runs differ"
        assert same_bits(a, run(K, W, y, bed, chunk=4096, all_tests=all_tests, **kw), keys), "chunk_variants 32 and 4096 differ"
        perm = np.random.default_rng(3).permutation(NV)
        b = run(K, W, y, bed[perm], chunk=32, all_tests=all_tests, **kw)
        assert same_bits({k: a[k][perm] for k in keys}, b, keys), "a permuted variant order changes a variant's numbers"
        assert (a["l0"], a["lam0"]) == (b["l0"], b["lam0"])
        if all_tests:
            two = run(K, W, y, bed, chunk=32, **kw)
            assert same_bits(a, two), "lrt, lambda or p of kgwas_lmm_test_bed_all differ from kgwas_lmm_test_bed's"
            assert a["null_reml"] == b["null_reml"]


# ---- 3. -lmm 4 ----

def check_statistics(name, K, W, y, X, out):
    n, q = W.shape
    df = n - q - 1
    gb = gs = gF = 0.0
    Fs_model = np.zeros(len(X))
    for v, x in enumerate(X):
        b, s, F, _ = CV.gls_G(K, y, W, x, out["lam_remle"][v])
        Fs_model[v] = CV.score_G(K, y, W, x, out["lam0"])
        gb, gs = max(gb, abs(out["beta"][v] / b - 1)), max(gs, abs(out["se"][v] / s - 1))
        gF = max(gF, abs((out["beta"][v] / out["se"][v]) ** 2 / F - 1))
    print("%s: beta within %.3e (allowed %.1e), se within %.3e (allowed %.1e), F_wald within %.3e (allowed %.1e) of model G, relative"
          % (name, gb, BETA_TOL, gs, SE_TOL, gF, F_TOL))
    assert gb <= BETA_TOL and gs <= SE_TOL and gF <= F_TOL
    Fw = (out["beta"] / out["se"]) ** 2
    check_tail(name + ", p_wald", out["p_wald"], Fw, df)
    check_tail(name + ", p_score", out["p_score"], Fs_model, df, extra=F_TOL * tail_sensitivity(Fs_model, df))
    # l_remle through the likelihood, on the basis the tool uses
    worst = 0.0
    for x, lam in list(zip(X, out["lam_remle"]))[:4]:
        worst = max(worst, CV.fit_reml_R(K, y, W, x)[0] - CV.reml_R_at(K, y, W, x, lam))
    lR0, lam, vg, ve = out["null_reml"]
    best0 = CV.fit_reml_R(K, y, W, None)[0]
    at_tool = CV.reml_R_at(K, y, W, None, lam)
    gvg, gve = CV.vg_ve_G(K, y, W, lam)
    gap = max(abs(vg / gvg - 1), abs(ve / gve - 1))
    print("%s: model R' loses at most %.3e at the tool's l_remle and %.3e at lambda0_remle, the tool's REML value differs by %.3e (allowed %.1e); "
          "vg, ve within %.3e of model G's (allowed %.1e)" % (name, worst, best0 - at_tool, abs(lR0 - at_tool), REML_TOL, gap, VG_VE_TOL))
    assert worst <= REML_TOL and best0 - at_tool <= REML_TOL and abs(lR0 - at_tool) <= REML_TOL and gap <= VG_VE_TOL and vg == lam * ve


@pytest.mark.parametrize("q", [2, 3])
@pytest.mark.parametrize("n", [67, 241])
def test_lmm4(n, q):
    W = CV.width(n, ROWS[n], q)
    K, base, g, V = M.strong_fixture(n, M.STRONG_ROWS[n], nv=12)
    cases = [("strong n=%d q=%d" % (n, q), CV.phenotype(base + 10.0 * g, W)), ("noise n=%d q=%d" % (n, q), CV.phenotype(WN.noise_phenotype(n), W))]
    for name, y in cases:
        bed = M.presence_bed(V)
        out = run(K, W, y, bed, all_tests=True)
        assert out["tested"].all() and np.isfinite(np.stack([out[k] for k in ALL_KEYS[:8]])).all()
        check_statistics(name, K, W, y, 2.0 * V, out)
        two = run(K, W, y, bed)
        assert same_bits(out, two), name + ": lrt, lambda or p of kgwas_lmm_test_bed_all differ from kgwas_lmm_test_bed's"
        if name.startswith("strong"):
            assert out["beta"][0] == pytest.approx(5.0, rel=0.2)  # (per unit of the dosage: presence is 2)


# ---- 4. the session's state ----

def test_state():
    n = 67
    K, y0, V = panel(n)
    W = CV.width(n, ROWS[n], 3)
    y = CV.phenotype(y0, W)
    bed = M.presence_bed(V)
    fresh = run(K, None, y, bed)
    with_w = run(K, W, y, bed)
    h = HandleC(K)
    try:
        before = h.null(y)
        assert before == (fresh["l0"], fresh["lam0"])
        h.set_covariates(W)
        assert h.null(y) == (with_w["l0"], with_w["lam0"]) != before, "the null model was not fitted again"
        assert same_bits(h.test(bed, y), with_w)
        Y = np.stack([y, y0])
        out = np.zeros((2, NV))
        rc = lib.kgwas_lmm_test_bed_multi(h.h, 2, ptr(Y), ptr(bed), NV, 0.0, 1.0, ptr(out), None, None, None, None, None, None, None)
        assert rc == capi.KGWAS_ERR_ARG and "covariates are not built for the multi-phenotype passes" in lib.kgwas_last_error().decode()
        # refused covariates leave the handle as it was
        bad = W.copy()
        bad[:, 2] = 2 * bad[:, 1] - bad[:, 0]
        assert lib.kgwas_lmm_set_covariates(h.h, 3, ptr(bad)) == capi.KGWAS_ERR_ARG and "rank-deficient" in lib.kgwas_last_error().decode()
        no_one, wide = np.ascontiguousarray(W[:, 1:]), np.ones((n, 9))
        assert lib.kgwas_lmm_set_covariates(h.h, 2, ptr(no_one)) == capi.KGWAS_ERR_ARG
        assert "do not span the constant" in lib.kgwas_last_error().decode()
        assert lib.kgwas_lmm_set_covariates(h.h, 9, ptr(wide)) == capi.KGWAS_ERR_ARG and "at most 8" in lib.kgwas_last_error().decode()
        ones = np.ones((n, 1))  # (a valid W: what is refused here are the null pointers)
        assert lib.kgwas_lmm_set_covariates(h.h, 1, None) == capi.KGWAS_ERR_ARG and lib.kgwas_lmm_set_covariates(None, 1, ptr(ones)) == capi.KGWAS_ERR_ARG
        assert same_bits(h.test(bed, y), with_w)
        h.set_covariates(None)
        assert same_bits(h.test(bed, y), fresh) and h.null(y) == before, "q = 0 does not restore the bits of a fresh handle"
        capi.check(lib.kgwas_lmm_test_bed_multi(h.h, 2, ptr(Y), ptr(bed), NV, 0.0, 1.0, ptr(out), None, None, None, None, None, None, None))
        assert out[0].tobytes() == fresh["lrt"].tobytes()
    finally:
        h.close()
    # the Python class takes covariates= and refuses the multi-phenotype .bed pass too
    import kmersgwas_amd as kg
    m = kg.LmmLrt(K, lmin=M.LMIN, lmax=M.LMAX, chunk_variants=32, covariates=W)
    r = m.test(bed.tobytes(), y)
    assert r["lrt"].tobytes() == with_w["lrt"].tobytes() and m.null(y) == (with_w["l0"], with_w["lam0"])
    with pytest.raises(capi.KgwasError, match="multi-phenotype"):
        m.test_bed_multi(Y, bed.tobytes())
    m.set_covariates(None)
    assert m.test(bed.tobytes(), y)["lrt"].tobytes() == fresh["lrt"].tobytes()
    m.close()


def test_too_few_individuals_on_a_live_handle():
    """n >= q + 2 through the C ABI: 5 individuals take q = 3 (the boundary: one residual degree of freedom under H1, so the numbers
    are only asked to be finite here) and refuse q = 4, and the refusal leaves the handle's covariates"""
    n = 5
    G, K, y = M.fixture(n, ROWS[n], 3.0)
    V = M.varying(G)[:8]
    bed = M.presence_bed(V)
    W4 = np.column_stack([np.ones(n), np.arange(n), np.arange(n) ** 2.0, [1.0, 0, 0, 1, 0]])
    W3 = np.ascontiguousarray(W4[:, :3])
    h = HandleC(K)
    try:
        h.set_covariates(W3)
        with_w3 = h.test(bed, y)
        assert with_w3["tested"].all() and np.isfinite(with_w3["lrt"]).all()
        assert lib.kgwas_lmm_set_covariates(h.h, 4, ptr(W4)) == capi.KGWAS_ERR_ARG
        msg = lib.kgwas_last_error().decode()
        assert "5 individuals are too few for 4 covariate columns" in msg and "at least 6" in msg, msg
        assert same_bits(h.test(bed, y), with_w3)
    finally:
        h.close()


def test_multi_phenotype_table_pass_refuses_covariates(tmp_path):
    """kgwas_lmm_test_table_multi on a handle with covariates answers with the stated error before it reads the table, the handle
    keeps its covariates, and after set_covariates(None) the pass runs with the bits of the one-column pass of a fresh handle."""
    import kmersgwas_amd as kg
    S, n_rows = 67, 300
    K, y = T.kinship_and_phenotype(S)
    pick = np.arange(S, dtype=np.uint64)
    rows = T.table_from_bits(T.random_bits(n_rows, S, 41), S, pick, 41)
    base, _ = write_case(tmp_path, rows, S, pick)
    W = CV.width(S, ROWS[S], 3)
    Y = np.stack([CV.phenotype(y, W), y])
    tbl = kg.KmersTable(base, T.K_LEN)
    fresh = kg.LmmLrt(K, chunk_variants=32)
    m = kg.LmmLrt(K, chunk_variants=32, covariates=W)
    try:
        plain = [fresh.test_table(tbl, pick, Y[k], 5, 0.05, 20) for k in range(2)]
        with_w = m.test_table(tbl, pick, Y[0], 5, 0.05, 20)
        assert len(with_w["row"]) == 20 and with_w["lrt"].tobytes() != plain[0]["lrt"].tobytes()
        before = m.stats()
        with pytest.raises(capi.KgwasError, match="covariates are not built for the multi-phenotype passes") as e:
            m.test_table_multi(tbl, pick, Y, 5, 0.05, 20)
        assert e.value.code == capi.KGWAS_ERR_ARG and "kgwas_lmm_test_table_multi" in e.value.msg
        assert m.stats() == before, "rows were read or tested before the refusal"
        again = m.test_table(tbl, pick, Y[0], 5, 0.05, 20)
        assert all(again[k].tobytes() == with_w[k].tobytes() for k in ("row", "lrt", "lambda", "p", "af")), "the refusal changed the handle"
        m.set_covariates(None)
        res = m.test_table_multi(tbl, pick, Y, 5, 0.05, 20)
        for k in range(2):
            for f in ("row", "kmer", "lrt", "lambda", "p", "af"):
                assert res["columns"][k][f].tobytes() == plain[k][f].tobytes(), (k, f)
    finally:
        m.close()
        fresh.close()
        tbl.close()


# ---- 5. the tool ----

def _write_bfile(base, D, pheno):
    """PLINK files by hand: D dosages (variants x individuals), pheno one value per individual (NaN: -9)"""
    m, n = D.shape
    open(base + ".bed", "wb").write(bytes([0x6C, 0x1B, 0x01]) + M.pack_bed(D).tobytes())
    open(base + ".bim", "w").write("".join("1\tv%d\t0\t%d\tA\tC\n" % (v, 100 + v) for v in range(m)))
    open(base + ".fam", "w").write("".join("f%d i%d 0 0 0 %s\n" % (i, i, "-9" if np.isnan(p) else repr(float(p))) for i, p in enumerate(pheno)))
    return base


def _write_cov(path, W, na_rows=()):
    lines = []
    for i, r in enumerate(W):
        f = [repr(float(v)) for v in r]
        if i in na_rows:
            f[-1] = "NA"
        lines.append(" ".join(f))
    open(path, "w").write("\n".join(lines) + "\n")
    return path


def _write_kin(path, K):
    open(path, "w").write("\n".join("\t".join("%.17g" % v for v in r) for r in K) + "\n")
    return path


def _tool(args):
    r = subprocess.run([BIN] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def _log(path):
    return dict(l.split("\t", 1) for l in open(path).read().split("\n") if "\t" in l)


@pytest.mark.parametrize("mode", ["2", "4"])
def test_cli_dropped_individuals(tmp_path, mode):
    K, D, pheno = M.dropped_panel()
    n = K.shape[0]
    y = pheno[:, 0]
    W = CV.width(n, 400, 3)
    na_rows = (5, 17, 40)
    assert not set(na_rows) & set(M.DROPPED)
    kept = np.array([i for i in range(n) if not np.isnan(y[i]) and i not in na_rows])
    assert len(kept) == n - len(M.DROPPED) - 3
    full = _write_bfile(str(tmp_path / "full"), D, y)
    small = _write_bfile(str(tmp_path / "small"), D[:, kept], y[kept])
    cov_full = _write_cov(str(tmp_path / "full.cov"), W, na_rows)
    cov_small = _write_cov(str(tmp_path / "small.cov"), W[kept])
    kin_full = _write_kin(str(tmp_path / "full.kin"), K)
    kin_small = _write_kin(str(tmp_path / "small.kin"), K[np.ix_(kept, kept)])
    out = str(tmp_path / "out")
    tail = ["-lmm", mode, "-outdir", out, "-maf", "0.05", "-miss", "0.05"]
    _tool(["-bfile", full, "-k", kin_full, "-c", cov_full, "-o", "full"] + tail)
    _tool(["-bfile", small, "-k", kin_small, "-c", cov_small, "-o", "small"] + tail)
    a, b = (open(os.path.join(out, "%s.assoc.txt" % s), "rb").read() for s in ("full", "small"))
    assert a == b and a.count(b"\n") > 10
    log = _log(os.path.join(out, "full.log.txt"))
    assert log["covariates"] == cov_full and log["n_covariates"] == "3"
    assert log["individuals_in_fam"] == str(n) and log["individuals_used"] == str(len(kept))
    keys = [l.split("\t")[0] for l in open(os.path.join(out, "full.log.txt")).read().split("\n") if "\t" in l]
    assert keys[keys.index("kinship") + 1:keys.index("kinship") + 3] == ["covariates", "n_covariates"]
    # without -c the log has neither line, and the numbers differ
    _tool(["-bfile", full, "-k", kin_full, "-o", "plain"] + tail)
    plain = open(os.path.join(out, "plain.log.txt")).read()
    assert "covariates" not in plain and open(os.path.join(out, "plain.assoc.txt"), "rb").read() != a


def test_cli_bfiles(tmp_path):
    K, D, pheno = M.dropped_panel()
    n = K.shape[0]
    W = CV.width(n, 400, 2)
    cov = _write_cov(str(tmp_path / "c.cov"), W, (5,))
    kin = _write_kin(str(tmp_path / "k.kin"), K)
    bases = [_write_bfile(str(tmp_path / ("B%d" % j)), D[10 * j:10 * j + 20], pheno[:, c]) for j, c in enumerate((0, 2))]  # one missing set
    out = str(tmp_path / "out")
    tail = ["-k", kin, "-c", cov, "-lmm", "2", "-outdir", out, "-maf", "0.05", "-miss", "0.05"]
    for j, b in enumerate(bases):
        _tool(["-bfile", b, "-o", "S%d" % j] + tail)
    lst = str(tmp_path / "list.txt")
    open(lst, "w").write("".join("%s\tM%d\n" % (b, j) for j, b in enumerate(bases)))
    r = _tool(["--bfiles", lst] + tail)
    assert "eigendecompositions=1 " in r.stderr, r.stderr
    for j in range(2):
        single = open(os.path.join(out, "S%d.assoc.txt" % j), "rb").read()
        assert open(os.path.join(out, "M%d.assoc.txt" % j), "rb").read() == single and single.count(b"\n") > 5
        assert _log(os.path.join(out, "M%d.log.txt" % j))["n_covariates"] == "2"


def test_cli_table_route(tmp_path):
    S, n_rows = 67, 300
    K, y = T.kinship_and_phenotype(S)
    pick = np.arange(S)
    rows = T.table_from_bits(T.random_bits(n_rows, S, 41), S, pick, 41)
    base, acc = write_case(tmp_path, rows, S, pick)
    W = CV.width(S, ROWS[S], 3)
    ph = tmp_path / "pheno.tsv"
    ph.write_text("accession_id\tv\n" + "".join("%s\t%.6f\n" % (a, v) for a, v in zip(acc, CV.phenotype(y, W))))
    cov = _write_cov(str(tmp_path / "c.cov"), W)
    kin = _write_kin(str(tmp_path / "k.kin"), K)
    out, plink = str(tmp_path / "out"), str(tmp_path / "plink")
    r = subprocess.run([os.path.join(BINDIR, "kmers_table_to_bed"), "-t", base, "-k", str(T.K_LEN), "-p", str(ph), "--maf", "0.05", "--mac", "5",
                        "-b", "100000", "-o", plink], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    common = ["-lmm", "2", "-k", kin, "-c", cov, "-outdir", out, "-maf", "0.05"]
    _tool(["-bfile", plink + ".0", "-o", "bed"] + common)
    bed_lines = open(os.path.join(out, "bed.assoc.txt")).read().split("\n")
    assert len(bed_lines) > 50
    table = ["--kmers_table", base, "--kmers_len", str(T.K_LEN), "-p", str(ph), "--mac", "5"]
    _tool(table + ["-o", "all"] + common)
    assert open(os.path.join(out, "all.assoc.txt")).read().split("\n") == bed_lines, "the whole file differs"
    # the best 20: ranked with the library on the files the first tool wrote
    import kmersgwas_amd as kg
    yy, keep, cnt = np.zeros(S), np.zeros(S, np.uint8), C.c_uint64()
    capi.check(lib.kgwas_lmm_read_fam((plink + ".0.fam").encode(), 1, S, ptr(yy), ptr(keep), C.byref(cnt)))
    assert keep.all()
    m = kg.LmmLrt(K, chunk_variants=64, covariates=W)
    res = m.test(np.frombuffer(open(plink + ".0.bed", "rb").read(), np.uint8)[3:], yy, maf=0.05, miss=0.05)
    m.close()
    tested = np.flatnonzero(res["tested"])
    assert len(tested) == len(bed_lines) - 2
    top = np.sort(np.lexsort((tested, -res["lrt"][tested]))[:20])
    _tool(table + ["-o", "top", "--best", "20", "--chunk_variants", "32"] + common)
    top_lines = open(os.path.join(out, "top.assoc.txt")).read().split("\n")
    assert top_lines == [bed_lines[0]] + [bed_lines[1 + i] for i in top] + [""], "the best 20 differ"
    lb, lt = _log(os.path.join(out, "bed.log.txt")), _log(os.path.join(out, "top.log.txt"))
    assert lt["covariates"] == cov and lt["n_covariates"] == "3" and lt["lambda0"] == lb["lambda0"] and lt["logl_H0"] == lb["logl_H0"]
    _tool(table + ["-o", "plain", "-lmm", "2", "-k", kin, "-outdir", out, "-maf", "0.05"])
    assert open(os.path.join(out, "plain.assoc.txt")).read().split("\n") != bed_lines
