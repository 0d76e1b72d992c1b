"""lmm_lrt with covariates (-c) on the GPU at every width: the eight <Q> instantiations of lmm_base_cov_kernel, lmm_null_cov_kernel,
lmm_null_reml_cov_kernel, lmm_refine_cov_kernel and lmm_refine_all_cov_kernel against the numpy models of lmm_covar_np.py, their
bits, W that strains the factorisation, likelihoods with two interior maxima, and variants whose x lies in span(W).
test_gpu_lmm_lrt_covar.py has q = 1, 2, 3, 8 for the ML LRT, q = 2, 3 for -lmm 4 and q = 3 for the bits; this module has the rest
(the table under "which Q where" below), so that between the two every Q of 1..8 runs kgwas_lmm_test_bed, kgwas_lmm_test_bed_all,
kgwas_lmm_null and kgwas_lmm_null_reml against a model.

Tolerances: check_lrt and check_statistics of test_gpu_lmm_lrt_covar.py are called as they are and assert that module's own gates.
On top, every family of fixtures has its models' gaps measured by test_lmm_covar_model.py without a GPU (MEASURED_WIDTHS_GAPS,
MEASURED_WIDTH_1135_GAPS, MEASURED_EIGEN_Q_GAPS, MEASURED_RECOMBINED_Q8_GAPS, MEASURED_TWO_PEAK_W_*), and the tool is held to
min(1e-8, 1000 x that family's gap) as well: LRT and l0 (absolute, against model R), beta, se, F (relative), the REML value
(absolute), vg and ve (relative). So the smaller of the two gates holds. The chi-square tail has P_RTOL of test_gpu_lmm_lrt.py, the
F tails check_tail of test_gpu_lmm_lrt_wald.py. Statistics are compared at the tool's own lambdas; lambdas through the likelihood.

Which Q where (n in brackets):
  ML against models R and E     q = 4, 5, 6, 7 [64, 67]; 5, 6, 7 [241]; eigen_q 4, 6, 8 [67]; recombined 8 [67]; two peaks 2, 3 [8, 16, 67]
  ML against model R            q = 7 [1135]
  -lmm 4 against model G        q = 1, 4, 5, 6, 7, 8 [67]; 1, 8 [241]; eigen_q 4, 6, 8 [67]; recombined 8 [67]; two peaks 2, 3 [67]
  -lmm 4 against model R'       q = 7 [1135]
  bits                          q = 1, 2, 4, 5, 6, 7, 8 [67]
  x in span(W)                  q = 2 [67], and q = 4 [67] as the control

Largest deviations measured on the MI355X (each test prints its own; DESIGN.md 4.12 has them too):
  width q = 4 .. 7 (n = 64, 67, 241), the span panel's control   LRT within 5.1e-13 of model R and 1.1e-12 of model E, l0 within 3.4e-13 and
      5.7e-13, p within 3.0e-14 of chi2.sf, model R loses at most 1.7e-13 at the tool's lambdas
  width q = 7, n = 1135          LRT within 3.6e-12 of model R, which loses at most 9.1e-13 at the tool's lambdas
  -lmm 4, width q = 1, 4 .. 8    beta within 1.0e-12, se 1.6e-14, F_wald 2.1e-12 of model G; p_wald within 5.2e-14 of the t tail of the tool's
      own F, p_score within 6.9e-13 of the tail of the model's F_score; model R' loses at most 1.1e-13 at the tool's l_remle; the REML null
      value within 1.4e-12, vg and ve within 7.9e-15
  -lmm 4, q = 7, n = 1135        beta within 1.8e-11, se 4.8e-13, F_wald 3.5e-11 of model R'; p_wald 1.8e-13, p_score 6.9e-11; model R' loses at
      most 4.5e-13; the REML null value within 2.7e-11, vg and ve within 1.6e-15
  eigen_q q = 4, 6, 8            LRT within 1.1e-13 of model R and 5.1e-12 of model E; beta 5.6e-12, se 9.1e-15, F_wald 1.1e-11; REML value 2.0e-13
  recombined_q8                  LRT within 5.1e-13 of model R and 8.0e-13 of model E; beta 1.3e-11, F_wald 2.7e-11. W against W A: |dLRT| <= 1.7e-13,
      l0 equal; each run against model G of the other basis: beta 7.4e-12, se 5.1e-15, F 1.5e-11; run against run at their own l_remle
      (a record, not a gate): beta 8.1e-13, se 2.7e-15, F 1.6e-12, log l_remle 2.2e-13
  two interior maxima            LRT within 2.1e-12 of model R and 4.4e-12 of model E; model R loses at most 5.7e-14 at the tool's lambda over all
      variants and under H0. -lmm 4: beta 4.0e-13, se 4.0e-15, F_wald 8.0e-13 of model G; model R' loses at most 5.7e-14 at the tool's l_remle
  x in span(W)                   through the C ABI (range e^-10 .. e^10): lrt 0, p 1, p_score 1, p_wald NaN, beta +-inf, se NaN on all three rows;
      the tool (its default range): p_lrt, p_wald and p_score 1.000000e+00, beta +-4.000000e+00, se -nan

Each of three arithmetic-only mutations of lmm_kernels.hip (scratch builds) fails this module: RSS0' of cov_record<6> with adb in place of
2 adb fails test_widths[241-6] and test_leading_eigenvectors_as_covariates[6]; ll_cov<8> without log xx.w under REML fails test_lmm4[67-8]
and test_leading_eigenvectors_as_covariates[8]; a CovModel search that takes an interior candidate only if it beats the ends by 1.0 fails
31 tests, every two-peaked n = 67 case among them. test_gpu_lmm_lrt_covar.py passes under the first two.
"""
import functools
import os

import numpy as np
import pytest

import lmm_covar_np as CV
import lmm_lrt_np as M
import lmm_wald_np as WN
from test_gpu_lmm_lrt import P_RTOL, ROWS
from test_gpu_lmm_lrt_covar import (ALL_KEYS, LRT_KEYS, LRT_TOL, NV, REML_TOL, HandleC, _tool, _write_cov, _write_kin, check_lrt,
                                    check_statistics, panel, run, same_bits)
from test_gpu_lmm_lrt_wald import check_tail, tail_sensitivity
from test_lmm_covar_model import (MEASURED_EIGEN_Q_GAPS, MEASURED_RECOMBINED_Q8_GAPS, MEASURED_RECOMBINED_Q8_INVARIANCE,
                                  MEASURED_TWO_PEAK_W_G_GAPS, MEASURED_TWO_PEAK_W_LRT_GAP, MEASURED_WIDTH_1135_GAPS, MEASURED_WIDTHS_GAPS,
                                  TWO_PEAK_G_MAX)

pytestmark = pytest.mark.gpu


def tolerances(gaps):
    return {k: min(1e-8, 1000 * v) for k, v in gaps.items()}


WIDTHS_TOL = tolerances(MEASURED_WIDTHS_GAPS)
WIDTH_1135_TOL = tolerances(MEASURED_WIDTH_1135_GAPS)
EIGEN_Q_TOL = tolerances(MEASURED_EIGEN_Q_GAPS)
RECOMBINED_Q8_TOL = tolerances(MEASURED_RECOMBINED_Q8_GAPS)
INVARIANCE_TOL = min(1e-8, 1000 * MEASURED_RECOMBINED_Q8_INVARIANCE)
TWO_PEAK_LRT_TOL = min(1e-8, 1000 * MEASURED_TWO_PEAK_W_LRT_GAP)
STATS = ALL_KEYS[:8]


def check_lrt_family(name, K, W, y, xs, out, model_E, tol):
    """check_lrt with its own gates, then LRT and l0 against model R within the family's tolerance"""
    ref = check_lrt(name, K, W, y, xs, out, model_E)
    err, err0 = np.abs(out["lrt"] - ref).max(), abs(out["l0"] - M.fit_R(K, y, CV.design(W))[0])
    print("%s: the family allows %.1e for |LRT - model R| = %.3e and |l0 - model R| = %.3e" % (name, tol["lrt"], err, err0))
    assert err <= tol["lrt"] and err0 <= tol["lrt"]
    return ref


def statistic_deviations(K, W, y, X, out, model="G"):
    """(beta, se, F_wald: largest relative deviation from the model at the tool's l_remle; |REML value - model R'|; vg, ve relative)"""
    gb = gs = gF = 0.0
    for v, x in enumerate(X):
        b, s, F = (CV.gls_G(K, y, W, x, out["lam_remle"][v])[:3] if model == "G" else CV.wald_R(K, y, W, x, out["lam_remle"][v]))
        gb, gs = max(gb, abs(out["beta"][v] / b - 1)), max(gs, abs(out["se"][v] / s - 1))
        gF = max(gF, abs((out["beta"][v] / out["se"][v]) ** 2 / F - 1))
    lR0, lam, vg, ve = out["null_reml"]
    mvg, mve = (CV.vg_ve_G if model == "G" else CV.vg_ve_R)(K, y, W, lam)
    return dict(beta=gb, se=gs, F=gF, reml=abs(lR0 - CV.reml_R_at(K, y, W, None, lam)), vgve=max(abs(vg / mvg - 1), abs(ve / mve - 1)))


def check_statistics_family(name, K, W, y, X, out, tol):
    """check_statistics (model G) with its own gates, then the same deviations within the family's tolerances"""
    check_statistics(name, K, W, y, X, out)
    dev = statistic_deviations(K, W, y, X, out)
    print("%s: the family allows %s for %s" % (name, " ".join("%s %.1e" % (k, tol[k]) for k in dev), " ".join("%s %.3e" % kv for kv in dev.items())))
    assert all(dev[k] <= tol[k] for k in dev), dev
    return dev


def check_statistics_R(name, K, W, y, X, out, tol):
    """check_statistics against model R' (wald_R, score_R, reml_R_at, vg_ve_R) at the tool's lambdas: at n = 1135 model G costs a
    Cholesky factor of 1135 x 1135 per variant"""
    n, q = W.shape
    df = n - q - 1
    dev = statistic_deviations(K, W, y, X, out, model="R'")
    print("%s: beta within %.3e (allowed %.1e), se within %.3e (allowed %.1e), F_wald within %.3e (allowed %.1e) of model R', relative"
          % (name, dev["beta"], tol["beta"], dev["se"], tol["se"], dev["F"], tol["F"]))
    assert dev["beta"] <= tol["beta"] and dev["se"] <= tol["se"] and dev["F"] <= tol["F"]
    Fs_model = np.array([CV.score_R(K, y, W, x, out["lam0"]) for x in X])
    check_tail(name + ", p_wald", out["p_wald"], (out["beta"] / out["se"]) ** 2, df)
    check_tail(name + ", p_score", out["p_score"], Fs_model, df, extra=tol["F"] * tail_sensitivity(Fs_model, df))
    worst = 0.0
    for x, lam in list(zip(X, out["lam_remle"]))[:4]:
        worst = max(worst, CV.fit_reml_R(K, y, W, x)[0] - CV.reml_R_at(K, y, W, x, lam))
    lR0, lam, vg, ve = out["null_reml"]
    loss0 = CV.fit_reml_R(K, y, W, None)[0] - CV.reml_R_at(K, y, W, None, lam)
    print("%s: model R' loses at most %.3e at the tool's l_remle and %.3e at lambda0_remle, the tool's REML value differs by %.3e (allowed %.1e); "
          "vg, ve within %.3e of model R''s (allowed %.1e)" % (name, worst, loss0, dev["reml"], tol["reml"], dev["vgve"], tol["vgve"]))
    assert worst <= tol["reml"] and loss0 <= tol["reml"] and dev["reml"] <= tol["reml"] and dev["vgve"] <= tol["vgve"] and vg == lam * ve


def first(out, k):
    """the first k variants of a result, with what belongs to the run"""
    return {key: (v[:k] if isinstance(v, np.ndarray) else v) for key, v in out.items()}


# ---- 1. every width, ML ----

@pytest.mark.parametrize("n,q", [(n, q) for n in (64, 67) for q in (4, 5, 6, 7)] + [(241, q) for q in (5, 6, 7)])
def test_widths(n, q):
    K, y0, V = panel(n)
    V = V if n < 241 else V[:16]  # (model E costs an eigendecomposition per variant)
    W = CV.width(n, ROWS[n], q)
    y = CV.phenotype(y0, W)
    out = run(K, W, y, M.presence_bed(V))
    check_lrt_family("n=%d q=%d" % (n, q), K, W, y, 2.0 * V, out, True, WIDTHS_TOL)
    np.testing.assert_array_equal(out["af"], V.mean(axis=1))


def test_real_panel_width():
    """n % 64 != 0 and 18 strides of the lanes over i: the tails of cov_sum_pass differ from the small sizes"""
    n, q = 1135, 7
    G, K, y0 = M.fixture(n, ROWS[n], 3.0)
    V = M.varying(G)[:16]
    W = CV.width(n, ROWS[n], q)
    y = CV.phenotype(y0, W)
    out = run(K, W, y, M.presence_bed(V), chunk=64)
    check_lrt_family("n=1135 q=7", K, W, y, 2.0 * V, out, False, WIDTH_1135_TOL)


# ---- 2. every width, -lmm 4 ----

def lmm4_cases(n, q, rows):
    W = CV.width(n, rows, q)
    K, base, g, V = M.strong_fixture(n, M.STRONG_ROWS[n], nv=12)
    return K, W, V, [("strong n=%d q=%d" % (n, q), CV.phenotype(base + 10.0 * g, W))]


@pytest.mark.parametrize("n,q", [(67, q) for q in (1, 4, 5, 6, 7, 8)] + [(241, 1), (241, 8)])
def test_lmm4(n, q):
    K, W, V, cases = lmm4_cases(n, q, ROWS[n])
    cases.append(("noise n=%d q=%d" % (n, q), CV.phenotype(WN.noise_phenotype(n), W)))
    bed = M.presence_bed(V)
    for name, y in cases:
        out = run(K, W, y, bed, all_tests=True)
        assert out["tested"].all() and np.isfinite(np.stack([out[k] for k in STATS])).all()
        check_statistics_family(name, K, W, y, 2.0 * V, out, WIDTHS_TOL)
        assert same_bits(out, run(K, W, y, bed)), name + ": lrt, lambda or p of kgwas_lmm_test_bed_all differ from kgwas_lmm_test_bed's"
        if name.startswith("strong"):
            assert out["beta"][0] == pytest.approx(5.0, rel=0.2)  # (per unit of the dosage: presence is 2)


def test_lmm4_real_panel_width():
    n, q = 1135, 7
    K, W, V, [(name, y)] = lmm4_cases(n, q, ROWS[n])
    bed = M.presence_bed(V)
    out = run(K, W, y, bed, all_tests=True, chunk=64)
    assert out["tested"].all() and np.isfinite(np.stack([out[k] for k in STATS])).all()
    check_statistics_R(name, K, W, y, 2.0 * V, out, WIDTH_1135_TOL)
    assert same_bits(out, run(K, W, y, bed, chunk=64)), "lrt, lambda or p of kgwas_lmm_test_bed_all differ from kgwas_lmm_test_bed's"
    assert out["beta"][0] == pytest.approx(5.0, rel=0.2)


# ---- 3. bits at every width ----

@pytest.mark.parametrize("q", [1, 2, 4, 5, 6, 7, 8])
def test_bits(q):
    """test_gpu_lmm_lrt_covar.py's test_bits (q = 3) at the other widths: heterozygous and missing calls are in the panel"""
    n = 67
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
            assert a["null_reml"] == b["null_reml"], "null_reml is not stable"
            t = a["tested"].astype(bool)
            assert all(np.isfinite(a[k][t]).all() and np.isnan(a[k][~t]).all() for k in STATS)


# ---- 4. W that strains the factorisation ----

def ml_and_lmm4(name, K, W, y, V, tol, n_stat=12):
    """One kgwas_lmm_test_bed_all run over the panel: its LRT against models R and E (and bit-equal to kgwas_lmm_test_bed's), the
    statistics of its first n_stat variants against model G"""
    bed = M.presence_bed(V)
    out = run(K, W, y, bed, all_tests=True)
    assert out["tested"].all() and np.isfinite(np.stack([out[k] for k in STATS])).all()
    assert same_bits(out, run(K, W, y, bed)), name + ": lrt, lambda or p of kgwas_lmm_test_bed_all differ from kgwas_lmm_test_bed's"
    check_lrt_family(name, K, W, y, 2.0 * V, out, True, tol)
    check_statistics_family(name, K, W, y, 2.0 * V[:n_stat], first(out, n_stat), tol)
    return out


@pytest.mark.parametrize("q", [4, 6, 8])
def test_leading_eigenvectors_as_covariates(q):
    """A's diagonal runs from 1 down to 1 / (lambda d_max + 1), 1e-7 at the upper end of the range"""
    n = 67
    K, y0, V = panel(n)
    W = CV.eigen_q(n, ROWS[n], q)
    ml_and_lmm4("n=67 eigen_q q=%d" % q, K, W, CV.phenotype(y0, W), V, EIGEN_Q_TOL)


def test_recombined_q8():
    """W A with a badly scaled A (condition number 2.9e5; test_lmm_covar_model.py asserts 1e4 .. 1e6): the host's Gram-Schmidt has
    work to do, and nothing but the REML value may move"""
    n = 67
    K, y0, V = panel(n)
    W, WA = CV.width(n, ROWS[n], 8), CV.recombined_q8(n, ROWS[n])
    y = CV.phenotype(y0, W)
    a = ml_and_lmm4("n=67 q=8 W", K, W, y, V, WIDTHS_TOL)
    b = ml_and_lmm4("n=67 q=8 W A", K, WA, y, V, RECOMBINED_Q8_TOL)
    # LRT and l0 are values at an optimum and compare run against run. beta, se and F are taken at each run's own l_remle, and the
    # optimum is flat: two correct searches may stop 1e-7 apart in log lambda, which moves beta by 1e-6 (the float64 models do, run
    # against run). As everywhere in these modules they are compared at the tool's own lambdas: each run against model G of the
    # OTHER basis at this run's l_remle. The run-against-run differences are printed.
    dev = dict(lrt=np.abs(a["lrt"] - b["lrt"]).max(), l0=abs(a["l0"] - b["l0"]))
    for name, out, other in (("W", a, WA), ("W A", b, W)):
        d = statistic_deviations(K, other, y, 2.0 * V[:12], first(out, 12))
        dev.update({"%s of the run on %s" % (k, name): d[k] for k in ("beta", "se", "F")})
    Fa, Fb = (a["beta"] / a["se"]) ** 2, (b["beta"] / b["se"]) ** 2
    print("W against W A: %s (allowed %.1e); run against run at their own l_remle: beta %.3e, se %.3e, F %.3e, log l_remle %.3e"
          % (", ".join("%s %.3e" % kv for kv in dev.items()), INVARIANCE_TOL, np.abs(b["beta"] / a["beta"] - 1).max(),
             np.abs(b["se"] / a["se"] - 1).max(), np.abs(Fb / Fa - 1).max(), np.abs(np.log(b["lam_remle"] / a["lam_remle"])).max()))
    assert max(dev.values()) <= INVARIANCE_TOL
    assert abs(a["null_reml"][0] - b["null_reml"][0]) > 1.0, "the REML value is reported for W as given: log |det A| must show"


# ---- 5. two interior maxima, with covariates ----

@pytest.mark.parametrize("n,seed,q", CV.TWO_PEAK_W_CASES)
def test_two_interior_maxima(n, seed, q):
    """test_lmm_covar_model.py asserts that 87 ML models of these cases have two interior maxima (all 17 of each n = 67 case), > 1e-6
    apart in l (typically 0.05 .. 40). Had the search on CovModel returned the wrong peak, model R would lose that at the tool's lambda."""
    K, y, W, V = CV.two_peak_case(n, seed, q)
    xs = 2.0 * V
    out = run(K, W, y, M.presence_bed(V))
    name = "two-peak n=%d seed=%d q=%d" % (n, seed, q)
    check_lrt_family(name, K, W, y, xs, out, True, dict(lrt=TWO_PEAK_LRT_TOL))
    worst = max(M.fit_R(K, y, CV.design(W, x))[0] - CV.loglik_R_at(K, y, W, x, lam) for x, lam in zip(xs, out["lam"]))
    worst0 = M.fit_R(K, y, CV.design(W))[0] - CV.loglik_R_at(K, y, W, None, out["lam0"])
    print("%s: model R loses at most %.3e at the tool's lambda over all 16 variants and %.3e at lambda0 (allowed %.1e)" % (name, worst, worst0, LRT_TOL))
    assert worst <= LRT_TOL and worst0 <= LRT_TOL


@pytest.mark.parametrize("n,seed,q", [c for c in CV.TWO_PEAK_W_CASES if c[0] == 67])
def test_two_reml_maxima(n, seed, q):
    """All 17 REML models of each of these cases have two interior maxima. Model G's V = lambda K + I is well enough conditioned on
    all four (test_lmm_covar_model.py measures its gap to model R' per case and asserts it <= 1e-9): model G is the reference."""
    K, y, W, V = CV.two_peak_case(n, seed, q)
    xs = 2.0 * V
    gap = MEASURED_TWO_PEAK_W_G_GAPS[(n, seed, q)]
    assert gap <= TWO_PEAK_G_MAX
    bed = M.presence_bed(V)
    out = run(K, W, y, bed, all_tests=True)
    name = "two-peak -lmm 4 n=%d seed=%d q=%d" % (n, seed, q)
    assert out["tested"].all() and same_bits(out, run(K, W, y, bed))
    tol = min(1e-8, 1000 * gap)
    check_statistics_family(name, K, W, y, xs, out, dict(beta=tol, se=tol, F=tol, reml=REML_TOL, vgve=tol))
    worst = max(CV.fit_reml_R(K, y, W, x)[0] - CV.reml_R_at(K, y, W, x, lam) for x, lam in zip(xs, out["lam_remle"]))
    print("%s: model R' loses at most %.3e at the tool's l_remle over all 16 variants (allowed %.1e)" % (name, worst, REML_TOL))
    assert worst <= REML_TOL


# ---- 6. a variant inside span(W) ----

def nan_or(a, ok):
    a = np.asarray(a)
    with np.errstate(invalid="ignore"):
        return bool((np.isnan(a) | ok(a)).all())


@functools.lru_cache(maxsize=None)
def span_case(q):
    n = 67
    K, y0, V, b = CV.span_panel(n, ROWS[n])
    W = CV.covariates(n, ROWS[n], "batch") if q == 2 else CV.width(n, ROWS[n], q)
    return K, CV.phenotype(y0, W), W, V


@pytest.mark.parametrize("all_tests", [False, True], ids=["test_bed", "test_bed_all"])
def test_variant_in_span_of_W(all_tests):
    """W = [1, b]: the rows b, 1 - b and b again (the last behind the chunk boundary) have x in span(W), so xx.w and xy.w are
    rounding. The call succeeds (run raises unless it returns KGWAS_OK), the ordinary rows keep the bits of a run without the three,
    and no statistic of the three looks like a hit: each is NaN or says nothing."""
    K, y, W, V = span_case(2)
    deg = np.zeros(CV.SPAN_ROWS, bool)
    deg[list(CV.SPAN_DEGENERATE)] = True
    keys = ALL_KEYS if all_tests else LRT_KEYS
    out = run(K, W, y, M.presence_bed(V), chunk=32, all_tests=all_tests)
    without = run(K, W, y, M.presence_bed(V[~deg]), chunk=32, all_tests=all_tests)
    assert same_bits({k: out[k][~deg] for k in keys}, without, keys), "a degenerate neighbour changes an ordinary row"
    assert (out["l0"], out["lam0"]) == (without["l0"], without["lam0"])
    print("x in span(W) (%s): lrt %s, p %s%s" % ("test_bed_all" if all_tests else "test_bed", out["lrt"][deg], out["p"][deg],
          ", beta %s, se %s, p_wald %s, p_score %s" % tuple(out[k][deg] for k in ("beta", "se", "p_wald", "p_score")) if all_tests else ""))
    assert nan_or(out["lrt"][deg], lambda a: a <= LRT_TOL)
    assert nan_or(out["p"][deg], lambda a: a >= 1 - 1e-6)
    if all_tests:
        assert nan_or(out["p_wald"][deg], lambda a: a >= 0.5) and nan_or(out["p_score"][deg], lambda a: a >= 0.5)
    # the ordinary rows are what the models say
    sub = {k: (v[~deg] if isinstance(v, np.ndarray) else v) for k, v in out.items()}
    assert sub["tested"].all()
    check_lrt("n=67 W=[1, b], the ordinary rows", K, W, y, 2.0 * V[~deg], sub, model_E=False)


@pytest.mark.parametrize("all_tests", [False, True], ids=["test_bed", "test_bed_all"])
def test_variant_outside_span_of_W_control(all_tests):
    """The same panel under width q = 4: the three rows are not in span(W) and are tested like any other"""
    K, y, W, V = span_case(4)
    out = run(K, W, y, M.presence_bed(V), chunk=32, all_tests=all_tests)
    assert out["tested"].all()
    check_lrt_family("n=67 q=4, the span panel", K, W, y, 2.0 * V, out, True, WIDTHS_TOL)
    if all_tests:
        d = list(CV.SPAN_DEGENERATE)
        assert np.isfinite(np.stack([out[k] for k in STATS])).all()
        sub = {k: (v[d] if isinstance(v, np.ndarray) else v) for k, v in out.items()}
        check_statistics_family("n=67 q=4, the rows b, 1 - b, b", K, W, y, 2.0 * V[d], sub, WIDTHS_TOL)
        assert out["lrt"][d[0]] == out["lrt"][d[2]] and out["beta"][d[0]] == out["beta"][d[2]]


def _write_panel(base, V, ids, y):
    """PLINK files of presence rows V whose .bim names are ids, so that a row's line is the same in a panel without its neighbours"""
    open(base + ".bed", "wb").write(bytes([0x6C, 0x1B, 0x01]) + M.presence_bed(V).tobytes())
    open(base + ".bim", "w").write("".join("1\tv%d\t0\t%d\tA\tC\n" % (v, 100 + v) for v in ids))
    open(base + ".fam", "w").write("".join("f%d i%d 0 0 0 %s\n" % (i, i, repr(float(p))) for i, p in enumerate(y)))
    return base


@pytest.mark.parametrize("mode", ["2", "4"])
def test_cli_variant_in_span_of_W(tmp_path, mode):
    """The files do not break on the three rows: exit 0 (_tool asserts it), every numeric field of every line parses, and the
    ordinary rows' lines are the bytes of a run on the panel without the three"""
    K, y, W, V = span_case(2)
    deg = np.zeros(CV.SPAN_ROWS, bool)
    deg[list(CV.SPAN_DEGENERATE)] = True
    ids = np.arange(CV.SPAN_ROWS)
    full = _write_panel(str(tmp_path / "full"), V, ids, y)
    plain = _write_panel(str(tmp_path / "plain"), V[~deg], ids[~deg], y)
    cov, kin = _write_cov(str(tmp_path / "c.cov"), W), _write_kin(str(tmp_path / "k.kin"), K)
    out = str(tmp_path / "out")
    tail = ["-k", kin, "-c", cov, "-lmm", mode, "-outdir", out, "--chunk_variants", "32"]
    _tool(["-bfile", full, "-o", "full"] + tail)
    _tool(["-bfile", plain, "-o", "plain"] + tail)
    a, b = (open(os.path.join(out, "%s.assoc.txt" % s)).read().split("\n") for s in ("full", "plain"))
    assert a[-1] == "" and a[0] == b[0] and len(b) == 2 + (~deg).sum()
    names = {"v%d" % v for v in CV.SPAN_DEGENERATE}
    assert [l for l in a[1:-1] if l.split("\t")[1] not in names] == b[1:-1], "an ordinary row's line differs"
    n_fields = len(a[0].split("\t"))
    for l in a[1:-1]:
        f = l.split("\t")
        assert len(f) == n_fields
        for c, v in enumerate(f):
            if c not in (1, 4, 5):  # (rs, allele1, allele0)
                float(v)
        if f[1] in names:
            print("-lmm %s, %s: %s" % (mode, f[1], l))
