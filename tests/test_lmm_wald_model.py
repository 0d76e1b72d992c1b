"""lmm_lrt -lmm 4 without a GPU: the two numpy models of lmm_wald_np.py against each other, the REML peaks of the two-peaked
fixtures, and the F(1, df) tail the Wald and score tests share (kgwas_fdist_tail, the host instance of the kernel's function).

Measured here (float64, -lmin / -lmax = e^-10 / e^10; fixture(67, 400, hg) and fixture(241, 600, hg) at hg 0 and 3, strong_fixture(241)
at the effects 3, 10 and 40, every TWO_PEAK_CASES fixture; 8 variants each):
  at the fixed lambdas e^-4, 1 and e^3, model R' against model G: beta within 8.5e-11, se within 2.7e-12, F_wald and F_score
  within 1.7e-10, all relative; the REML value within 8.9e-11 absolute. The largest are on the two-peaked fixtures at n = 67, whose
  K has eigenvalues up to e^8: V = lambda K + I has a condition number of 6e4 .. 6e7 there, which is model G's Cholesky factor's error,
  not a difference of the formulas (the other fixtures stay under 1e-12, se under 1e-14).
  at the models' own optima (H0 and 2 variants each; a Cholesky factor per grid point): the REML maxima agree to 6.8e-13, log l_remle
  to 2.5e-6 (the optimum is flat: an error dt costs l'' dt^2 / 2), and beta, se, F, which move with log lambda at first order, to
  1.6e-6, 4.1e-8 and 3.3e-6 relative. That is why the GPU module compares beta, se and F at the tool's own lambda.
The GPU module (test_gpu_lmm_lrt_wald.py) allows 1000 x the fixed-lambda gaps, capped at 1e-8.

The tail: against 2 t.sf(sqrt(F), df) over df in {3 .. 65533} and 400 values of F the largest relative error is 3.8e-12, at
df = 65533 and F = 5.7 (fdist_tail.h says where it comes from); 2.4e-13 up to df = 1133.
"""
import numpy as np
import pytest
from scipy.stats import t as student_t

from kmersgwas_amd.capi import lib

import lmm_lrt_np as M
import lmm_wald_np as W

# largest gaps between model R' and model G at fixed lambdas (printed by test_model_gaps)
MEASURED_BETA_GAP = 8.5e-11   # relative
MEASURED_SE_GAP = 2.7e-12     # relative
MEASURED_F_GAP = 1.7e-10      # relative; F_wald and F_score
MEASURED_REML_GAP = 8.9e-11   # absolute
# and at the models' own optima
MEASURED_REML_GAP_AT_OPTIMA = 6.8e-13
MEASURED_LOG_LAMBDA_GAP_AT_OPTIMA = 2.5e-6
MEASURED_BETA_GAP_AT_OPTIMA, MEASURED_SE_GAP_AT_OPTIMA, MEASURED_F_GAP_AT_OPTIMA = 1.6e-6, 4.1e-8, 3.3e-6
MEASURED_VG_VE_GAP = 6.0e-15  # relative; emma.REMLE's vg and ve against model G's at fixed lambdas (printed by test_null_model_by_reml)
MEASURED_TAIL_RELERR = 3.8e-12  # largest |kgwas_fdist_tail / (2 t.sf(sqrt(F), df)) - 1| (printed by test_fdist_tail)

GAP_MAX = 1e-9        # a tenth of the GPU tolerances' cap of 1e-8, as test_lmm_lrt_model.py's test_models_agree asserts its gap
OPTIMA_MAX = 1e-4     # beta, se, F at the models' own optima: they carry the location error of a flat optimum (about 1e-6 in log
                      # lambda) at first order; a wrong peak is >= 1.0 away in log lambda (test_lmm_lrt_model.py) and moves them by far more
FIXED_LAMBDAS = (float(np.exp(-4.0)), 1.0, float(np.exp(3.0)))
N_VARIANTS, N_AT_OPTIMA = 8, 2


def gap_cases():
    for n, rows in ((67, 400), (241, 600)):
        for hg in (0.0, 3.0):
            G, K, y = M.fixture(n, rows, hg)
            yield "fixture n=%d hg=%g" % (n, hg), K, y, M.varying(G)[:N_VARIANTS].astype(np.float64)
    K, base, g, V = M.strong_fixture(241, M.STRONG_ROWS[241])
    for effect in M.STRONG_EFFECTS:
        yield "strong n=241 effect=%g" % effect, K, base + effect * g, V[:N_VARIANTS].astype(np.float64)
    for n, seed in M.TWO_PEAK_CASES:
        K, y, X = M.two_peak_fixture(n, seed, M.two_peak_rows(n))
        yield "two-peak n=%d seed=%d" % (n, seed), K, y, X[:N_VARIANTS].astype(np.float64)


def _rel(a, b):
    return abs(a - b) / abs(b)


def test_model_gaps():
    worst = dict(beta=0.0, se=0.0, F=0.0, reml=0.0)
    worst_opt = dict(beta=0.0, se=0.0, F=0.0, reml=0.0, loglam=0.0)
    for name, K, y, xs in gap_cases():
        g = dict(beta=0.0, se=0.0, F=0.0, reml=0.0)
        for lam in FIXED_LAMBDAS:
            g["reml"] = max(g["reml"], abs(W.reml_R_at(K, y, None, lam) - W.gls_G(K, y, None, lam)[3]))
            for x in xs:
                b, s, F, l = W.gls_G(K, y, x, lam)
                b2, s2, F2 = W.wald_R(K, y, x, lam)
                g["beta"] = max(g["beta"], _rel(b2, b))
                g["se"] = max(g["se"], _rel(s2, s))
                g["F"] = max(g["F"], _rel(F2, F), _rel(W.score_R(K, y, x, lam), W.score_G(K, y, x, lam)))
                g["reml"] = max(g["reml"], abs(W.reml_R_at(K, y, x, lam) - l))
        o = dict(beta=0.0, se=0.0, F=0.0, reml=0.0, loglam=0.0)
        for x in [None] + list(xs[:N_AT_OPTIMA]):
            lg, lam_g = W.fit_reml_G(K, y, x)
            lr, lam_r = W.fit_reml_R(K, y, x)
            o["reml"] = max(o["reml"], abs(lr - lg))
            o["loglam"] = max(o["loglam"], abs(np.log(lam_r / lam_g)))
            if x is not None:
                b, s, F, _ = W.gls_G(K, y, x, lam_g)
                b2, s2, F2 = W.wald_R(K, y, x, lam_r)
                o["beta"], o["se"], o["F"] = max(o["beta"], _rel(b2, b)), max(o["se"], _rel(s2, s)), max(o["F"], _rel(F2, F))
        print("%s: fixed lambdas %s; own optima %s" % (name, " ".join("%s %.1e" % kv for kv in g.items()), " ".join("%s %.1e" % kv for kv in o.items())))
        assert max(g.values()) <= GAP_MAX, name
        assert o["reml"] <= GAP_MAX and o["loglam"] <= OPTIMA_MAX and max(o["beta"], o["se"], o["F"]) <= OPTIMA_MAX, name
        for k in worst:
            worst[k] = max(worst[k], g[k])
        for k in worst_opt:
            worst_opt[k] = max(worst_opt[k], o[k])
    print("largest gaps at fixed lambdas: %s (MEASURED_BETA_GAP %.1e, MEASURED_SE_GAP %.1e, MEASURED_F_GAP %.1e, MEASURED_REML_GAP %.1e)"
          % (" ".join("%s %.1e" % kv for kv in worst.items()), MEASURED_BETA_GAP, MEASURED_SE_GAP, MEASURED_F_GAP, MEASURED_REML_GAP))
    print("largest gaps at the own optima: %s" % " ".join("%s %.1e" % kv for kv in worst_opt.items()))


def test_reml_peaks_of_the_two_peak_fixtures():
    """Model R''s interior REML maxima on its 2001-point grid, for H0 and every variant's H1 of every TWO_PEAK_CASES fixture with
    two_peak_rows(n) rows. A GPU test on a fixture without a second REML peak shows nothing about the candidate rule: the fixtures
    test_gpu_lmm_lrt_wald.py runs are asserted here to have one."""
    models = two_peaked = first = last = 0
    per_fixture = {}
    for n, seed in M.TWO_PEAK_CASES:
        K, y, X = M.two_peak_fixture(n, seed, M.two_peak_rows(n))
        counts = []
        for x in [None] + list(X.astype(np.float64)):
            pk = W.interior_reml_maxima(K, y, x)
            counts.append(len(pk))
            if len(pk) == 2:
                win = int(np.argmax([l for _, l in pk]))
                first += win == 0
                last += win == 1
        per_fixture[(n, seed)] = (len(counts), sum(c == 2 for c in counts))
        models += len(counts)
        two_peaked += sum(c == 2 for c in counts)
        assert max(counts) <= 2
        print("n=%d seed=%d: %d models, %d with two interior REML maxima" % (n, seed, len(counts), per_fixture[(n, seed)][1]))
    print("%d models, %d two-peaked: the first peak is the larger in %d, the last in %d" % (models, two_peaked, first, last))
    assert (models, two_peaked, first, last) == (351, 131, 64, 67)
    assert per_fixture[(16, 148)][1] == 0
    assert per_fixture[(8, 36)] == (65, 64) and per_fixture[(67, 56)] == (17, 17)
    assert per_fixture[(8, 18)][1] >= 8 and per_fixture[(67, 54)] == (17, 17)


def test_null_model_by_reml():
    """vg and ve: the restatement of emma.REMLE against model G's s^2 at fixed lambdas (MEASURED_VG_VE_GAP, relative), emma's REML
    likelihood against model R''s up to its constant, and the phenotype whose REML optimum is the lower end of the range."""
    worst = worst_ll = 0.0
    for n, rows in ((67, 400), (241, 600)):
        for hg in (0.0, 3.0):
            G, K, y = M.fixture(n, rows, hg)
            lams = np.array(FIXED_LAMBDAS)
            diff = W.emma_reml_ll(K, y, lams) - np.array([W.reml_R_at(K, y, None, L) for L in lams])
            worst_ll = max(worst_ll, float(np.abs(diff - diff[0]).max()))
            for lam in FIXED_LAMBDAS:
                (vg, ve), (vg_g, ve_g) = W.emma_vg_ve(K, y, lam), W.vg_ve_G(K, y, lam)
                worst = max(worst, _rel(vg, vg_g), _rel(ve, ve_g))
        y = W.noise_phenotype(n)
        lr, lam = W.fit_reml_R(K, y, None)
        assert lam == pytest.approx(M.LMIN, rel=1e-12) and not W.interior_reml_maxima(K, y, None), n
    print("vg, ve: emma.REMLE's against model G's within %.1e relative (MEASURED_VG_VE_GAP = %.1e); emma's REML likelihood differs from "
          "model R''s by a constant to %.1e" % (worst, MEASURED_VG_VE_GAP, worst_ll))
    assert worst <= GAP_MAX and worst_ll <= GAP_MAX


TAIL_DFS = (3, 4, 6, 14, 65, 239, 1133, 5998, 65533)
TINY = 2.3e-308


def test_fdist_tail():
    """Against 2 t.sf(sqrt(F), df), which agrees with a 40-digit evaluation to 2e-15 (scipy.stats.f.sf does not: 1.3e-8 off at
    df = 65533, F = 1e-8). Where the reference is below the normal doubles a relative error says nothing: 0 <= p <= 2.3e-308 there."""
    F = np.logspace(-8, np.log10(2e4), 400)
    worst, below = 0.0, 0
    for df in TAIL_DFS:
        ref = 2.0 * student_t.sf(np.sqrt(F), df)
        p = np.array([lib.kgwas_fdist_tail(float(f), float(df)) for f in F])
        normal = ref >= TINY
        rel = np.abs(p[normal] / ref[normal] - 1.0)
        print("df=%d: largest relative error %.3e at F=%.4g; %d points below the normal doubles" % (df, rel.max(), F[normal][rel.argmax()], (~normal).sum()))
        assert ((p[~normal] >= 0) & (p[~normal] <= TINY)).all()
        assert (np.diff(p) <= 0).all(), "the tail is not monotone in F"
        below += int((~normal).sum())
        worst = max(worst, float(rel.max()))
        assert lib.kgwas_fdist_tail(0.0, float(df)) == 1.0
    tol = min(1e-9, 10 * MEASURED_TAIL_RELERR)
    print("largest relative error %.3e (MEASURED_TAIL_RELERR = %.1e, allowed %.1e); %d points below the normal doubles" % (worst, MEASURED_TAIL_RELERR, tol, below))
    assert worst <= tol and below > 0
    assert np.isnan(lib.kgwas_fdist_tail(float("nan"), 5.0)) and lib.kgwas_fdist_tail(float("inf"), 5.0) == 0.0
