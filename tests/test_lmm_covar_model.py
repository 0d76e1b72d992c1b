"""lmm_lrt with covariates without a GPU: the numpy models of lmm_covar_np.py against each other, and their invariance to W -> W A.

Measured here (float64, -lmin / -lmax = e^-10 / e^10; fixture(67, 400, 3) and fixture(241, 600, 3) with every form of W of
lmm_covar_np.FORMS, the phenotype carrying an effect of every covariate; 4 variants each):
  the ML LRT and l0, model R against model E at their own optima: within 3.8e-12 (the form "eigen" at n = 67);
  at the fixed lambdas e^-4, 1 and e^3, model R' against model G: beta within 9.3e-12, se within 1.2e-13, F_wald and F_score within
  1.9e-11, vg and ve within 4.3e-15, all relative; the REML value within 1.3e-12 absolute;
  at the models' own REML optima (n = 67, H0 and 2 variants): the maxima within 5.7e-14;
  W against W A and against its orthonormal basis: every statistic within 1.4e-12; the REML value moves by log |det R|.
Every gap is asserted to stay under 1e-9; the constants record what was measured.
The GPU module (test_gpu_lmm_lrt_covar.py) allows 1000 x these gaps, capped at 1e-8.
"""
import numpy as np
import pytest

import lmm_lrt_np as M
import lmm_covar_np as CV

# largest gaps between the models (printed by the tests below)
MEASURED_LRT_GAP = 3.8e-12    # absolute; model R against model E, LRT and l0
MEASURED_BETA_GAP = 9.3e-12   # relative; model R' against model G at fixed lambdas
MEASURED_SE_GAP = 1.2e-13     # relative
MEASURED_F_GAP = 1.9e-11      # relative; F_wald and F_score
MEASURED_REML_GAP = 1.3e-12   # absolute
MEASURED_VG_VE_GAP = 4.3e-15  # relative
MEASURED_REML_GAP_AT_OPTIMA = 5.7e-14
MEASURED_INVARIANCE_GAP = 1.4e-12 # W against W A: LRT absolute, beta, se, F relative, in either model

GAP_MAX = 1e-9  # a tenth of the GPU tolerances' cap of 1e-8, as test_lmm_wald_model.py asserts its gaps
FIXED_LAMBDAS = (float(np.exp(-4.0)), 1.0, float(np.exp(3.0)))
SIZES = ((67, 400), (241, 600))
N_VARIANTS, N_AT_OPTIMA = 4, 2


def cases():
    for n, rows in SIZES:
        G, K, y = M.fixture(n, rows, 3.0)
        xs = 2.0 * M.varying(G)[:N_VARIANTS]
        for form in CV.FORMS:
            W = CV.covariates(n, rows, form)
            yield "n=%d %s" % (n, form), K, CV.phenotype(y, W), W, xs


def _rel(a, b):
    return abs(a - b) / abs(b)


def test_lrt_models_agree():
    worst = 0.0
    for name, K, y, W, xs in cases():
        (r, l0r), (e, l0e) = CV.lrt_R(K, y, W, xs), CV.lrt_E(K, y, W, xs)
        gap = max(float(np.abs(r - e).max()), abs(l0r - l0e))
        print("%s: LRT up to %.1f, model R against model E within %.1e" % (name, r.max(), gap))
        assert gap <= GAP_MAX, name
        worst = max(worst, gap)
    print("largest gap %.1e (MEASURED_LRT_GAP %.1e)" % (worst, MEASURED_LRT_GAP))


def test_wald_models_agree():
    worst = dict(beta=0.0, se=0.0, F=0.0, reml=0.0, vgve=0.0, reml_opt=0.0)
    for name, K, y, W, xs in cases():
        g = dict(beta=0.0, se=0.0, F=0.0, reml=0.0, vgve=0.0, reml_opt=0.0)
        for lam in FIXED_LAMBDAS:
            g["reml"] = max(g["reml"], abs(CV.reml_R_at(K, y, W, None, lam) - CV.gls_G(K, y, W, None, lam)[3]))
            g["vgve"] = max(g["vgve"], *[_rel(a, b) for a, b in zip(CV.vg_ve_R(K, y, W, lam), CV.vg_ve_G(K, y, W, lam))])
            for x in xs:
                b, s, F, l = CV.gls_G(K, y, W, x, lam)
                b2, s2, F2 = CV.wald_R(K, y, W, x, lam)
                g["beta"], g["se"] = max(g["beta"], _rel(b2, b)), max(g["se"], _rel(s2, s))
                g["F"] = max(g["F"], _rel(F2, F), _rel(CV.score_R(K, y, W, x, lam), CV.score_G(K, y, W, x, lam)))
                g["reml"] = max(g["reml"], abs(CV.reml_R_at(K, y, W, x, lam) - l))
        if y.size <= 67:  # (model G's optimum costs a Cholesky factor per grid point)
            for x in [None] + list(xs[:N_AT_OPTIMA]):
                g["reml_opt"] = max(g["reml_opt"], abs(CV.fit_reml_R(K, y, W, x)[0] - CV.fit_reml_G(K, y, W, x)[0]))
        print("%s: %s" % (name, " ".join("%s %.1e" % kv for kv in g.items())))
        assert max(g.values()) <= GAP_MAX, name
        for k in worst:
            worst[k] = max(worst[k], g[k])
    print("largest gaps: %s (MEASURED_BETA_GAP %.1e, MEASURED_SE_GAP %.1e, MEASURED_F_GAP %.1e, MEASURED_REML_GAP %.1e, MEASURED_VG_VE_GAP %.1e, "
          "MEASURED_REML_GAP_AT_OPTIMA %.1e)" % (" ".join("%s %.1e" % kv for kv in worst.items()), MEASURED_BETA_GAP, MEASURED_SE_GAP,
                                                 MEASURED_F_GAP, MEASURED_REML_GAP, MEASURED_VG_VE_GAP, MEASURED_REML_GAP_AT_OPTIMA))


def test_models_are_invariant_to_a_change_of_basis():
    """W and W A (the forms "normal" and "recombined"), and W against its orthonormal basis: the LRT, beta, se, F_wald, F_score,
    vg and ve do not move; the REML value moves by log |det R| exactly."""
    worst = 0.0
    for n, rows in SIZES:
        G, K, y0 = M.fixture(n, rows, 3.0)
        xs = 2.0 * M.varying(G)[:N_VARIANTS]
        W, WA = CV.covariates(n, rows, "normal"), CV.covariates(n, rows, "recombined")
        y = CV.phenotype(y0, W)
        Q, logdet = CV.orthonormal(WA)
        assert np.allclose(Q.T @ Q, np.eye(2), atol=1e-14) and np.allclose(Q @ (Q.T @ W), W, rtol=0, atol=1e-12)
        for other in (WA, Q):
            (a, l0a), (b, l0b) = CV.lrt_R(K, y, W, xs), CV.lrt_R(K, y, other, xs)
            (c, _), (d, _) = CV.lrt_E(K, y, W, xs[:2]), CV.lrt_E(K, y, other, xs[:2])
            g = max(float(np.abs(a - b).max()), abs(l0a - l0b), float(np.abs(c - d).max()))
            for lam in FIXED_LAMBDAS:
                g = max(g, *[_rel(p, q) for p, q in zip(CV.vg_ve_G(K, y, W, lam), CV.vg_ve_G(K, y, other, lam))])
                for x in xs:
                    for f in (CV.gls_G, CV.wald_R):
                        g = max(g, *[_rel(p, q) for p, q in zip(f(K, y, W, x, lam)[:3], f(K, y, other, x, lam)[:3])])
                    g = max(g, _rel(CV.score_G(K, y, W, x, lam), CV.score_G(K, y, other, x, lam)),
                            _rel(CV.score_R(K, y, W, x, lam), CV.score_R(K, y, other, x, lam)))
            worst = max(worst, g)
        lam = 1.0
        shift = CV.reml_R_at(K, y, Q, None, lam) - CV.reml_R_at(K, y, WA, None, lam)
        assert shift == pytest.approx(logdet, abs=1e-9) and abs(logdet) > 1.0
    print("W against W A and against its orthonormal basis: within %.1e (MEASURED_INVARIANCE_GAP %.1e)" % (worst, MEASURED_INVARIANCE_GAP))
    assert worst <= GAP_MAX


def test_a_left_out_covariate_shows():
    """The fixtures' phenotypes carry the covariates' effects: the LRT without W differs by far more than any tolerance."""
    for n, rows in SIZES:
        G, K, y0 = M.fixture(n, rows, 3.0)
        xs = 2.0 * M.varying(G)[:N_VARIANTS]
        W = CV.covariates(n, rows, "normal")
        y = CV.phenotype(y0, W)
        with_w, _ = CV.lrt_R(K, y, W, xs)
        without, _ = M.lrt_R(K, y, xs)
        assert np.abs(with_w - without).max() > 1e-3
