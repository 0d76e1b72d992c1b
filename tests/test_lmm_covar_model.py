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
The second half qualifies the fixtures of test_gpu_lmm_lrt_covar_widths.py the same way, family by family (every width, [1, leading
eigenvectors of K], a badly scaled recombination of eight columns, two-peaked likelihoods with covariates, rows inside span(W)),
under constants of their own: that module allows 1000 x its family's gaps, capped at 1e-8.
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


# ---- the fixtures of test_gpu_lmm_lrt_covar_widths.py. Each family's gaps are measured as above and recorded under names of their
# own (the constants above stay what they were); the GPU module allows min(1e-8, 1000 x its family's gap). ----

# width(n, rows, q), q = 4 .. 7, n = 67 and 241
MEASURED_WIDTHS_GAPS = dict(lrt=5.7e-13, beta=3.4e-12, se=2.5e-15, F=6.8e-12, reml=2.8e-13, vgve=2.3e-15)
# width(1135, ., 7) on strong_fixture(1135, 1400)
MEASURED_WIDTH_1135_GAPS = dict(lrt=1.9e-11, beta=1.3e-11, se=3.6e-15, F=2.5e-11, reml=4.5e-12, vgve=5.3e-15)
# eigen_q(67, 400, q), q = 4, 6, 8
MEASURED_EIGEN_Q_GAPS = dict(lrt=5.1e-12, beta=1.2e-10, se=1.2e-13, F=2.4e-10, reml=1.5e-12, vgve=3.7e-15)
# recombined_q8(67, 400)
MEASURED_RECOMBINED_Q8_GAPS = dict(lrt=7.4e-13, beta=1.9e-12, se=4.3e-14, F=3.7e-12, reml=4.8e-13, vgve=3.0e-15)
MEASURED_RECOMBINED_Q8_INVARIANCE = 4.4e-12  # width(67, 400, 8) against recombined_q8: LRT absolute, beta, se, F relative, either model
# two_peak_case(n, seed, q): LRT and l0, model R against model E, at their own optima
MEASURED_TWO_PEAK_W_LRT_GAP = 4.5e-12
# the two n = 67 fixtures, model R' against model G at model R''s REML optima (beta, se, F_wald, F_score relative; vg, ve relative)
MEASURED_TWO_PEAK_W_G_GAPS = {(67, 54, 2): 9.5e-14, (67, 54, 3): 1.2e-14, (67, 56, 2): 6.5e-12, (67, 56, 3): 4.5e-13}
TWO_PEAK_G_MAX = 1e-9  # past this gap model G is no reference for the fixture: the GPU test compares with model R' there


def _family_gaps(fixtures):
    """The models' gaps over (name, K, y, W, xs): LRT and l0 at the models' own optima, the rest at FIXED_LAMBDAS"""
    worst = dict(lrt=0.0, beta=0.0, se=0.0, F=0.0, reml=0.0, vgve=0.0)
    for name, K, y, W, xs in fixtures:
        g = dict.fromkeys(worst, 0.0)
        (r, l0r), (e, l0e) = CV.lrt_R(K, y, W, xs), CV.lrt_E(K, y, W, xs)
        g["lrt"] = max(float(np.abs(r - e).max()), abs(l0r - l0e))
        for lam in FIXED_LAMBDAS:
            g["reml"] = max(g["reml"], abs(CV.reml_R_at(K, y, W, None, lam) - CV.gls_G(K, y, W, None, lam)[3]))
            g["vgve"] = max(g["vgve"], *[_rel(a, b) for a, b in zip(CV.vg_ve_R(K, y, W, lam), CV.vg_ve_G(K, y, W, lam))])
            for x in xs:
                b, s, F, l = CV.gls_G(K, y, W, x, lam)
                b2, s2, F2 = CV.wald_R(K, y, W, x, lam)
                g["beta"], g["se"] = max(g["beta"], _rel(b2, b)), max(g["se"], _rel(s2, s))
                g["F"] = max(g["F"], _rel(F2, F), _rel(CV.score_R(K, y, W, x, lam), CV.score_G(K, y, W, x, lam)))
                g["reml"] = max(g["reml"], abs(CV.reml_R_at(K, y, W, x, lam) - l))
        print("%s: %s" % (name, " ".join("%s %.1e" % kv for kv in g.items())))
        assert max(g.values()) <= GAP_MAX, name
        for k in worst:
            worst[k] = max(worst[k], g[k])
    return worst


def _report(family, worst, recorded):
    print("%s: largest gaps %s (recorded: %s)" % (family, " ".join("%s %.1e" % kv for kv in worst.items()),
                                                  " ".join("%s %.1e" % kv for kv in recorded.items())))


def _width_like(W_of, sizes, qs):
    for n, rows in sizes:
        G, K, y0 = M.fixture(n, rows, 3.0)
        xs = 2.0 * M.varying(G)[:N_VARIANTS]
        for q in qs:
            W = W_of(n, rows, q)
            yield "n=%d q=%d" % (n, q), K, CV.phenotype(y0, W), W, xs


def test_width_fixtures():
    _report("width q = 4 .. 7", _family_gaps(_width_like(CV.width, SIZES, (4, 5, 6, 7))), MEASURED_WIDTHS_GAPS)


def test_width_fixture_at_the_real_panel_width():
    """q = 7 at n = 1135 on the strong panel (the GPU module runs -lmm 4 there against model R'): the causal variant and one of each
    kind of the others, since model E and model G cost an eigendecomposition and a Cholesky factor of 1135 x 1135 each time"""
    n = 1135
    K, base, g, V = M.strong_fixture(n, M.STRONG_ROWS[n], nv=12)
    W = CV.width(n, 600, 7)
    _report("width q = 7, n = 1135", _family_gaps([("n=1135 q=7", K, CV.phenotype(base + 10.0 * g, W), W, 2.0 * V[[0, 1, 5, 9]])]), MEASURED_WIDTH_1135_GAPS)


def test_eigen_q_fixtures():
    assert CV.eigen_q(67, 400, 3).tobytes() == CV.covariates(67, 400, "eigen").tobytes()
    _report("eigen_q q = 4, 6, 8", _family_gaps(_width_like(CV.eigen_q, SIZES[:1], (4, 6, 8))), MEASURED_EIGEN_Q_GAPS)


def test_recombined_q8_fixture():
    """The recombination matrix is badly scaled but nowhere near the tool's rank refusal (a remainder of 1e-8 of a column's norm);
    the models pass on W A, and nothing but the REML value moves against W."""
    n, rows = SIZES[0]
    cond = np.linalg.cond(CV.RECOMBINE_Q8)
    W, WA = CV.width(n, rows, 8), CV.recombined_q8(n, rows)
    print("cond(RECOMBINE_Q8) = %.3e, cond(W A) = %.3e" % (cond, np.linalg.cond(WA)))
    assert 1e4 <= cond <= 1e6 and np.linalg.cond(WA) <= 1e6
    G, K, y0 = M.fixture(n, rows, 3.0)
    xs = 2.0 * M.varying(G)[:N_VARIANTS]
    y = CV.phenotype(y0, W)
    _report("recombined_q8", _family_gaps([("n=%d W A" % n, K, y, WA, xs)]), MEASURED_RECOMBINED_Q8_GAPS)
    (a, l0a), (b, l0b) = CV.lrt_R(K, y, W, xs), CV.lrt_R(K, y, WA, xs)
    (c, _), (d, _) = CV.lrt_E(K, y, W, xs[:2]), CV.lrt_E(K, y, WA, xs[:2])
    g = max(float(np.abs(a - b).max()), abs(l0a - l0b), float(np.abs(c - d).max()))
    for lam in FIXED_LAMBDAS:
        g = max(g, *[_rel(p, q) for p, q in zip(CV.vg_ve_G(K, y, W, lam), CV.vg_ve_G(K, y, WA, lam))])
        for x in xs:
            for f in (CV.gls_G, CV.wald_R):
                g = max(g, *[_rel(p, q) for p, q in zip(f(K, y, W, x, lam)[:3], f(K, y, WA, x, lam)[:3])])
            g = max(g, _rel(CV.score_G(K, y, W, x, lam), CV.score_G(K, y, WA, x, lam)), _rel(CV.score_R(K, y, W, x, lam), CV.score_R(K, y, WA, x, lam)))
    print("width q = 8 against recombined_q8: within %.1e (MEASURED_RECOMBINED_Q8_INVARIANCE %.1e)" % (g, MEASURED_RECOMBINED_Q8_INVARIANCE))
    assert g <= GAP_MAX


TWO_PEAK_W_GAP_MAX = 1e-10  # test_lmm_lrt_model.py's NEW_GAP_MAX: a fixture past it is replaced by another seed, not tolerated


def test_two_peak_fixtures_with_covariates():
    """What test_lmm_lrt_model.py and test_lmm_wald_model.py assert of the two-peaked fixtures, with covariates in the design: over
    H0 and the 16 H1 designs of every case, models with two interior maxima on the 2001-point grid exist in numbers, under both
    objectives and with either peak the larger one; the peaks are >= 1.0 apart in log lambda and > 1e-6 apart in l. The models' gap
    on every case is within TWO_PEAK_W_GAP_MAX; model G's gap at model R''s REML optima is measured per n = 67 case."""
    two = {False: 0, True: 0}
    first = {False: 0, True: 0}
    last = {False: 0, True: 0}
    worst = 0.0
    for n, seed, q in CV.TWO_PEAK_W_CASES:
        K, y, W, V = CV.two_peak_case(n, seed, q)
        xs = 2.0 * V
        (r, l0r), (e, l0e) = CV.lrt_R(K, y, W, xs), CV.lrt_E(K, y, W, xs)
        gap = max(float(np.abs(r - e).max()), abs(l0r - l0e))
        worst = max(worst, gap)
        counts = {False: [], True: []}
        for x in [None] + list(xs):
            for reml in (False, True):
                pk = CV.interior_maxima(K, y, CV.design(W, x), reml)
                counts[reml].append(len(pk))
                if len(pk) != 2:
                    continue
                two[reml] += 1
                assert abs(pk[0][1] - pk[1][1]) > 1e-6 and pk[1][0] - pk[0][0] >= 1.0, (n, seed, q, reml, pk)
                first[reml] += pk[0][1] > pk[1][1]
                last[reml] += pk[1][1] > pk[0][1]
        print("two-peak n=%d seed=%d q=%d: model R against model E within %.1e; models with two maxima: ML %d, REML %d of 17"
              % (n, seed, q, gap, sum(c == 2 for c in counts[False]), sum(c == 2 for c in counts[True])))
        assert gap <= TWO_PEAK_W_GAP_MAX, (n, seed, q)
        if n == 67:
            assert all(c == 2 for c in counts[False]), "an ML model of an n = 67 case has lost its second peak"
            g = 0.0
            for x in xs:
                lam, lam0 = CV.fit_reml_R(K, y, W, x)[1], M.fit_R(K, y, W)[1]
                g = max(g, *[_rel(a, b) for a, b in zip(CV.wald_R(K, y, W, x, lam), CV.gls_G(K, y, W, x, lam)[:3])],
                        _rel(CV.score_R(K, y, W, x, lam0), CV.score_G(K, y, W, x, lam0)))
            lam = CV.fit_reml_R(K, y, W, None)[1]
            g = max(g, *[_rel(a, b) for a, b in zip(CV.vg_ve_R(K, y, W, lam), CV.vg_ve_G(K, y, W, lam))])
            print("  model R' against model G at model R''s optima: within %.1e (recorded %.1e)" % (g, MEASURED_TWO_PEAK_W_G_GAPS[(n, seed, q)]))
            assert g <= TWO_PEAK_G_MAX, "model G is no reference for this fixture any more: the GPU test compares with it"
    print("two interior maxima: ML %d models (first peak the larger %d, last %d), REML %d (%d, %d); largest gap %.1e (MEASURED_TWO_PEAK_W_LRT_GAP %.1e)"
          % (two[False], first[False], last[False], two[True], first[True], last[True], worst, MEASURED_TWO_PEAK_W_LRT_GAP))
    assert two[False] >= 40 and two[True] >= 20
    assert min(first[False], last[False], first[True], last[True]) >= 5


def test_span_panel():
    """The three degenerate rows lie in span([1, b]) and not in span of width(67, 400, 4); no ordinary row lies in either"""
    n, rows = SIZES[0]
    K, y0, V, b = CV.span_panel(n, rows)
    assert V.shape == (CV.SPAN_ROWS, n) and len(M.varying(V)) == CV.SPAN_ROWS
    for W, inside in ((CV.covariates(n, rows, "batch"), True), (CV.width(n, rows, 4), False)):
        Q, _ = CV.orthonormal(W)
        rem = np.array([np.linalg.norm(x - Q @ (Q.T @ x)) / np.linalg.norm(x) for x in 2.0 * V])
        deg = np.zeros(CV.SPAN_ROWS, bool)
        deg[list(CV.SPAN_DEGENERATE)] = True
        assert (rem[~deg] > 0.1).all()
        assert (rem[deg] < 1e-14).all() if inside else (rem[deg] > 0.1).all()
