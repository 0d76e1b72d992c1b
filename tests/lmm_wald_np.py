"""Two float64 numpy models of what lmm_lrt -lmm 4 adds to the LRT: the REML likelihood of y = 1 a + x b + u + e, its maximiser
l_remle, the effect estimate beta with its standard error and the Wald statistic at l_remle, and the score statistic at the null
model's ML lambda. Neither takes the tool's route through sums and Schur complements. The fixtures are lmm_lrt_np.py's.

Model R' (rotated) follows model R of lmm_lrt_np.py: K = U diag(d) U^T, everything rotated by U^T, h_i = 1 / (lambda d_i + 1), the
h-weighted regression by lstsq on the sqrt(h)-scaled columns A, and
    lR(lambda) = df/2 (log(df / 2 pi) - 1) + 1/2 sum log h_i - 1/2 log |A^T A| - df/2 log RSS,  df = n - q,
with slogdet of the weighted Gram matrix. It is maximised with lmm_lrt_np.maximise (2000 intervals, then the bounded search).

Model G (generalised least squares) never rotates: V = lambda K + I = L L^T, X* = L^-1 X, y* = L^-1 y, beta by the normal equations of
X*, s^2 = r^T V^-1 r / df, se from (X^T V^-1 X)^-1, and
    lR(lambda) = -1/2 [df log(2 pi RSS / df) + df + log |V| + log |X^T V^-1 X|].
Its score statistic is n (x^T P0 y)^2 / ((x^T P0 x) (y^T P0 y)), P0 = V0^-1 - V0^-1 1 (1^T V0^-1 1)^-1 1^T V0^-1 at V0 = lambda0 K + I.

emma_vg_ve restates what the reference tree's src/R/emma.R (emma.REMLE with q = 1, emma.eigen.R.wo.Z) gives
transform_and_permute_phenotypes.R: the n - 1 leading eigenpairs of S (K + I) S, etas = vectors^T y, vg = sum etas^2 / (values +
delta) / (n - 1), ve = vg delta, delta = 1 / lambda; emma_reml_ll is its emma.delta.REML.LL.wo.Z.
"""
import numpy as np
from scipy.linalg import cho_solve, solve_triangular

import lmm_lrt_np as M

TWO_PI = 2 * np.pi


def design(y, x=None):
    one = np.ones(y.size)
    return one[:, None] if x is None else np.column_stack([one, x])


# ---- model R' ----

def reml_R(d, yt, Ct, lam):
    """lR(lambda) for rotated y and rotated covariates Ct (n x q); lam an array."""
    n, q = Ct.shape
    df = n - q
    out = np.empty(len(lam))
    for k, L in enumerate(lam):
        h = 1.0 / (L * d + 1.0)
        s = np.sqrt(h)
        A = Ct * s[:, None]
        beta, *_ = np.linalg.lstsq(A, yt * s, rcond=None)
        r = (yt - Ct @ beta) * s
        sign, logdet = np.linalg.slogdet(A.T @ A)
        assert sign > 0
        out[k] = 0.5 * df * (np.log(df / TWO_PI) - 1.0) + 0.5 * np.sum(np.log(h)) - 0.5 * logdet - 0.5 * df * np.log(r @ r)
    return out


def _reml_R_fast(d, yt, Ct, lam):
    """The same through the normal equations, vectorised over lam (the 2001-point grid); the bounded search uses reml_R."""
    n, q = Ct.shape
    df = n - q
    H = 1.0 / (lam[:, None] * d[None, :] + 1.0)
    G = np.einsum("mi,ia,ib->mab", H, Ct, Ct)
    b = np.einsum("mi,ia,i->ma", H, Ct, yt)
    beta = np.linalg.solve(G, b[:, :, None])[:, :, 0]
    rss = H @ (yt * yt) - np.einsum("ma,ma->m", beta, b)
    return 0.5 * df * (np.log(df / TWO_PI) - 1.0) + 0.5 * np.sum(np.log(H), axis=1) - 0.5 * np.linalg.slogdet(G)[1] - 0.5 * df * np.log(rss)


def _rotated(K, y, x):
    d, U = M.eig_of(K)
    return d, U.T @ y, U.T @ design(y, x)


def reml_R_at(K, y, x, lam):
    """Model R''s lR at one lambda, H1 (x given) or H0 (x None)."""
    d, yt, Ct = _rotated(K, y, x)
    return float(reml_R(d, yt, Ct, np.array([lam]))[0])


def fit_reml_R(K, y, x, lmin=M.LMIN, lmax=M.LMAX):
    """(lR, lambda) at model R''s REML optimum, H1 (x given) or H0 (x None)."""
    d, yt, Ct = _rotated(K, y, x)

    def f(t):
        return (_reml_R_fast if len(t) > 1 else reml_R)(d, yt, Ct, np.exp(t))

    v, t = M.maximise(f, np.log(lmin), np.log(lmax))
    lam = float(np.exp(t))
    return float(reml_R(d, yt, Ct, np.array([lam]))[0]), lam


def reml_grid_R(K, y, x, lmin=M.LMIN, lmax=M.LMAX):
    """lR on the 2001-point grid: (log lambda, lR)."""
    d, yt, Ct = _rotated(K, y, x)
    t = np.linspace(np.log(lmin), np.log(lmax), M.GRID + 1)
    return t, _reml_R_fast(d, yt, Ct, np.exp(t))


def wald_R(K, y, x, lam):
    """(beta, se, F_wald) of model R' at lambda."""
    d, yt, Ct = _rotated(K, y, x)
    s = np.sqrt(1.0 / (lam * d + 1.0))
    A = Ct * s[:, None]
    coef, *_ = np.linalg.lstsq(A, yt * s, rcond=None)
    r = (yt - Ct @ coef) * s
    df = y.size - 2
    se = np.sqrt(r @ r / df * np.linalg.inv(A.T @ A)[1, 1])
    return float(coef[1]), float(se), float((coef[1] / se) ** 2)


def score_R(K, y, x, lam0):
    """F_score of model R' at lambda0: x and y are regressed on the intercept under the weights, by lstsq."""
    d, yt, Ct = _rotated(K, y, x)
    s = np.sqrt(1.0 / (lam0 * d + 1.0))
    w = (Ct[:, 0] * s)[:, None]
    B = np.column_stack([Ct[:, 1] * s, yt * s])
    coef, *_ = np.linalg.lstsq(w, B, rcond=None)
    R = B - w @ coef
    return float(y.size * (R[:, 0] @ R[:, 1]) ** 2 / ((R[:, 0] @ R[:, 0]) * (R[:, 1] @ R[:, 1])))


# ---- model G ----

def _whiten(K, lam, *cols):
    L = np.linalg.cholesky(lam * K + np.eye(K.shape[0]))
    return L, [solve_triangular(L, c, lower=True) for c in cols]


def gls_G(K, y, x, lam):
    """(beta, se, F_wald, lR) of model G at lambda; x None: the null model, (None, None, None, lR0)."""
    X = design(y, x)
    n, q = X.shape
    df = n - q
    L, (Xs, ys) = _whiten(K, lam, X, y)
    XtX = Xs.T @ Xs
    coef = np.linalg.solve(XtX, Xs.T @ ys)
    r = ys - Xs @ coef
    rss = float(r @ r)
    logdet_V = 2.0 * np.sum(np.log(np.diag(L)))
    reml = -0.5 * (df * np.log(TWO_PI * rss / df) + df + logdet_V + np.linalg.slogdet(XtX)[1])
    if x is None:
        return None, None, None, float(reml)
    se = np.sqrt(rss / df * np.linalg.inv(XtX)[1, 1])
    return float(coef[1]), float(se), float((coef[1] / se) ** 2), float(reml)


def vg_ve_G(K, y, lam):
    """(vg, ve) of model G's null model at lambda: ve = s^2 = r^T V^-1 r / (n - 1), vg = lambda ve."""
    X = design(y)
    L, (Xs, ys) = _whiten(K, lam, X, y)
    r = ys - Xs @ np.linalg.solve(Xs.T @ Xs, Xs.T @ ys)
    ve = float(r @ r) / (y.size - 1)
    return lam * ve, ve


def score_G(K, y, x, lam0):
    n = y.size
    L = np.linalg.cholesky(lam0 * K + np.eye(n))
    one = np.ones(n)

    def P0(v):
        a, b = cho_solve((L, True), v), cho_solve((L, True), one)
        return a - b * (one @ a) / (one @ b)

    Py = P0(y)
    Px = P0(np.asarray(x, np.float64))
    return float(n * (x @ Py) ** 2 / ((x @ Px) * (y @ Py)))


def fit_reml_G(K, y, x, lmin=M.LMIN, lmax=M.LMAX):
    """(lR, lambda) at model G's own REML optimum (a Cholesky factor per point: use it at n <= 241)."""
    def f(t):
        return np.array([gls_G(K, y, x, float(np.exp(s)))[3] for s in t])

    v, t = M.maximise(f, np.log(lmin), np.log(lmax))
    return float(v), float(np.exp(t))


# ---- emma.REMLE, q = 1 ----

def _emma_eig_R(K, y):
    n = y.size
    S = np.eye(n) - np.ones((n, n)) / n
    w, V = np.linalg.eigh(S @ (K + np.eye(n)) @ S)
    values, vectors = w[1:] - 1.0, V[:, 1:]  # the n - 1 largest
    return values, vectors.T @ y


def emma_vg_ve(K, y, lam):
    values, etas = _emma_eig_R(K, y)
    delta = 1.0 / lam
    vg = float(np.sum(etas * etas / (values + delta)) / (y.size - 1))
    return vg, vg * delta


def emma_reml_ll(K, y, lam):
    """emma.delta.REML.LL.wo.Z at delta = 1 / lambda; lam an array."""
    values, etas = _emma_eig_R(K, y)
    nq = etas.size
    delta = 1.0 / np.atleast_1d(lam)[:, None]
    return 0.5 * (nq * (np.log(nq / TWO_PI) - 1.0 - np.log(np.sum(etas * etas / (values[None, :] + delta), axis=1)))
                  - np.sum(np.log(values[None, :] + delta), axis=1))


def interior_reml_maxima(K, y, x):
    """The interior local maxima of model R''s lR on its 2001-point grid: [(log lambda, lR)], in grid order."""
    t, v = reml_grid_R(K, y, x)
    return [(float(t[i]), float(v[i])) for i in range(1, M.GRID) if v[i] > v[i - 1] and v[i] >= v[i + 1]]


# ---- a phenotype without a heritable part ----

NOISE_SEED = {67: 1, 241: 0}


def noise_phenotype(n):
    """Standard normal noise whose REML null optimum over fixture(n, ..)'s K is the lower end of the range (test_lmm_wald_model.py
    asserts it on model R'; under REML, unlike under ML, the fixtures' own hg = 0 phenotypes have an interior optimum)."""
    return np.random.default_rng([21, n, NOISE_SEED[n]]).standard_normal(n)
