"""Float64 numpy models of lmm_lrt with covariates (-c), y = W a + x b + u + e with W of q columns, and the seeded fixtures of
its tests. lmm_lrt_np.py and lmm_wald_np.py are imported and not changed.

The ML LRT is lmm_lrt_np's fit_R and fit_E with the designs X = [W] and [W, x]: both already take a design of any width.

For -lmm 4 the two models of lmm_wald_np.py are restated for a design [W, x] (theirs has the intercept written in):
  model R' (rotated): the sqrt(h)-weighted lstsq and slogdet of the weighted Gram matrix,
      lR(lambda) = df/2 (log(df / 2 pi) - 1) + 1/2 sum log h_i - 1/2 log |A^T A| - df/2 log RSS,  df = n - columns of the design;
  model G (never rotates): V = lambda K + I = L L^T, the design and y whitened by L^-1, beta by the normal equations, the t-test
      of the LAST coefficient, and the score statistic n (x^T P0 y)^2 / ((x^T P0 x) (y^T P0 y)) with the null projection
      P0 = V0^-1 - V0^-1 W (W^T V0^-1 W)^-1 W^T V0^-1.
The REML value depends on the basis of W (by log |det A| under W -> W A); everything else does not.
"""
import functools

import numpy as np
from scipy.linalg import cho_solve, solve_triangular

import lmm_lrt_np as M
import lmm_wald_np as WN

TWO_PI = WN.TWO_PI


def design(W, x=None):
    W = np.asarray(W, np.float64)
    return W if x is None else np.column_stack([W, x])


# ---- the ML LRT ----

def lrt_R(K, y, W, xs):
    """(LRT of every row of xs, l0) by model R"""
    l0, _ = M.fit_R(K, y, design(W))
    return np.array([max(0.0, 2 * (M.fit_R(K, y, design(W, x))[0] - l0)) for x in xs]), l0


def lrt_E(K, y, W, xs):
    l0, _ = M.fit_E(K, y, design(W))
    return np.array([max(0.0, 2 * (M.fit_E(K, y, design(W, x))[0] - l0)) for x in xs]), l0


def loglik_R_at(K, y, W, x, lam):
    d, U = M.eig_of(K)
    return float(M.loglik_R(d, U.T @ y, U.T @ design(W, x), np.array([lam]))[0])


# ---- model R' ----

def _rotated(K, y, W, x):
    d, U = M.eig_of(K)
    return d, U.T @ y, U.T @ design(W, x)


def reml_R_at(K, y, W, x, lam):
    d, yt, Ct = _rotated(K, y, W, x)
    return float(WN.reml_R(d, yt, Ct, np.array([lam]))[0])


def fit_reml_R(K, y, W, x, lmin=M.LMIN, lmax=M.LMAX):
    """(lR, lambda) at model R''s REML optimum of the design [W, x] (x None: [W])"""
    d, yt, Ct = _rotated(K, y, W, x)

    def f(t):
        return (WN._reml_R_fast if len(t) > 1 else WN.reml_R)(d, yt, Ct, np.exp(t))

    v, t = M.maximise(f, np.log(lmin), np.log(lmax))
    lam = float(np.exp(t))
    return float(WN.reml_R(d, yt, Ct, np.array([lam]))[0]), lam


def wald_R(K, y, W, x, lam):
    """(beta, se, F_wald) of the last coefficient of model R' at lambda"""
    d, yt, Ct = _rotated(K, y, W, x)
    s = np.sqrt(1.0 / (lam * d + 1.0))
    A = Ct * s[:, None]
    coef, *_ = np.linalg.lstsq(A, yt * s, rcond=None)
    r = (yt - Ct @ coef) * s
    df = y.size - Ct.shape[1]
    se = np.sqrt(r @ r / df * np.linalg.inv(A.T @ A)[-1, -1])
    return float(coef[-1]), float(se), float((coef[-1] / se) ** 2)


def score_R(K, y, W, x, lam0):
    """F_score of model R' at lambda0: x and y regressed on W under the weights, by lstsq"""
    d, yt, Ct = _rotated(K, y, W, x)
    s = np.sqrt(1.0 / (lam0 * d + 1.0))
    w = Ct[:, :-1] * s[:, None]
    B = np.column_stack([Ct[:, -1] * s, yt * s])
    coef, *_ = np.linalg.lstsq(w, B, rcond=None)
    R = B - w @ coef
    return float(y.size * (R[:, 0] @ R[:, 1]) ** 2 / ((R[:, 0] @ R[:, 0]) * (R[:, 1] @ R[:, 1])))


# ---- model G ----

def gls_G(K, y, W, x, lam):
    """(beta, se, F_wald, lR) of model G at lambda for the last column of [W, x]; x None: (None, None, None, lR0)"""
    X = design(W, x)
    n, c = X.shape
    df = n - c
    L, (Xs, ys) = WN._whiten(K, lam, X, y)
    XtX = Xs.T @ Xs
    coef = np.linalg.solve(XtX, Xs.T @ ys)
    r = ys - Xs @ coef
    rss = float(r @ r)
    logdet_V = 2.0 * np.sum(np.log(np.diag(L)))
    reml = -0.5 * (df * np.log(TWO_PI * rss / df) + df + logdet_V + np.linalg.slogdet(XtX)[1])
    if x is None:
        return None, None, None, float(reml)
    se = np.sqrt(rss / df * np.linalg.inv(XtX)[-1, -1])
    return float(coef[-1]), float(se), float((coef[-1] / se) ** 2), float(reml)


def vg_ve_G(K, y, W, lam):
    """(vg, ve) of model G's null model at lambda: ve = r^T V^-1 r / (n - q), vg = lambda ve"""
    X = design(W)
    L, (Xs, ys) = WN._whiten(K, lam, X, y)
    r = ys - Xs @ np.linalg.solve(Xs.T @ Xs, Xs.T @ ys)
    ve = float(r @ r) / (y.size - X.shape[1])
    return lam * ve, ve


def vg_ve_R(K, y, W, lam):
    """The same from model R': the weighted lstsq's RSS / (n - q)"""
    d, yt, Ct = _rotated(K, y, W, None)
    s = np.sqrt(1.0 / (lam * d + 1.0))
    coef, *_ = np.linalg.lstsq(Ct * s[:, None], yt * s, rcond=None)
    r = (yt - Ct @ coef) * s
    ve = float(r @ r) / (y.size - Ct.shape[1])
    return lam * ve, ve


def score_G(K, y, W, x, lam0):
    n = y.size
    W = design(W)
    L = np.linalg.cholesky(lam0 * K + np.eye(n))
    VW = cho_solve((L, True), W)

    def P0(v):
        a = cho_solve((L, True), v)
        return a - VW @ np.linalg.solve(W.T @ VW, W.T @ a)

    x = np.asarray(x, np.float64)
    Py, Px = P0(y), P0(x)
    return float(n * (x @ Py) ** 2 / ((x @ Px) * (y @ Py)))


def fit_reml_G(K, y, W, x, lmin=M.LMIN, lmax=M.LMAX):
    def f(t):
        return np.array([gls_G(K, y, W, x, float(np.exp(s)))[3] for s in t])

    v, t = M.maximise(f, np.log(lmin), np.log(lmax))
    return float(v), float(np.exp(t))


def orthonormal(W):
    """The basis the tool replaces W by, and log |det R| of W = Q R (numpy's QR with the signs of modified Gram-Schmidt)"""
    Q, R = np.linalg.qr(np.asarray(W, np.float64))
    s = np.sign(np.diag(R))
    return Q * s, float(np.sum(np.log(np.abs(np.diag(R)))))


# ---- fixtures ----

FORMS = ("ones", "normal", "batch", "eigen", "q8", "recombined")
RECOMBINE = np.array([[3.0e3, 2.0e-2], [-1.0e3, 5.0e-3]])  # W A of the form "normal": not orthogonal, badly scaled


@functools.lru_cache(maxsize=None)
def covariates(n, rows, form, seed=1):
    """W (n x q) over fixture(n, rows, .)'s K:
      ones        [1]
      normal      [1, z], z standard normal
      batch       [1, b], b a 0 / 1 covariate
      eigen       [1, the two leading eigenvectors of K]: the practical case; Wt is near unit vectors
      q8          [1, seven normals]
      recombined  the form "normal" times RECOMBINE"""
    rng = np.random.default_rng([seed, n, 31])
    one = np.ones(n)
    z = rng.standard_normal((n, 7))
    b = (rng.random(n) < 0.4).astype(np.float64)
    if form == "ones":
        W = one[:, None]
    elif form == "normal":
        W = np.column_stack([one, z[:, 0]])
    elif form == "batch":
        W = np.column_stack([one, b])
    elif form == "eigen":
        _, K, _ = M.fixture(n, rows, 3.0)
        d, U = M.eig_of(K)
        W = np.column_stack([one, U[:, -1], U[:, -2]])
    elif form == "q8":
        W = np.column_stack([one, z])
    elif form == "recombined":
        W = covariates(n, rows, "normal", seed) @ RECOMBINE
    else:
        raise ValueError(form)
    W = np.ascontiguousarray(W)
    W.setflags(write=False)
    return W


@functools.lru_cache(maxsize=None)
def width(n, rows, q, seed=1):
    """[1, q - 1 normals]: the widths of the grid sums' row groups"""
    W = np.ascontiguousarray(covariates(n, rows, "q8", seed)[:, :q])
    W.setflags(write=False)
    return W


def phenotype(y, W, seed=1):
    """y plus an effect of every covariate but the first (so that leaving W out would show)"""
    rng = np.random.default_rng([seed, W.shape[0], W.shape[1], 41])
    Q, _ = orthonormal(W)
    out = y + (Q[:, 1:] * np.sqrt(W.shape[0])) @ rng.uniform(0.5, 1.5, W.shape[1] - 1) if W.shape[1] > 1 else y.copy()
    return out


# ---- the fixtures of test_gpu_lmm_lrt_covar_widths.py (test_lmm_covar_model.py qualifies each without a GPU) ----

@functools.lru_cache(maxsize=None)
def eigen_q(n, rows, q):
    """[1, the q - 1 leading eigenvectors of fixture(n, rows, .)'s K]: population structure as covariates. Wt is near unit vectors,
    and the diagonal of A = Wt^T H Wt runs from 1 down to 1 / (lambda d_max + 1). q = 3 is the form "eigen"."""
    _, K, _ = M.fixture(n, rows, 3.0)
    d, U = M.eig_of(K)
    W = np.ascontiguousarray(np.column_stack([np.ones(n)] + [U[:, -1 - j] for j in range(q - 1)]))
    W.setflags(write=False)
    return W


def _recombine_q8():
    """A fixed, badly scaled 8 x 8 matrix: standard normals (seeded) with columns scaled from 1e-2 to 1e2. Its condition number is
    asserted by test_lmm_covar_model.py to lie in [1e4, 1e6], far from the tool's rank refusal at 1e-8."""
    A = np.random.default_rng([8, 31, 7]).standard_normal((8, 8)) * 10.0 ** np.linspace(-2.0, 2.0, 8)[None, :]
    A.setflags(write=False)
    return A


RECOMBINE_Q8 = _recombine_q8()


@functools.lru_cache(maxsize=None)
def recombined_q8(n, rows):
    """width(n, rows, 8) times RECOMBINE_Q8: the same column space in a basis that is neither orthogonal nor scaled"""
    W = np.ascontiguousarray(width(n, rows, 8) @ RECOMBINE_Q8)
    W.setflags(write=False)
    return W


# (n, seed, q): two_peak_fixture(n, seed) with q - 1 normal covariates beside the intercept. (16, 148) at q = 3 and (16, 69) are
# left out: models R and E differ by 2.2e-10 and 3.5e-9 there.
TWO_PEAK_W_CASES = ((67, 54, 2), (67, 54, 3), (67, 56, 2), (67, 56, 3), (8, 18, 2), (8, 18, 3), (16, 148, 2))


@functools.lru_cache(maxsize=None)
def two_peak_case(n, seed, q):
    """(K, y, W, V): lmm_lrt_np.two_peak_fixture's K and y (y as it is: phenotype() would flatten the structure), W = [1, q - 1
    standard normals], V = the fixture's first 16 presence rows (the dosages are 2 V)."""
    K, y, X = M.two_peak_fixture(n, seed, M.two_peak_rows(n))
    V = X[:16]
    assert len(V) == 16
    W = np.column_stack([np.ones(n), np.random.default_rng([n, seed, q]).standard_normal((n, q - 1))])
    W.setflags(write=False)
    return K, y, W, V


def interior_maxima(K, y, C, reml=False):
    """The interior local maxima of model R's l (reml: model R''s lR) of the design C on the 2001-point grid: [(log lambda, l)]"""
    d, U = M.eig_of(K)
    t = np.linspace(np.log(M.LMIN), np.log(M.LMAX), M.GRID + 1)
    v = (WN._reml_R_fast if reml else M._loglik_R_fast)(d, U.T @ y, U.T @ C, np.exp(t))
    return [(float(t[i]), float(v[i])) for i in range(1, M.GRID) if v[i] > v[i - 1] and v[i] >= v[i + 1]]


SPAN_ROWS = 40                 # with chunk_variants 32: a chunk boundary
SPAN_DEGENERATE = (5, 11, 35)  # b, 1 - b, and b again behind the chunk boundary


@functools.lru_cache(maxsize=None)
def span_panel(n, rows):
    """(K, y0, V, b): 40 presence rows over fixture(n, rows, 3.0), 37 ordinary ones and, at SPAN_DEGENERATE, the batch covariate b
    of covariates(n, rows, "batch"), 1 - b and b again: with W = [1, b] their x lies in span(W)."""
    G, K, y0 = M.fixture(n, rows, 3.0)
    b = covariates(n, rows, "batch")[:, 1].astype(np.uint8)
    assert 0 < b.sum() < n
    ordinary = [r for r in M.varying(G) if not (np.array_equal(r, b) or np.array_equal(r, 1 - b))][:SPAN_ROWS - len(SPAN_DEGENERATE)]
    V = np.zeros((SPAN_ROWS, n), np.uint8)
    keep = np.setdiff1d(np.arange(SPAN_ROWS), SPAN_DEGENERATE)
    V[keep] = ordinary
    V[SPAN_DEGENERATE[0]], V[SPAN_DEGENERATE[1]], V[SPAN_DEGENERATE[2]] = b, 1 - b, b
    V.setflags(write=False)
    return K, y0, V, b
