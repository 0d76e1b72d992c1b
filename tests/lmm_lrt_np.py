"""Two float64 numpy models of the statistic lmm_lrt computes, and the seeded fixtures of its tests.

The statistic: the ML likelihood-ratio test of y = W a + x b + u + e, u ~ N(0, lambda K / tau), e ~ N(0, I / tau), W = 1.

Model R (rotated) follows the tool's formulation: K = U diag(d) U^T, everything rotated by U^T, h_i = 1 / (lambda d_i + 1),
    l(lambda) = n/2 log(n / 2 pi) - n/2 + 1/2 sum log h_i - n/2 log RSS(lambda),
RSS the residual sum of squares of the h-weighted regression (here by lstsq, not by a Schur complement).

Model E (per marker) restates the route of the reference tree's src/R/emma.R (emma.ML.LRT, emma.MLE, emma.eigen.R.wo.Z,
emma.delta.ML.LL.wo.Z): S = I - X (X^T X)^-1 X^T, the n - q leading eigenpairs of S (K + I) S, etas = vectors^T y and
    LL(delta) = 1/2 (n (log(n / 2 pi) - 1 - log sum etas^2 / (values + delta)) - sum log(xi + delta)),  delta = 1 / lambda,
xi the eigenvalues of K. It never rotates by K's eigenvectors and costs O(n^3) per marker: use it at n <= 241 only.

Both are maximised the same way: a uniform grid of 2000 intervals over log lambda in [log lmin, log lmax], then
scipy.optimize.minimize_scalar(bounded) over the two intervals around the best grid point; the larger of the two wins.
"""
import functools

import numpy as np
from scipy.optimize import minimize_scalar

GRID = 2000
LMIN, LMAX = float(np.exp(-10.0)), float(np.exp(10.0))  # the range both models and the tool search in the tests


def maximise(f, lo, hi):
    """max of f over t in [lo, hi]: (value, t). f takes an array of t."""
    t = np.linspace(lo, hi, GRID + 1)
    v = f(t)
    i = int(np.argmax(v))
    a, b = t[max(i - 1, 0)], t[min(i + 1, GRID)]
    r = minimize_scalar(lambda s: -float(f(np.array([s]))[0]), bounds=(a, b), method="bounded", options={"xatol": 1e-11})
    if -r.fun > v[i]:
        return -r.fun, float(r.x)
    return float(v[i]), float(t[i])


# ---- model R ----

@functools.lru_cache(maxsize=None)
def _eig_cached(key):
    K = _eig_cached.store[key]
    d, U = np.linalg.eigh(K)
    d[np.abs(d) < 1e-8] = 0.0
    return d, U


_eig_cached.store = {}


def eig_of(K):
    key = (K.shape[0], hash(K.tobytes()))
    _eig_cached.store[key] = K
    return _eig_cached(key)


def loglik_R(d, yt, Ct, lam):
    """l(lambda) for rotated y and rotated covariates Ct (n x q); lam an array."""
    n = yt.size
    out = np.empty(len(lam))
    for k, L in enumerate(lam):
        h = 1.0 / (L * d + 1.0)
        s = np.sqrt(h)
        beta, *_ = np.linalg.lstsq(Ct * s[:, None], yt * s, rcond=None)
        r = (yt - Ct @ beta) * s
        out[k] = 0.5 * n * (np.log(n / (2 * np.pi)) - 1.0) + 0.5 * np.sum(np.log(h)) - 0.5 * n * np.log(r @ r)
    return out


def _loglik_R_fast(d, yt, Ct, lam):
    """The same through the normal equations, vectorised over lam (the 2001-point grid); the bounded search uses loglik_R."""
    n = yt.size
    H = 1.0 / (lam[:, None] * d[None, :] + 1.0)  # (m, n)
    q = Ct.shape[1]
    G = np.einsum("mi,ia,ib->mab", H, Ct, Ct)
    b = np.einsum("mi,ia,i->ma", H, Ct, yt)
    yy = H @ (yt * yt)
    beta = np.linalg.solve(G, b[:, :, None])[:, :, 0] if q else np.zeros((len(lam), 0))
    rss = yy - np.einsum("ma,ma->m", beta, b)
    return 0.5 * n * (np.log(n / (2 * np.pi)) - 1.0) + 0.5 * np.sum(np.log(H), axis=1) - 0.5 * n * np.log(rss)


def fit_R(K, y, X, lmin=LMIN, lmax=LMAX):
    """(l, lambda) of the model with covariates X (n x q)."""
    d, U = eig_of(K)
    yt, Ct = U.T @ y, U.T @ X

    def f(t):
        if len(t) > 1:
            return _loglik_R_fast(d, yt, Ct, np.exp(t))
        return loglik_R(d, yt, Ct, np.exp(t))

    t = np.linspace(np.log(lmin), np.log(lmax), GRID + 1)
    v = f(t)
    i = int(np.argmax(v))
    a, b = t[max(i - 1, 0)], t[min(i + 1, GRID)]
    r = minimize_scalar(lambda s: -float(f(np.array([s]))[0]), bounds=(a, b), method="bounded", options={"xatol": 1e-11})
    vi = float(loglik_R(d, yt, Ct, np.exp(t[i:i + 1]))[0])
    return (-r.fun, float(np.exp(r.x))) if -r.fun > vi else (vi, float(np.exp(t[i])))


def lrt_R(K, y, xs, lmin=LMIN, lmax=LMAX):
    """LRT of every row of xs (variants x n, dosages); also l0."""
    one = np.ones((y.size, 1))
    l0, _ = fit_R(K, y, one, lmin, lmax)
    out = np.array([max(0.0, 2 * (fit_R(K, y, np.column_stack([one[:, 0], x]), lmin, lmax)[0] - l0)) for x in xs])
    return out, l0


def loglik_R_at(K, y, x, lam):
    """Model R's l at one lambda, H1 (x given) or H0 (x None)."""
    d, U = eig_of(K)
    one = np.ones(y.size)
    X = one[:, None] if x is None else np.column_stack([one, x])
    return float(loglik_R(d, U.T @ y, U.T @ X, np.array([lam]))[0])


# ---- model E ----

def fit_E(K, y, X, lmin=LMIN, lmax=LMAX):
    n, q = X.shape
    S = np.eye(n) - X @ np.linalg.solve(X.T @ X, X.T)
    w, V = np.linalg.eigh(S @ (K + np.eye(n)) @ S)
    values, vectors = w[q:] - 1.0, V[:, q:]  # the n - q largest
    etas = vectors.T @ y
    xi = np.linalg.eigvalsh(K)
    e2 = etas * etas

    def f(logdelta):
        delta = np.exp(np.atleast_1d(logdelta))[:, None]
        return 0.5 * (n * (np.log(n / (2 * np.pi)) - 1.0 - np.log(np.sum(e2[None, :] / (values[None, :] + delta), axis=1)))
                      - np.sum(np.log(xi[None, :] + delta), axis=1))

    v, t = maximise(f, -np.log(lmax), -np.log(lmin))
    return v, float(np.exp(-t))


def lrt_E(K, y, xs, lmin=LMIN, lmax=LMAX):
    one = np.ones(y.size)
    l0, _ = fit_E(K, y, one[:, None], lmin, lmax)
    return np.array([max(0.0, 2 * (fit_E(K, y, np.column_stack([one, x]), lmin, lmax)[0] - l0)) for x in xs]), l0


# ---- fixtures ----

@functools.lru_cache(maxsize=None)
def fixture(n, rows, hg, seed=1):
    """G (rows x n, 0 / 1), K = 1 - Hamming / rows, y = e + hg (U sqrt(d)) z + 1.2 G[7]."""
    rng = np.random.default_rng([seed, n, rows])
    f = rng.uniform(0.1, 0.9, rows)
    G = (rng.random((rows, n)) < f[:, None]).astype(np.uint8)
    Gf = G.astype(np.float64)
    ham = Gf.T @ (1 - Gf) + (1 - Gf).T @ Gf
    K = 1.0 - ham / rows
    d, U = np.linalg.eigh(K)
    d = np.clip(d, 0, None)
    e, z = rng.standard_normal(n), rng.standard_normal(n)
    y = e + hg * ((U * np.sqrt(d)) @ z) + 1.2 * Gf[7 % rows]
    for a in (G, K, y):
        a.setflags(write=False)
    return G, K, y


def varying(G):
    """Rows of G that are not constant."""
    s = G.sum(axis=1)
    return G[(s > 0) & (s < G.shape[1])]


CODE_OF_DOSAGE = {2: 0, 1: 2, 0: 3, -1: 1}  # .bed codes: 00 -> 2, 10 -> 1, 11 -> 0, 01 missing


def pack_bed(dosage):
    """dosage (variants x n; 2, 1, 0 or -1 for missing) -> .bed body, SNP-major, (n + 3) // 4 bytes per variant."""
    dosage = np.asarray(dosage)
    m, n = dosage.shape
    codes = np.zeros((m, (n + 3) // 4 * 4), np.uint8)
    lut = np.zeros(4, np.uint8)
    for k, v in CODE_OF_DOSAGE.items():
        lut[k + 1] = v
    codes[:, :n] = lut[dosage.astype(np.int64) + 1]
    c = codes.reshape(m, -1, 4)
    return (c[:, :, 0] | (c[:, :, 1] << 2) | (c[:, :, 2] << 4) | (c[:, :, 3] << 6)).astype(np.uint8)


def presence_bed(G):
    """k-mer presence rows as pass 2 writes them: present 00 (value 2), absent 11 (value 0)."""
    return pack_bed(2 * G.astype(np.int64))


def mean_imputed(dosage):
    x = np.asarray(dosage, np.float64).copy()
    for r in x:
        miss = r < 0
        r[miss] = r[~miss].mean() if (~miss).any() else 0.0
    return x
