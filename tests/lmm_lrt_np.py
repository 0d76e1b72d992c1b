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


@functools.lru_cache(maxsize=None)
def strong_fixture(n, rows, seed=1, nv=20):
    """A panel with a causal variant, for phenotypes y(effect) = 0.3 e + 0.5 (U sqrt(d)) z + effect G[r] on fixture(n, rows, 3.0)'s
    G and K: (K, base, g, V) with y(effect) = base + effect * g. V (nv x n, 0 / 1): the causal row g = G[r], two copies of it with
    2 %, 10 % and 30 % of their entries flipped (at least one entry), then unrelated varying rows of G. Nothing depends on the
    effect but y, so that the phenotypes of several effects are columns over one panel."""
    G, K, _ = fixture(n, rows, 3.0)
    rng = np.random.default_rng([seed, n, rows, 11])
    d, U = np.linalg.eigh(K)
    d = np.clip(d, 0, None)
    e, z = rng.standard_normal(n), rng.standard_normal(n)
    base = 0.3 * e + 0.5 * ((U * np.sqrt(d)) @ z)
    W = varying(G)
    r = int(rng.integers(len(W)))
    g = W[r]
    V = [g]
    for frac in (0.02, 0.02, 0.1, 0.1, 0.3, 0.3):
        c = g.copy()
        c[rng.permutation(n)[:max(1, round(frac * n))]] ^= 1
        V.append(c)
    V = np.array(V + [W[k] for k in range(len(W)) if k != r][:nv - len(V)], np.uint8)
    assert len(V) == nv and len(varying(V)) == nv
    g = g.astype(np.float64)
    for a in (base, g, V):
        a.setflags(write=False)
    return K, base, g, V


@functools.lru_cache(maxsize=None)
def two_peak_fixture(n, seed, rows=16):
    """A wide-spectrum kinship, under which l(log lambda) can have two interior maxima: (K, y, X). K = sym(Q diag(d) Q^T), Q from the
    QR of an n x n standard normal, d = exp(U(-8, 8)) with each entry set to 0 with probability 0.2, y = Q (z exp(U(-3, 3))), z
    standard normal; X = the varying ones of `rows` Bernoulli(0.4) rows (drawn last and row by row: more rows keep the first)."""
    rng = np.random.default_rng([seed, n, 7])
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    d = np.exp(rng.uniform(-8, 8, n))
    d[rng.random(n) < 0.2] = 0.0
    K = (Q * d) @ Q.T
    K = 0.5 * (K + K.T)
    z = rng.standard_normal(n)
    y = Q @ (z * np.exp(rng.uniform(-3, 3, n)))
    X = varying((rng.random((rows, n)) < 0.4).astype(np.uint8))
    for a in (K, y, X):
        a.setflags(write=False)
    return K, y, X


STRONG_EFFECTS = (3.0, 10.0, 40.0)
STRONG_ROWS = {67: 400, 241: 600, 1135: 1400}
# (n, seed) of two_peak_fixture with two interior maxima under H0, H1 or both (test_lmm_lrt_model.py recomputes and asserts which)
TWO_PEAK_CASES = ((8, 18), (8, 36), (16, 69), (16, 148), (5, 12), (67, 54), (67, 56))


def two_peak_rows(n):
    """16 rows, and 48 more at the small sizes, so that a 16-variant and a 32-variant tile are crossed"""
    return 64 if n <= 16 else 16


def interior_maxima(K, y, x=None, lmin=LMIN, lmax=LMAX):
    """The interior local maxima of model R's l on its 2001-point grid, H1 (x given) or H0: [(log lambda, l)], in grid order."""
    d, U = eig_of(K)
    one = np.ones(y.size)
    X = one[:, None] if x is None else np.column_stack([one, x])
    t = np.linspace(np.log(lmin), np.log(lmax), GRID + 1)
    v = _loglik_R_fast(d, U.T @ y, U.T @ X, np.exp(t))
    return [(float(t[i]), float(v[i])) for i in range(1, GRID) if v[i] > v[i - 1] and v[i] >= v[i + 1]]


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


def call_stats(D):
    """(af, n_miss, constant) of dosage rows the way the tool counts them: af = (sum of the called dosages / their number) / 2."""
    D = np.asarray(D)
    called = D >= 0
    cnt = called.sum(axis=1)
    af = 0.5 * (np.where(called, D, 0).sum(axis=1) / np.maximum(cnt, 1))
    constant = np.array([len(set(r[c])) < 2 for r, c in zip(D, called)])
    return af, (~called).sum(axis=1), constant


def expect_tested(D, maf, miss):
    af, n_miss, constant = call_stats(D)
    return ~constant & (np.minimum(af, 1 - af) >= maf) & (n_miss / D.shape[1] <= miss)


@functools.lru_cache(maxsize=None)
def codes_panel(n, rows, nv):
    """(K, y, D): nv dosage rows over fixture(n, rows, 3.0) with heterozygous (20 %) and missing (5 %) calls, of which row nv - 2
    has its only missing call, and row nv - 1 its only minor allele, at the last individual (the last 2-bit field of a row)."""
    G, K, y = fixture(n, rows, 3.0)
    rng = np.random.default_rng([5, n, nv])
    D = 2 * varying(G)[:nv].astype(np.int64)
    assert len(D) == nv
    D[:nv - 2][rng.random((nv - 2, n)) < 0.2] = 1
    D[:nv - 2][rng.random((nv - 2, n)) < 0.05] = -1
    D[nv - 2, n - 1] = -1
    D[nv - 1] = 0
    D[nv - 1, n - 1] = 2
    D.setflags(write=False)
    return K, y, D


DROPPED = (0, 3, 4, 33, 68, 69)  # the individuals without a phenotype in dropped_panel's columns 1, 3 and 4; column 2 also lacks 17


@functools.lru_cache(maxsize=None)
def dropped_panel():
    """70 individuals of whom some have no phenotype: (K, D, pheno). K 70 x 70, D 40 x 70 dosages with heterozygous and missing
    calls, pheno 70 x 4 (NaN = missing): columns 1, 3, 4 lack DROPPED (64 kept, a multiple of 4), column 2 lacks individual 17 as
    well (63 kept). Rows 0..5 of D change what the filters say once the dropped are gone:
      0  missing at the dropped and at 10: 7 / 70 of all, 1 / 64 of the kept
      1  its carriers are the dropped and individual 20: af 0.1 of all, 1 / 64 of the kept
      2  its carriers are the dropped alone: constant among the kept
      3  missing at 30 kept individuals
      4  missing at the dropped, heterozygous and homozygous calls elsewhere
      5  heterozygous everywhere but at individual 17: constant once 17 is gone"""
    n, nv = 70, 40
    G, K, y = fixture(n, 400, 3.0)
    rng = np.random.default_rng([9, n, nv])
    D = 2 * varying(G)[:nv].astype(np.int64)
    D[rng.random((nv, n)) < 0.2] = 1
    D[rng.random((nv, n)) < 0.03] = -1
    drop = list(DROPPED)
    D[0, drop + [10]] = -1
    D[0, [11, 12]] = 1
    D[1] = 0
    D[1, drop + [20]] = 2
    D[2] = 0
    D[2, drop] = 2
    D[3, rng.permutation(np.setdiff1d(np.arange(n), drop))[:30]] = -1
    D[4, drop] = -1
    D[5] = 1
    D[5, 17] = 2
    pheno = np.stack([y, y + 2.5 * (D[7] > 0), rng.permutation(y), rng.permutation(y)], axis=1)
    pheno[drop] = np.nan
    pheno[17, 1] = np.nan
    for a in (D, pheno):
        a.setflags(write=False)
    return K, D, pheno


@functools.lru_cache(maxsize=None)
def filter_edge_panel(n):
    """(K, y, D) over fixture(n, 400, 3.0): 6 ordinary rows, then row 6 with one homozygous carrier (af = 1 / n), row 7 with one
    missing call, row 8 with two, row 9 with every individual but the last one missing."""
    G, K, y = fixture(n, 400, 3.0)
    D = np.zeros((10, n), np.int64)
    D[:6] = 2 * varying(G)[:6]
    D[6, n // 2] = 2
    D[7:9] = 2 * varying(G)[6:8]
    D[7:9, 0], D[7:9, 2] = 2, 0  # (they vary whatever is missing)
    D[7, 1] = -1
    D[8, [1, n - 2]] = -1
    D[9] = -1
    D[9, n - 1] = 2
    D.setflags(write=False)
    return K, y, D
