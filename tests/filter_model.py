"""An exact model of what the matrix-pipe filters must keep (test infrastructure: numpy, float64 and integers; no product code).

The filters (score_mx.hip, score_mxs.hip, score_coarse.hip, score_narrow.hip) quantise every phenotype column on an integer
lattice: y_i - c = w * t_i + resid_i with c = sum / N (sum: the reference's sequential float32 sum of the column), w the
column's unit and t_i an integer of the form's lattice. Their accumulators are exact (acc = kappa * sum_i g_i t_i, integers far
below 2^24), so for a row with bits g, N1 = sum g, d = N1 (N - N1),

    r_model = N * (g . e) + N1 * (N c - sum),      e_i = y_i - c - resid_i = w t_i,

is what the device holds (up to its unit), and which (row, column) pairs a filter keeps against a threshold thr is a computable
set. With the column's own error terms, as the comment above column_bound (scan_plan.cpp) defines them,

    Eg   = gamma_{L/4+3} * sum |y_i|       float32 summation error of the reference's chains (L = padded length)
    Rall = max(sum of the positive resid_i, sum of the |negative resid_i|),   rmax = max |resid_i|
    rho  = N * |N c - sum|                 (bounds |N1 (N c - sum)|: the rounding of c)
    E(N1) = Eg + min(Rall, N1 rmax)

three sets of MAC-passing rows are defined per column and threshold:

    R (required): the oracle's float32-chain score is > thr
    I (inner):    |r_model| + rho + N E >= sqrt(thr d)                  float64, no padding
    O (outer):    the same with every safe-direction rounding of the product granted (below)

and a correct filter satisfies  R <= I  (the bound itself),  I <= survivors  (the kernel keeps what its own test keeps) and
survivors <= O  (and nothing else). Pairs of O \\ I may go either way: that is float32 evaluation, not an error.

Derivation of the outer set, wide filters (block-scaled and int8; score_coarse.hip lines "per-row terms" / "the test", the same
code in score_mx.hip and score_mxs.hip). The device keeps a pair iff

    fma(-al, sq, |acc|) + Ed >= 0,   al = float32(sqrt(thr) * kalpha),  sq = hw_sqrt(float32 d) * 0.99999905f,
                                     Ed = (eg_max + fminf(rall_max, N1 * rmax_max)) * 1.000001f.

  Right-hand side. kalpha = (1 - 2^-19) / (N u) in double; float32(.) rounds by at most 2^-24 relative; the hardware square
  root is within 1 ulp (2^-23); 0.99999905f is exactly 1 - 2^-20; the product al * sq inside the fma is exact and the fma rounds
  once, by at most 2^-24 of a result whose magnitude is Ed at the boundary (granted on the error term below); the int8 kernels
  convert the integer Dc to float32 first (2^-24 relative of |acc|, which equals al * sq at the boundary up to Ed). The final
  addition cannot change the sign of an exact sum. So the device's right-hand side is at least
      sqrt(thr d) / (N u) * (1 - 2^-19)(1 - 2^-20)(1 - 2^-23)(1 - 2^-24)^2,
  i.e. 1 - 3.16e-6 at the least; the double-precision roundings of sqrt(thr) * kalpha are 2^-52 each. DELTA = 2^-19 + 2^-20 +
  2^-21 = 3.34e-6 covers the sum with 1.8e-7 to spare.
  Error term. column_bound pads Eg by (1 + 1e-6) and adds 1e-12 (1 + A); eg = (Eg' + rho' / N)(1 + 1e-6) + 1e-30 with
  rho' = 2 N |N c - sum| + 1e-9 (1 + |sum|); rall and rmax are padded by (1 + 1e-6); each is rounded to float32 and one ulp up
  (`up`: (1 + 2^-24)(1 + 2^-23)), divided by u with another (1 + 1e-6) and `up`; the device multiplies, takes the minimum, adds
  and multiplies by 1.000001f (exactly 1 + 2^-20 = 1 + 9.54e-7) with three float32 roundings, plus the fma's. In all at most
      (1 + 1e-6)^3 (1 + 2^-20) (1 + 2^-23 + 2^-24)^2 (1 + 2^-24)^4 = 1 + 4.55e-6   ->   F_E = 1 + 5e-6.
  The absolute pads (1e-12 (1 + A), 1e-9 (1 + |sum|), the factor 2 in rho') are not relative, so the outer set carries them as
  they are written. The kernel takes ONE error term for all columns: the maximum over the session's columns of each term in
  accumulator units (fold_bound); for column p that is w_p * max_j(term_j / w_j) in phenotype units (u_j = w_j / kappa, the same
  kappa for every column of a form). |acc| stands for N (g . e) without the N1 (N c - sum) part: the outer (and inner) left side
  adds rho for it.

      O:  |r_model| + rho + N * F_E * w_p * (egA + min(rallA, N1 rmaxA)) >= sqrt(thr d) * (1 - DELTA)

Narrow filter (score_narrow.hip, narrow_test; narrow_bound in scan_plan.cpp). Per column, in double:

    lhs = (|N yc + N1 t1| + N (eg + min(rall, N1 rmax))) (1 + 2^-30) + pad,     kept iff lhs^2 >= thr d (1 - 2^-30)

  behind a float32 pre-screen that is a superset by design (its slackf holds N1 |t1|, N E, the pad and the float32 roundings; it
  only saves the double evaluation, so the model has no term for it: if it ever cut into the inner set, I <= survivors fails).
  t1 = N c - sum exactly as the model has it; eg = (Eg (1 + 1e-6) + 1e-12 (1 + A)) (1 + 1e-9); rall = (Rall + N fuzz)(1 + 1e-9),
  rmax = (rmax + fuzz)(1 + 1e-9), fuzz = 64 * 2^-52 (mx + |c|); pad = 256 * 2^-52 N^2 (mx + |c| + 1) + 1e-300. sqrt(1 - 2^-30)
  >= 1 - 2^-30; the device's double roundings of yc, rc and the products (a few ulps of N^2 max|y|) are what pad is for: the
  outer set grants the pad twice and doubles both 2^-30 factors, and pads the error terms by 1e-8 instead of 1e-9:

      O:  (|r_model| + rho + N En)(1 + 2^-29) + 2 pad >= sqrt(thr d)(1 - 2^-29)

None of these constants is tuned to a kernel's output; a kernel that fails an inclusion is wrong, or the model misses a
documented step of it - then that step goes into the model with a reference to the kernel's lines.
"""
import os

import numpy as np

U32 = 2.0 ** -24
DELTA = 2.0 ** -19 + 2.0 ** -20 + 2.0 ** -21
F_E = 1.0 + 5e-6
N_DELTA = 2.0 ** -29


def _signed(vals):
    v = np.array(sorted(set(vals)), dtype=np.int64)
    return np.unique(np.concatenate([-v, v]))


A6 = _signed(list(range(16)) + list(range(16, 31, 2)) + list(range(32, 61, 4)))  # E2M3 x 8
A4 = _signed([0, 1, 2, 3, 4, 6, 8, 12])                                           # E2M1 x 2


def _two(sh, second):
    return np.unique((sh * A6[:, None] + second[None, :]).reshape(-1))


# form -> (t_unit: w = max|y - c| / t_unit, lattice of t (sorted int64), index of the form for kgwas_scan_debug_residuals).
# t_unit is the lattice's largest point except where the product's unit leaves headroom: two int8 slices take u = mx / (127 * 254)
# (quantise_int8: the first slice alone spans the column, the second holds the remainder: t = 254 q0 + q1 reaches 127 * 254 + 127),
# the narrow filter's three slices u0 = mx / 15, u0 / 30, u0 / 900 (t = 900 q0 + 30 q1 + q2 in units of u0 / 900, |q| <= 15).
FORMS = {
    "fp6": (60.0, A6, 0),
    "fp6_fp4": (492.0, _two(8, A4), 1),
    "fp6_fp6": (1980.0, _two(32, A6), 1),
    "int8_1": (127.0, np.arange(-127, 128, dtype=np.int64), 0),
    "int8_2": (127.0 * 254.0, np.arange(-32385, 32386, dtype=np.int64), 1),
    "narrow": (13500.0, np.arange(-13965, 13966, dtype=np.int64), 2),
}


def padded_len(S):
    return 128 * ((S + 127) // 128)


def chain_gamma(L):
    n = L / 4.0 + 3.0
    return n * U32 / (1.0 - n * U32)


def chain_sums(Y):
    """The reference's column sums: the sequential float32 sum of R[128 b + 4 s + l] = V[128 b + 32 l + 31 - s], V the column
    zero-padded to L samples (an own restatement; test_filter_model.py compares it with oracle_np.permuted_sum)."""
    Y = np.asarray(Y, dtype=np.float32)
    P, S = Y.shape
    L = padded_len(S)
    V = np.zeros((P, L), np.float32)
    V[:, :S] = Y
    k = np.arange(L)
    b, sx, l = k // 128, (k % 128) // 4, k % 4
    R = V[:, 128 * b + 32 * l + 31 - sx]
    return np.cumsum(R, axis=1, dtype=np.float32)[:, -1].astype(np.float64)  # (cumsum adds in order, one float32 rounding each)


def nearest_on(lattice, x):
    """The lattice point nearest to x (ties to the lower one): the model's own quantiser - it need not be the product's choice."""
    hi = np.clip(np.searchsorted(lattice, x), 1, len(lattice) - 1)
    lo = hi - 1
    return np.where(x - lattice[lo] <= lattice[hi] - x, lattice[lo], lattice[hi])


class FilterModel:
    """One filter form over the columns Y [P, S] of a session. resid [P, S]: the session's quantisation residuals
    (kgwas_scan_debug_residuals) or None - then the model quantises itself, to the nearest lattice point."""

    def __init__(self, form, Y, resid=None, sums=None):
        self.form = form
        t_unit, lattice, _ = FORMS[form]
        Y64 = np.asarray(Y, dtype=np.float32).astype(np.float64)
        self.P, self.S = Y64.shape
        N = float(self.S)
        self.N = N
        self.sum = chain_sums(Y) if sums is None else np.asarray(sums, dtype=np.float64)
        self.c = self.sum / N
        yc = Y64 - self.c[:, None]
        self.mx = np.abs(yc).max(axis=1)
        self.w = np.where(self.mx > 0, self.mx / t_unit, 1.0)
        if resid is None:
            t = nearest_on(lattice, yc / self.w[:, None])
            self.e = self.w[:, None] * t
            self.resid = yc - self.e
        else:
            self.resid = np.asarray(resid, dtype=np.float64)
            self.e = yc - self.resid
        # the slices encode lattice points: e / w is an integer of the form's lattice
        t = self.e / self.w[:, None]
        ti = np.rint(t)
        assert np.abs(t - ti).max() <= 1e-6, "form %s: e / w is not an integer (off by %g)" % (form, np.abs(t - ti).max())
        assert np.isin(ti.astype(np.int64), lattice).all(), "form %s: e / w leaves the form's lattice" % form
        self.A = np.abs(Y64).sum(axis=1)
        self.Eg = chain_gamma(padded_len(self.S)) * self.A
        self.rpos = np.where(self.resid > 0, self.resid, 0.0).sum(axis=1)
        self.rneg = np.where(self.resid < 0, -self.resid, 0.0).sum(axis=1)
        self.Rall = np.maximum(self.rpos, self.rneg)
        self.rmax = np.abs(self.resid).max(axis=1)
        self.t1 = N * self.c - self.sum
        self.rho = N * np.abs(self.t1)
        if form == "narrow":
            fuzz = 64.0 * 2.0 ** -52 * (self.mx + np.abs(self.c))
            self.n_eg = (self.Eg * (1 + 1e-6) + 1e-12 * (1 + self.A)) * (1 + 1e-8)
            self.n_rall = (self.Rall + N * fuzz) * (1 + 1e-8)
            self.n_rmax = (self.rmax + fuzz) * (1 + 1e-8)
            self.n_pad = 256.0 * 2.0 ** -52 * N * N * (self.mx + np.abs(self.c) + 1.0) + 1e-300
        else:
            rho_dev = 2.0 * N * np.abs(self.t1) + 1e-9 * (1.0 + np.abs(self.sum))
            eg_dev = self.Eg + 1e-12 * (1.0 + self.A) + rho_dev / N + 1e-30
            self.egA = (eg_dev / self.w).max()
            self.rallA = (self.Rall / self.w).max()
            self.rmaxA = (self.rmax / self.w).max()

    def r_model(self, g, n1):
        """[rows, P] float64"""
        return self.N * (g.astype(np.float64) @ self.e.T) + n1[:, None].astype(np.float64) * self.t1[None, :]

    def sets(self, g, n1, keep, scores, thr, block=4096):
        """g [n, S] 0/1, n1 [n], keep [n] (MAC rule), scores [P, n] (the oracle's), thr [n, P] (NaN: the pair is in no set).
        Returns R, I, O as [n, P] bool."""
        n = len(n1)
        R = np.zeros((n, self.P), bool)
        I = np.zeros((n, self.P), bool)
        O = np.zeros((n, self.P), bool)
        for a in range(0, n, block):
            sl = slice(a, min(a + block, n))
            N1 = n1[sl].astype(np.float64)[:, None]
            k = keep[sl][:, None]
            T = thr[sl]
            with np.errstate(invalid="ignore"):
                X = np.sqrt(T * (N1 * (self.N - N1)))
                ar = np.abs(self.r_model(g[sl], n1[sl]))
                E = self.Eg[None, :] + np.minimum(self.Rall[None, :], N1 * self.rmax[None, :])
                I[sl] = k & (ar + self.rho[None, :] + self.N * E >= X)
                if self.form == "narrow":
                    En = self.n_eg[None, :] + np.minimum(self.n_rall[None, :], N1 * self.n_rmax[None, :])
                    O[sl] = k & ((ar + self.rho[None, :] + self.N * En) * (1 + N_DELTA) + 2.0 * self.n_pad[None, :] >= X * (1 - N_DELTA))
                else:
                    Eo = F_E * self.w[None, :] * (self.egA + np.minimum(self.rallA, N1 * self.rmaxA))
                    O[sl] = k & (ar + self.rho[None, :] + self.N * Eo >= X * (1 - DELTA))
                R[sl] = k & (scores[:, sl].T > T)
        return R, I, O


# ---- inputs -------------------------------------------------------------------------------------------------------------

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def ft10(S):
    """The first S values of tests/golden/FT10.pheno (flowering time: all large and positive)."""
    vals = []
    with open(os.path.join(GOLD, "FT10.pheno")) as f:
        next(f)
        for line in f:
            p = line.split()
            if len(p) == 2:
                vals.append(np.float32(p[1]))
    assert len(vals) >= S
    return np.array(vals[:S], dtype=np.float32)


def case_phenotypes(case):
    """Y [P, S] float32. cols = "perm": permutations of one phenotype (what production runs: all columns share their error
    terms). "scaled": unrelated orders AND scales - every column another permutation of the phenotype times another factor from
    1e-3 to 1e3 -, plus a constant column: in phenotype units the columns' error terms differ by six orders of magnitude, in
    accumulator units they agree, which is what the kernel's one error term for all columns relies on."""
    S, P = case["S"], case["P"]
    rng = np.random.default_rng(1000 + 7 * S + P)
    if case["pheno"].startswith("ft10"):  # "ft10", "ft10+512": the same trait measured from an earlier day
        y0 = (ft10(S) + np.float32(case["pheno"][4:] or 0)).astype(np.float32)
    elif case["pheno"].startswith("shift"):  # "shift40": N(40, 1)
        y0 = (rng.standard_normal(S) + float(case["pheno"][5:])).astype(np.float32)
    else:
        y0 = rng.standard_normal(S).astype(np.float32)
    Y = np.stack([y0] + [rng.permutation(y0) for _ in range(P - 1)]).astype(np.float32)
    if case["cols"] == "scaled":
        f = np.array([1e-3, 1.0, 37.0, 1e3, 0.25, 3e-2], dtype=np.float32)
        Y = (Y * f[np.arange(P) % len(f)][:, None]).astype(np.float32)
        Y[P // 2] = np.float32(1.25)  # the constant column
    return np.ascontiguousarray(Y)


def case_table(case):
    """rows [n, 1 + W] uint64 (file layout), col [S]: the table of a case - random presence/absence rows with per-row
    frequencies, a fifth of them duplicates of earlier rows; S_f > S: the phenotyped accessions are a shuffled subset."""
    n, S_f, S = case["n"], case["S_f"], case["S"]
    rng = np.random.default_rng(77 + 13 * S_f + case["P"])
    W = (S_f + 63) // 64
    f = rng.uniform(0.03, 0.97, size=n)
    bits = rng.random((n, S_f)) < f[:, None]
    n_dup = n // 5
    dst = rng.choice(np.arange(1, n), size=n_dup, replace=False)
    src = (rng.random(n_dup) * dst).astype(np.int64)
    bits[dst] = bits[src]
    pad = np.zeros((n, W * 64), dtype=bool)
    pad[:, :S_f] = bits
    rows = np.empty((n, 1 + W), dtype=np.uint64)
    rows[:, 0] = np.sort(rng.choice(1 << 40, size=n, replace=False)).astype(np.uint64)
    rows[:, 1:] = np.packbits(pad.reshape(n, W, 64), axis=2, bitorder="little").view(np.uint64).reshape(n, W)
    col = rng.permutation(S_f)[:S].astype(np.uint64) if S_f > S else np.arange(S, dtype=np.uint64)
    return rows, col


def case_feeds(case):
    """[(first_row, end)]: three feeds whose lengths are no multiples of 64, so chunks end inside a wave's rows"""
    n = case["n"]
    a, b = n * 2 // 5 + 7, n * 3 // 4 + 29
    return [(0, a), (a, b), (b, n)]


def min_count(S):
    return max(int(np.ceil(S * 0.05)), 5)


def unpack(rows, col):
    col = col.astype(np.int64)
    g = ((rows[:, 1 + col // 64] >> (col % 64).astype(np.uint64)) & np.uint64(1)).astype(np.uint8)
    n1 = g.sum(axis=1).astype(np.int64)
    S, mc = len(col), min_count(len(col))
    keep = (n1 >= mc) & (n1 <= S - mc) if S - mc >= 0 else np.zeros(len(n1), bool)
    return g, n1, keep


def simulated_chunks(case, scores, keep):
    """What a session does with a case's rows, as far as the oracle alone tells: dense chunks until every column has topn
    MAC-passing rows, then chunks of chunk_rows inside each feed, each filtered against the column's topn-th best score of
    the rows before it. [(first_row, n_rows, thr [P])] of the filtered chunks."""
    topn, cr = case["topn"], case["chunk_rows"]
    dense = min(cr, max(1024, (topn + topn // 8 + 512 + 127) // 128 * 128))
    out = []
    full = False
    for a, b in case_feeds(case):
        pos = a
        while pos < b:
            if not full:
                pos = min(pos + dense, b)
                full = int(keep[:pos].sum()) >= topn
                continue
            c = min(cr, b - pos)
            sc = np.where(keep[None, :pos], scores[:, :pos], -1.0)
            thr = np.partition(sc, pos - topn, axis=1)[:, pos - topn]
            out.append((pos, c, thr))
            pos += c
    return out


def thresholds_by_row(n, P, chunks):
    """[n, P]: the thresholds of the chunk a row lies in (NaN: in no filtered chunk)"""
    T = np.full((n, P), np.nan)
    for first, c, thr in chunks:
        T[first:first + c] = np.asarray(thr, dtype=np.float64)[None, :]
    return T


def check_conditions(case, n, chunks, R, I, O):
    """The conditions that keep a case from hiding a failure: the rounding band is thin and the inclusions have something to
    say. Returns the figures."""
    nR, nI, band = int(R.sum()), int(I.sum()), int((O & ~I).sum())
    covered = sum(c for _, c, _ in chunks)
    fig = dict(case=case["name"], chunks=len(chunks), covered=covered / n, R=nR, I=nI, I_not_R=int((I & ~R).sum()), band=band, O=int(O.sum()))
    print("  %-36s chunks %2d covered %.2f |R| %6d |I| %6d |I \\ R| %6d |O \\ I| %4d" % (case["name"], fig["chunks"], fig["covered"], nR, nI, fig["I_not_R"], band))
    assert band <= 0.01 * nI, ("rounding band too wide", fig)
    assert len(chunks) >= 8 and covered >= 0.8 * n, ("too few filtered rows", fig)
    assert nR >= 500 and fig["I_not_R"] >= 100, ("too few pairs at the thresholds", fig)
    return fig


# ---- the cases: tests/test_filter_model.py qualifies every one on the CPU, tests/test_gpu_filter_survivors.py runs them -------

def _case(name, env, forms, S, P, S_f=None, cols="perm", pheno="normal", n=24_011, topn=200, chunk_rows=2048, expect=None):
    return dict(name=name, env=env, forms=forms, S=S, P=P, S_f=S_f or S, cols=cols, pheno=pheno, n=n, topn=topn,
                chunk_rows=chunk_rows, expect=expect or {})


_MX = {"KGWAS_COARSE_MX": "1", "KGWAS_MXS": "0"}
_MX66 = dict(_MX, KGWAS_MX_S1="6")
_MX1 = dict(_MX, KGWAS_COARSE_SLICES="1")
_I8 = {"KGWAS_COARSE_MX": "0"}

# forms: logged operand set (0 one slice, 1 two slices, 2 narrow) -> the model's form
# expect: statistics that say the intended kernel form ran (kgwas_scan_stats)
CASES = [
    # block-scaled, operands resident, FP6 + FP4
    _case("mx_241x5", _MX, {1: "fp6_fp4"}, 241, 5, expect=dict(coarse_mx=1, coarse_mx_stream=0, coarse_mx_steps=2)),
    _case("mx_1024x101_one_group", _MX, {1: "fp6_fp4"}, 1024, 101, expect=dict(coarse_mx=1, coarse_mx_stream=0, lgroups1=1, tiles1=7)),
    _case("mx_1135x101_two_groups_quarters", _MX, {1: "fp6_fp4"}, 1135, 101, pheno="ft10", expect=dict(coarse_mx=1, coarse_mx_stream=0, lgroups1=2, tiles1=4, coarse_mx_steps=9)),
    _case("mx_2048x201_five_groups", _MX, {1: "fp6_fp4"}, 2048, 201, n=20_011, expect=dict(coarse_mx=1, coarse_mx_stream=0, lgroups1=5, tiles1=3)),
    # three full groups of 4 tiles (63 columns each) + a rest launch of one tile: 26 tile-slices instead of 4 x 4 x 2
    _case("mx_1536x192_full_groups_and_rest", _MX, {1: "fp6_fp4"}, 1536, 192, n=20_011, expect=dict(coarse_mx=1, coarse_mx_stream=0, lgroups1=4, tiles1=4, tile_slices1=26)),
    _case("mx_513x6", _MX, {1: "fp6_fp4"}, 513, 6, expect=dict(coarse_mx=1, coarse_mx_steps=5)),
    _case("mx_639x7_subset", _MX, {1: "fp6_fp4"}, 639, 7, S_f=700, expect=dict(coarse_mx=1, coarse_mx_steps=5)),
    _case("mx_640x9_scaled", _MX, {1: "fp6_fp4"}, 640, 9, cols="scaled", expect=dict(coarse_mx=1, coarse_mx_steps=5)),
    _case("mx_641x6", _MX, {1: "fp6_fp4"}, 641, 6, expect=dict(coarse_mx=1, coarse_mx_steps=6)),
    _case("mx_1023x8", _MX, {1: "fp6_fp4"}, 1023, 8, expect=dict(coarse_mx=1, coarse_mx_steps=8)),
    # FP6 + FP6 and one FP6 slice
    _case("mx66_1024x40", _MX66, {1: "fp6_fp6"}, 1024, 40, expect=dict(coarse_mx=1, coarse_mx_s1_fp6=1)),
    _case("mx66_1135x101_subset", _MX66, {1: "fp6_fp6"}, 1135, 101, S_f=1200, pheno="ft10", expect=dict(coarse_mx=1, coarse_mx_s1_fp6=1)),
    _case("mx6_1024x40_scaled", _MX1, {0: "fp6"}, 1024, 40, cols="scaled", expect=dict(coarse_mx=1, launches0=True)),
    _case("mx6_1135x101", _MX1, {0: "fp6"}, 1135, 101, pheno="ft10", expect=dict(coarse_mx=1, launches0=True)),
    # block-scaled, operands streamed
    _case("mxs3_1135x101_one_column_group", {"KGWAS_COARSE_MX": "1", "KGWAS_MXS": "3"}, {1: "fp6_fp4"}, 1135, 101, pheno="ft10", expect=dict(coarse_mx=1, coarse_mx_stream=1, tiles1=7)),
    _case("mxs3_2048x201_two_column_groups", {"KGWAS_COARSE_MX": "1", "KGWAS_MXS": "3"}, {1: "fp6_fp4"}, 2048, 201, n=20_011, expect=dict(coarse_mx=1, coarse_mx_stream=1, tiles1=7, lgroups1=1)),
    _case("mxs3_2048x201_form1", {"KGWAS_COARSE_MX": "1", "KGWAS_MXS": "3", "KGWAS_MXS_FORM": "1"}, {1: "fp6_fp4"}, 2048, 201, n=20_011, cols="scaled", expect=dict(coarse_mx=1, coarse_mx_stream=2, tiles1=13)),
    _case("mxs3_2048x201_form2", {"KGWAS_COARSE_MX": "1", "KGWAS_MXS": "3", "KGWAS_MXS_FORM": "2"}, {1: "fp6_fp4"}, 2048, 201, n=20_011, expect=dict(coarse_mx=1, coarse_mx_stream=3, tiles1=13)),
    _case("mxs1_5200x20_default", {"KGWAS_COARSE_MX": "1", "KGWAS_MXS": "1"}, {1: "fp6_fp4"}, 5200, 20, n=20_011, expect=dict(coarse_mx=1, coarse_mx_stream=1)),
    _case("mxs1_4096x100_default", {"KGWAS_COARSE_MX": "1", "KGWAS_MXS": "1"}, {1: "fp6_fp4"}, 4096, 100, n=20_011, expect=dict(coarse_mx=1, coarse_mx_stream=1, tiles1=7)),
    # int8, one and two slices
    _case("int8_1_241x5", dict(_I8, KGWAS_COARSE_SLICES="1"), {0: "int8_1"}, 241, 5, expect=dict(coarse_mx=0, launches0=True)),
    _case("int8_2_241x5_shifted", dict(_I8, KGWAS_COARSE_SLICES="2"), {1: "int8_2"}, 241, 5, pheno="shift2000", expect=dict(coarse_mx=0)),
    _case("int8_1_1024x130_scaled", dict(_I8, KGWAS_COARSE_SLICES="1"), {0: "int8_1"}, 1024, 130, cols="scaled", expect=dict(coarse_mx=0, launches0=True)),
    _case("int8_2_1024x130", dict(_I8, KGWAS_COARSE_SLICES="2"), {1: "int8_2"}, 1024, 130, expect=dict(coarse_mx=0)),
    _case("int8_2_2048x201_subset", dict(_I8, KGWAS_COARSE_SLICES="2"), {1: "int8_2"}, 2048, 201, S_f=2100, n=20_011, expect=dict(coarse_mx=0)),
    _case("int8_1_4096x100", dict(_I8, KGWAS_COARSE_SLICES="1"), {0: "int8_1"}, 4096, 100, n=20_011, expect=dict(coarse_mx=0, launches0=True)),
    # nothing forced at 4096 x 100 without the streaming form: the int8 one-slice set in the steady state, the block-scaled
    # two-slice set on the ramp - both must appear among the logged chunks
    # (the session leaves the two-slice set once candidates per row x (4.0 - survivors per candidate of the two-slice set) falls
    # below mode_k x the sets' difference in tile-slices, pick_coarse_mode: with 100 columns that is row 30 000 to 35 000 at top-12
    # and beyond row 250 000 at top-100 - so this case alone has a small heap and 50 011 rows, as the heap test of the same plan has)
    _case("mixed_4096x100", {"KGWAS_MXS": "0"}, {0: "int8_1", 1: "fp6_fp4"}, 4096, 100, n=50_011, topn=12, chunk_rows=2048, expect=dict(coarse_mx=0, coarse_mx_steps=32, both_sets=True)),
]
# narrow filter: one to four columns (one column: pack1, the column's operands in all four column slots). Its three slices leave
# residuals of 4e-5 of the largest value, so with one to four columns only a column far from zero - the chains' float32 summation
# error Eg = gamma * sum |y| - puts a hundred pairs between the required and the inner set: N(2000, 1) at 241 samples (gamma_67),
# N(40, 1) at 1024, and at 1135 the FT10 values counted from 512 days earlier (as they are: 20-70 such pairs with 1-3 columns).
for _S, _ph in ((241, "shift2000"), (1024, "shift40"), (1135, "ft10+512")):
    for _P in (1, 2, 3, 4):
        CASES.append(_case("narrow_%dx%d" % (_S, _P), {}, {2: "narrow"}, _S, _P, S_f=(_S + 59 if _P == 3 else None), pheno=_ph,
                           cols=("scaled" if (_P == 4 and _S == 1024) else "perm"), n=30_011, topn=300, chunk_rows=2048,
                           expect=dict(narrow=True)))
