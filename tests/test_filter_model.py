"""The filters' exact model (tests/filter_model.py) on the CPU: pinned on columns small enough to work by hand, then the bound
itself - every pair the oracle scores above a threshold lies in the model's inner set, for every form's lattice - and the
qualification of the inputs that tests/test_gpu_filter_survivors.py runs on the device."""
import numpy as np
import pytest

import filter_model as fm
from oracle import binding as ob
from oracle import oracle_np as onp


def test_chain_sums_equal_the_oracles_permuted_sum():
    rng = np.random.default_rng(3)
    for S in (5, 128, 241, 1135):
        Y = (rng.standard_normal((3, S)) * 7 + 2).astype(np.float32)
        got = fm.chain_sums(Y)
        for j in range(3):
            assert got[j] == float(onp.permuted_sum(Y[j]))
        assert fm.padded_len(S) == onp.padded_len(S)


def test_unpack_is_the_oracles_mac_filter():
    case = dict(n=500, S_f=300, S=257, P=3)
    rows, col = fm.case_table(case)
    g, n1, keep = fm.unpack(rows, col)
    g2, n12, keep2 = onp.mac_filter(rows, col, onp.min_count(257, 0.05, 5))
    assert (g == g2).all() and (n1 == n12).all() and (keep == keep2).all() and fm.min_count(257) == onp.min_count(257, 0.05, 5)


def test_lattices_are_the_documented_ones():
    assert len(fm.A6) == 63 and fm.A6.max() == 60 and set(np.abs(fm.A6)) == set(range(16)) | set(range(16, 31, 2)) | set(range(32, 61, 4))
    assert sorted(set(np.abs(fm.A4))) == [0, 1, 2, 3, 4, 6, 8, 12]
    for form, tmax in (("fp6", 60), ("fp6_fp4", 492), ("fp6_fp6", 1980), ("int8_1", 127), ("int8_2", 32385)):
        assert fm.FORMS[form][1].max() == tmax and fm.FORMS[form][0] == (127 * 254 if form == "int8_2" else tmax)
    assert 7 in fm.FORMS["fp6_fp4"][1] and 491 not in fm.FORMS["fp6_fp4"][1]  # 8 * 1 - 1; 8 * 60 + 11 does not exist
    assert fm.FORMS["narrow"][1].max() == 900 * 15 + 30 * 15 + 15


def test_one_int8_slice_by_hand():
    """S = 4, y = (1, 2, 3, 6): sum 12, c = 3, y - c = (-2, -1, 0, 3), w = 3 / 127. t = (-84.67, -42.33, 0, 127) -> (-85, -42, 0, 127),
    resid = (+1/127, -1/127, 0, 0): Rall = rmax = 1 / 127. The row (1, 0, 0, 1) has N1 = 2, d = 4, reference score
    (4 * 7 - 2 * 12)^2 / 4 = 4, and it holds exactly the positive residual: N (g . e) = 4 - 4 / 127, and N E = 4 / 127 + 4 Eg
    gives the 4 back - the bound is attained, the pair sits in the inner set up to thr = 4 (1 + Eg)^2 and not beyond."""
    y = np.array([[1, 2, 3, 6]], dtype=np.float32)
    m = fm.FilterModel("int8_1", y)
    assert m.sum[0] == 12 and m.c[0] == 3 and m.mx[0] == 3 and m.rho[0] == 0
    assert np.allclose(m.e[0] / m.w[0], [-85, -42, 0, 127], atol=1e-9)
    assert np.allclose(m.resid[0], [1 / 127, -1 / 127, 0, 0], atol=1e-12)
    assert abs(m.Rall[0] - 1 / 127) < 1e-12 and abs(m.rmax[0] - 1 / 127) < 1e-12
    gam = (128 / 4 + 3) * 2.0 ** -24 / (1 - (128 / 4 + 3) * 2.0 ** -24)
    assert abs(m.Eg[0] - gam * 12) < 1e-18
    g = np.array([[1, 0, 0, 1], [0, 1, 1, 0]], dtype=np.uint8)
    n1 = np.array([2, 2])
    assert np.allclose(m.r_model(g, n1)[:, 0], [4 - 4 / 127, -(4 - 4 / 127)], atol=1e-12)
    keep = np.array([True, True])
    scores = np.array([[4.0, 4.0]])
    for thr, inR, inI in ((3.99, True, True), (4.0, False, True), (4.0 * (1 + gam * 12) ** 2 * (1 - 1e-12), False, True), (4.001, False, False)):
        R, I, O = m.sets(g, n1, keep, scores, np.full((2, 1), thr))
        assert R[0, 0] == inR and I[0, 0] == inI and (O[0, 0] or not I[0, 0])
    # the complementary row holds the negative residual: same score, same tightness
    R, I, O = m.sets(g, n1, keep, scores, np.full((2, 1), 4.0))
    assert I[1, 0] and not R[1, 0]
    # a row outside the MAC rule is in no set
    R, I, O = m.sets(g, n1, np.array([False, True]), scores, np.full((2, 1), 0.0))
    assert not (R[0, 0] or I[0, 0] or O[0, 0]) and R[1, 0] and I[1, 0] and O[1, 0]


def test_fp6_fp4_by_hand():
    """S = 8, y = (-61.5, 61.5, 10, -10, 0.875, -0.875, 0.6875, -0.6875): sum 0 exactly, w = 61.5 / 492 = 1 / 8, y / w =
    (-492, 492, 80, -80, 7, -7, 5.5, -5.5). 492 = 8 * 60 + 12, 80 = 8 * 10, 7 = 8 * 1 - 1 are lattice points; 5.5 lies between 5 =
    8 * 1 - 3 and 6 (the tie goes down: 5 and -6), resid = +1/16 twice: Rall = 1/8, rmax = 1/16, no negative residual."""
    y = np.array([[-61.5, 61.5, 10, -10, 0.875, -0.875, 0.6875, -0.6875]], dtype=np.float32)
    m = fm.FilterModel("fp6_fp4", y)
    assert m.sum[0] == 0 and m.c[0] == 0 and m.w[0] == 0.125
    assert (m.e[0] / m.w[0] == [-492, 492, 80, -80, 7, -7, 5, -6]).all()
    assert m.Rall[0] == 0.125 and m.rmax[0] == 0.0625 and m.rneg[0] == 0 and m.rho[0] == 0
    # the row of the two rounded samples and the largest value: N1 = 3, d = 15; N (g . e) = 8 * (61.5 + 0.625 - 0.75) = 491
    g = np.array([[0, 1, 0, 0, 0, 0, 1, 1]], dtype=np.uint8)
    assert m.r_model(g, np.array([3]))[0, 0] == 491.0
    # the reference: 8 * 61.5 = 492, score 492^2 / 15; the inner set's left side: 491 + 8 * (Eg + min(1/8, 3/16)) = 492 + 8 Eg
    s = 492.0 ** 2 / 15
    for thr, inR, inI in ((s * (1 - 1e-9), True, True), (s, False, True), (s * (1 + 1e-3), False, False)):
        R, I, O = m.sets(g, np.array([3]), np.array([True]), np.array([[s]]), np.array([[thr]]))
        assert R[0, 0] == inR and I[0, 0] == inI and (O[0, 0] or not I[0, 0])
    # the session's own residuals instead of the model's quantiser: the other neighbour (6 and -5) is a lattice point too
    resid = np.zeros((1, 8))
    resid[0, 6:] = -0.0625
    m2 = fm.FilterModel("fp6_fp4", y, resid=resid)
    assert (m2.e[0] / m2.w[0] == [-492, 492, 80, -80, 7, -7, 6, -5]).all() and m2.rpos[0] == 0 and m2.Rall[0] == 0.125
    # ... and a value the slices cannot encode is caught (8 * 60 + 11)
    bad = np.zeros((1, 8))
    bad[0, 1] = 0.125
    with pytest.raises(AssertionError):
        fm.FilterModel("fp6_fp4", y, resid=bad)


def test_constant_column_and_the_common_error_term_by_hand():
    """A constant column: c = y, max|y - c| = 0, w = 1, nothing to encode, r_model = 0 for every row. Beside it a column
    (0, 4, 0, 4, ...) * 1000: the kernel's one error term is the maximum in units of w, so the outer set of the small column
    does not inherit the large column's phenotype-unit terms."""
    S = 8
    Y = np.array([[1.25] * S, [0, 4000, 0, 4000, 0, 4000, 0, 4000], [0, 4e-3, 0, 4e-3, 0, 4e-3, 0, 4e-3]], dtype=np.float32)
    m = fm.FilterModel("int8_1", Y)
    assert m.mx[0] == 0 and m.w[0] == 1 and (m.e[0] == 0).all() and m.Rall[0] == 0
    assert m.w[1] == 2000 / 127 and abs(m.w[2] / m.w[1] - 1e-6) < 1e-12
    g = np.array([[1, 1, 1, 0, 0, 0, 0, 0]], dtype=np.uint8)
    assert (m.r_model(g, np.array([3]))[0, 0]) == 0
    # accumulator units: the two scaled columns have the same terms up to float32's rounding of 4e-3
    assert abs(m.Eg[1] / m.w[1] - m.Eg[2] / m.w[2]) < 1e-6 * m.Eg[1] / m.w[1]
    # (the absolute pads of column_bound, 1e-12 and 1e-9 / N, weigh 0.4 % in the units of the column scaled by 1e-3)
    assert m.egA >= (m.Eg / m.w).max() and m.egA < (m.Eg / m.w).max() * 1.01


# ---- the trial: R <= I for every form's lattice ---------------------------------------------------------------------------

def _trial_columns(S, kind, rng):
    if kind == "perm":
        y0 = rng.standard_normal(S).astype(np.float32)
        return np.stack([y0] + [rng.permutation(y0) for _ in range(19)])
    if kind == "shifted":
        y0 = (rng.standard_normal(S) * 3 + 100).astype(np.float32)
        return np.stack([y0] + [rng.permutation(y0) for _ in range(5)])
    # unrelated columns, different scales, and a constant one
    y0 = rng.standard_normal(S).astype(np.float32)
    Y = np.stack([rng.permutation(y0) * np.float32(f) for f in (1e-3, 1.0, 37.0, 1e3, 0.25, 3e-2)] + [np.full(S, 1.25)])
    return Y


@pytest.mark.parametrize("kind", ["perm", "scaled", "shifted"])
@pytest.mark.parametrize("S", [241, 1024, 1135])
def test_required_pairs_lie_in_the_inner_set(S, kind, capsys):
    """20 000 random rows against each column's 300th best score: the oracle's candidates (R) are inside the bound (I) without a
    single exception, for every form's lattice, and the outer set adds at most 1 % to the inner one."""
    rng = np.random.default_rng(S * 3 + len(kind))
    Y = np.ascontiguousarray(_trial_columns(S, kind, rng).astype(np.float32))
    P = len(Y)
    case = dict(n=20_000, S_f=S, S=S, P=P)
    rows, col = fm.case_table(case)
    g, n1, keep = fm.unpack(rows, col)
    scores, kept = ob.scores_dense(rows, S, col, Y, fm.min_count(S))
    assert (kept == keep).all()
    sc = np.where(keep[None, :], scores, -1.0)
    thr = np.partition(sc, len(n1) - 300, axis=1)[:, len(n1) - 300]
    T = np.broadcast_to(thr[None, :], (len(n1), P)).copy()
    for form in fm.FORMS:
        m = fm.FilterModel(form, Y)
        R, I, O = m.sets(g, n1, keep, scores, T)
        nR, nI, band = int(R.sum()), int(I.sum()), int((O & ~I).sum())
        with capsys.disabled():
            print("\n  trial %s S=%d %-8s |R| %6d |I| %6d |O \\ I| %4d  (%.2f kept per required pair)" % (kind, S, form, nR, nI, band, nI / max(nR, 1)), end="")
        assert not (R & ~I).any(), "%d required pairs outside the bound" % int((R & ~I).sum())
        assert not (I & ~O).any()
        assert band <= 0.01 * nI
        assert nR >= 0.9 * 299 * (P - (1 if kind == "scaled" else 0))  # (duplicated rows tie with a threshold here and there)


# ---- qualification of the GPU test's inputs -------------------------------------------------------------------------------

@pytest.mark.parametrize("case", fm.CASES, ids=[c["name"] for c in fm.CASES])
def test_gpu_case_is_sharp_enough(case, capsys):
    """Every case of tests/test_gpu_filter_survivors.py, from the oracle alone (own quantiser, thresholds = the running topn-th
    best score at each chunk's start): R <= I, the rounding band O \\ I is at most 1 % of I, at least eight filtered chunks
    cover at least 80 % of the rows, and |R| >= 500, |I \\ R| >= 100 - otherwise the inclusions on the device would say nothing."""
    rows, col = fm.case_table(case)
    Y = fm.case_phenotypes(case)
    g, n1, keep = fm.unpack(rows, col)
    scores, kept = ob.scores_dense(rows, case["S_f"], col, Y, fm.min_count(case["S"]))
    assert (kept == keep).all()
    chunks = fm.simulated_chunks(case, scores, keep)
    assert any(c % 64 for _, c, _ in chunks)
    T = fm.thresholds_by_row(case["n"], case["P"], chunks)
    for form in case["forms"].values():
        m = fm.FilterModel(form, Y)
        R, I, O = m.sets(g, n1, keep, scores, T)
        assert not (R & ~I).any() and not (I & ~O).any()
        with capsys.disabled():
            print()
            fm.check_conditions(case, case["n"], chunks, R, I, O)
