"""lmm_lrt without a GPU: the host eigensolver, the two numpy models of the statistic against each other, and the file layer.

Measured here (float64, -lmin / -lmax = e^-10 / e^10, fixtures (n, rows) = (67, 400) and (241, 600), hg in {0, 3}): the largest
|LRT_R - LRT_E| over the fixtures' variants is 2.7e-12; the test asserts it stays under 1e-9. The fixtures of
test_gpu_lmm_lrt_regimes.py (strong associations up to LRT 4720, two-peaked likelihoods under a wide-spectrum K, dropped
individuals, the smaller edges) are measured by the tests after that one, each asserted <= 1e-10: 2.3e-13 .. 2.2e-11 for the strong
ones up to n = 241 (the largest at LRT 1760), 7.0e-11 at n = 1135 and LRT 4720, 9.1e-13 .. 5.3e-11 for the two-peaked ones, at
most 1.2e-11 for the rest. MEASURED_MODEL_GAP below is the largest of all of them. The GPU tests allow 1000 x that gap, capped at
1e-8: since the strong fixtures came, the cap is what holds.

Two fixtures were replaced for the models' own error, not for the tool's. The strong panel at n = 1135 takes its K from 1400 rows
and not 600: a K of rank 601 has 534 zero eigenvalues, which model R sets to 0 and model E keeps as +-1e-13, and under a strong
effect, where lambda differs between H0 and H1, that alone is a gap of 4e-10. Seed 14 of the two-peaked recipe at n = 16 has, among
its 48 further rows, two on which the models differ by 1e-9 and 2e-9; seed 148 (one peak under H0, two under H1 likewise) is used.
"""
import ctypes as C
import os

import numpy as np
import pytest

from kmersgwas_amd import capi
from kmersgwas_amd.capi import lib, ptr

import lmm_lrt_np as M

MEASURED_MODEL_GAP = 7.1e-11  # largest |LRT_R - LRT_E| seen on the fixtures below (printed by test_models_agree and by _gap)


def sym_eigen(K, threads):
    n = K.shape[0]
    K = np.ascontiguousarray(K, np.float64)
    d, U = np.zeros(n), np.zeros((n, n))
    capi.check(lib.kgwas_sym_eigen(n, ptr(K), ptr(d), ptr(U), threads))
    return d, U


def residuals(K, d, U):
    nk = np.linalg.norm(K)
    return np.linalg.norm(K - (U * d) @ U.T) / (nk if nk else 1.0), np.linalg.norm(U.T @ U - np.eye(K.shape[0]))


def eigen_cases():
    for n in (1, 2, 5, 67, 241, 1135):
        rng = np.random.default_rng(n)
        rows = max(8, n // 2)
        G = (rng.random((rows, n)) < rng.uniform(0.1, 0.9, rows)[:, None]).astype(np.float64)
        if n >= 5:  # duplicated individuals: repeated (zero) eigenvalues
            G[:, 1] = G[:, 0]
            G[:, n - 1] = G[:, 2]
        K = 1.0 - (G.T @ (1 - G) + (1 - G).T @ G) / rows
        yield "hamming-%d" % n, K
        yield "diagonal-%d" % n, np.diag(rng.uniform(0.5, 2.0, n))


@pytest.mark.parametrize("name,K", list(eigen_cases()), ids=[c[0] for c in eigen_cases()])
def test_sym_eigen(name, K):
    n = K.shape[0]
    d1, U1 = sym_eigen(K, 1)
    d16, U16 = sym_eigen(K, 16)
    assert d1.tobytes() == d16.tobytes() and U1.tobytes() == U16.tobytes(), "threads 1 and 16 differ"
    assert (np.diff(d1) >= 0).all(), "eigenvalues are not sorted"
    dn, Un = np.linalg.eigh(K)
    rec, orth = residuals(K, d1, U1)
    rec_np, orth_np = residuals(K, dn, Un)
    msg = "%s: ||K - U D U^T|| / ||K|| = %.3e (numpy %.3e), ||U^T U - I|| = %.3e (numpy %.3e)" % (name, rec, rec_np, orth, orth_np)
    print(msg)
    assert rec <= 8 * rec_np and orth <= 8 * orth_np, msg
    # both solvers are backward stable: each eigenvalue is within c n eps ||K|| of the true one; 1e-12 n max|d| is c = 4500
    assert np.abs(d1 - dn).max() <= 1e-12 * max(1.0, np.abs(dn).max()) * n, msg


def test_models_agree():
    worst = 0.0
    for n, rows in ((67, 400), (241, 600)):
        for hg in (0.0, 3.0):
            G, K, y = M.fixture(n, rows, hg)
            xs = M.varying(G)[:24].astype(np.float64)
            a, l0a = M.lrt_R(K, y, xs)
            b, l0b = M.lrt_E(K, y, xs)
            gap = float(np.abs(a - b).max())
            print("n=%d rows=%d hg=%g: max |LRT_R - LRT_E| = %.3e, |l0_R - l0_E| = %.3e, LRT range %.3g..%.3g"
                  % (n, rows, hg, gap, abs(l0a - l0b), a.min(), a.max()))
            worst = max(worst, gap)
    print("largest gap %.3e (MEASURED_MODEL_GAP = %.1e)" % (worst, MEASURED_MODEL_GAP))
    assert worst < 1e-9


def test_fixture_optimum_interior_and_at_lmin():
    for hg, interior in ((3.0, True), (0.0, False)):
        G, K, y = M.fixture(67, 400, hg)
        _, lam = M.fit_R(K, y, np.ones((67, 1)))
        assert (M.LMIN * 1.0001 < lam < M.LMAX / 1.0001) == interior, (hg, lam)


# ---- the fixtures of test_gpu_lmm_lrt_regimes.py: what each is for is asserted here, on the models; every gap <= NEW_GAP_MAX ----

NEW_GAP_MAX = 1e-10  # a hundredth of the GPU tolerance's cap of 1e-8: a fixture that misses it is replaced, not tolerated


def _gap(name, K, y, xs, lmin=M.LMIN, lmax=M.LMAX):
    a, l0a = M.lrt_R(K, y, xs, lmin, lmax)
    b, l0b = M.lrt_E(K, y, xs, lmin, lmax)
    gap = max(float(np.abs(a - b).max()), abs(l0a - l0b))
    print("%s: max |LRT_R - LRT_E| = %.3e, |l0_R - l0_E| = %.3e, LRT range %.3g..%.3g" % (name, np.abs(a - b).max(), abs(l0a - l0b), a.min(), a.max()))
    assert gap <= NEW_GAP_MAX, name
    return a


def test_strong_fixtures():
    for n in (67, 241):
        K, base, g, V = M.strong_fixture(n, M.STRONG_ROWS[n])
        for effect in M.STRONG_EFFECTS:
            lrt = _gap("strong n=%d effect=%g" % (n, effect), K, base + effect * g, V.astype(np.float64))
            assert lrt.max() > 100 and lrt.argmax() == 0 and lrt.min() < 10, lrt
    # n = 1135 is past what model E is meant for (O(n^3) per marker, and the rounding of an 1135 x 1135 eigenproblem in every
    # marker): the gap is taken on the causal row and one of each kind of the others
    n = 1135
    K, base, g, V = M.strong_fixture(n, M.STRONG_ROWS[n], nv=16)
    lrt = _gap("strong n=1135 effect=10 (4 of 16 variants)", K, base + 10.0 * g, V[[0, 1, 5, 9]].astype(np.float64))
    assert lrt.max() > 100 and lrt.argmax() == 0


def test_two_peak_fixtures():
    """Model R's interior maxima on its 2001-point grid, for H0 and every variant's H1 of every two-peaked fixture: the set has
    models whose first peak wins, models whose second wins, and fixtures where H0 and H1 differ in their number of peaks; the
    peaks of one model are >= 1.0 apart in log lambda (5 of the tool's 101-point grid's intervals of 0.2) and differ by > 1e-6 in l."""
    first = second = differ = 0
    for n, seed in M.TWO_PEAK_CASES:
        K, y, X = M.two_peak_fixture(n, seed, M.two_peak_rows(n))
        xs = X.astype(np.float64)
        _gap("two-peak n=%d seed=%d (%d variants)" % (n, seed, len(xs)), K, y, xs)
        models = [("H0", None)] + [("x%d" % k, x) for k, x in enumerate(xs)]
        counts = []
        for name, x in models:
            pk = M.interior_maxima(K, y, x)
            counts.append(len(pk))
            ends = [M.loglik_R_at(K, y, x, lam) for lam in (M.LMIN, M.LMAX)]
            if name in ("H0", "x0"):
                print("  n=%d seed=%d %s: peaks (log lambda, l) %s, l at the ends %.3f %.3f"
                      % (n, seed, name, " ".join("(%.2f, %.4f)" % p for p in pk), ends[0], ends[1]))
            if len(pk) < 2:
                continue
            ls = sorted((l for _, l in pk), reverse=True)
            assert ls[0] - ls[1] > 1e-6, (n, seed, name, pk)
            assert min(np.diff([t for t, _ in pk])) >= 1.0, (n, seed, name, pk)
            if ls[0] > max(ends):  # the global optimum is a peak: which one
                win = int(np.argmax([l for _, l in pk]))
                first += win == 0
                second += win == len(pk) - 1 and win > 0
        differ += any(c != counts[0] for c in counts[1:])
        print("  n=%d seed=%d: peaks under H0 %d, under H1 %s" % (n, seed, counts[0], dict(zip(*np.unique(counts[1:], return_counts=True)))))
    print("two-peaked models whose first peak is the global optimum: %d, whose last: %d; fixtures where H0 and H1 differ: %d" % (first, second, differ))
    assert first >= 2 and second >= 2 and differ >= 1


def test_edge_fixtures():
    """The model gap of the remaining panels of test_gpu_lmm_lrt_regimes.py, each with the calls and the search range it is run with."""
    K, y, D = M.codes_panel(241, 600, 24)
    assert not M.call_stats(D)[2].any()
    _gap("codes n=241", K, y, M.mean_imputed(D))
    K, y, D = M.codes_panel(1135, 600, 12)
    _gap("codes n=1135 (3 of 12 variants)", K, y, M.mean_imputed(D)[[0, 10, 11]])
    for hg in (0.0, 3.0):
        G, K, y = M.fixture(67, 400, hg)
        _gap("default range n=67 hg=%g" % hg, K, y, M.varying(G)[:24].astype(np.float64), 1e-5, 1e5)
    assert M.fit_R(M.fixture(67, 400, 0.0)[1], M.fixture(67, 400, 0.0)[2], np.ones((67, 1)), 1e-5, 1e5)[1] == pytest.approx(1e-5, rel=1e-12)
    for n, maf, miss in ((20, 0.05, 1.0), (21, 0.05, 1.0), (5, 0.0, 0.2)):
        K, y, D = M.filter_edge_panel(n)
        t = M.expect_tested(D, maf, miss)
        assert list(t[6:]) == {20: [True, True, True, False], 21: [False, True, True, False], 5: [True, True, False, False]}[n]
        assert t[:6].sum() >= 2
        _gap("filter edges n=%d" % n, K, y, M.mean_imputed(D[t]))
    K, D, pheno = M.dropped_panel()
    for col in range(4):
        keep = np.flatnonzero(~np.isnan(pheno[:, col]))
        assert len(keep) == (63 if col == 1 else 64)
        Ds = D[:, keep]
        t = M.expect_tested(Ds, 0.05, 0.05)
        full = M.expect_tested(D, 0.05, 0.05)
        # rows 0..3: the filters say something else about the kept than about all 70; row 5 falls with individual 17
        assert list(t[:4]) == [True, False, False, False] and list(full[:4]) == [False, True, True, False]
        assert t[5] == (col != 1) and t.sum() >= 20
        _gap("dropped individuals column %d (%d kept, %d tested)" % (col + 1, len(keep), t.sum()), K[np.ix_(keep, keep)], pheno[keep, col],
             M.mean_imputed(Ds[t]), 1e-5, 1e5)


def test_assoc_formatting_of_a_p_below_the_normal_doubles():
    """erfc underflows past LRT = 1420 or so: such a p is printed as a number that parses back (a subnormal or 0), never as nan"""
    for p in (0.0, 4.9406564584124654e-324, 1.5e-310, 2.2250738585072014e-308, 3.1e-300):
        field = _format(b"1", b"r", b"5", 0, b"A", b"C", 0.5, 1.0, p).rstrip("\n").split("\t")[8]
        back = float(field)
        assert "nan" not in field.lower() and "inf" not in field.lower() and back == float("%.6e" % p), (p, field)
        assert 0.0 <= back <= 2.3e-308 or p > 1e-307


# ---- host side of the tool ----

def _err(rc):
    return (lib.kgwas_last_error() or b"").decode()


def test_read_kinship(tmp_path):
    K = np.array([[1.0, 0.25, -1e-3], [0.25, 1.0, 0.5], [-1e-3, 0.5, 1.0]])
    p = tmp_path / "k.txt"
    p.write_text("\n".join("\t".join("%.17g" % v for v in r) for r in K) + "\n")
    out = np.zeros((3, 3))
    capi.check(lib.kgwas_lmm_read_kinship(str(p).encode(), 3, ptr(out)))
    assert (out == K).all()
    assert lib.kgwas_lmm_read_kinship(str(p).encode(), 4, ptr(np.zeros((4, 4)))) == capi.KGWAS_ERR_FORMAT  # rows
    assert "rows" in _err(0)
    p.write_text("1\t0\t0\n0\t1\n0\t0\t1\n")
    assert lib.kgwas_lmm_read_kinship(str(p).encode(), 3, ptr(out)) == capi.KGWAS_ERR_FORMAT  # a short row
    p.write_text("1\t0\t0\n0\tx\t0\n0\t0\t1\n")
    assert lib.kgwas_lmm_read_kinship(str(p).encode(), 3, ptr(out)) == capi.KGWAS_ERR_FORMAT  # text
    assert lib.kgwas_lmm_read_kinship(str(tmp_path / "none").encode(), 3, ptr(out)) == capi.KGWAS_ERR_IO


def test_read_fam_phenotype_column_and_missing(tmp_path):
    p = tmp_path / "a.fam"
    p.write_text("f1 i1 0 0 0 1.5 7\nf2 i2 0 0 0 -9 8\nf3 i3 0 0 0 NA -9\nf4 i4 0 0 0 -2.25e1 NA\n")
    for col, exp_v, exp_k in ((1, [1.5, np.nan, np.nan, -22.5], [1, 0, 0, 1]), (2, [7, 8, np.nan, np.nan], [1, 1, 0, 0])):
        v, k, n = np.zeros(8), np.zeros(8, np.uint8), C.c_uint64()
        capi.check(lib.kgwas_lmm_read_fam(str(p).encode(), col, 8, ptr(v), ptr(k), C.byref(n)))
        assert n.value == 4 and list(k[:4]) == exp_k
        np.testing.assert_array_equal(v[:4], np.array(exp_v, float))
    n = C.c_uint64()
    assert lib.kgwas_lmm_read_fam(str(p).encode(), 3, 0, None, None, C.byref(n)) == capi.KGWAS_ERR_FORMAT  # no such column
    assert lib.kgwas_lmm_read_fam(str(p).encode(), 0, 0, None, None, C.byref(n)) == capi.KGWAS_ERR_ARG
    p.write_text("f1 i1 0 0 0 abc\n")
    assert lib.kgwas_lmm_read_fam(str(p).encode(), 1, 0, None, None, C.byref(n)) == capi.KGWAS_ERR_FORMAT


def _format(*a):
    buf = C.create_string_buffer(512)
    need = lib.kgwas_lmm_format_assoc(*a, buf, 512)
    return buf.raw[:need].decode()


def test_assoc_formatting():
    assert _format(None, None, None, 0, None, None, 0.0, 0.0, 0.0) == "chr\trs\tps\tn_miss\tallele1\tallele0\taf\tl_mle\tp_lrt\n"
    line = _format(b"0", b"ACGT_12", b"0", 3, b"0", b"1", 0.12345, 123.456789, 1.23456789e-12)
    assert line == "0\tACGT_12\t0\t3\t0\t1\t0.123\t1.234568e+02\t1.234568e-12\n"
    assert float(line.split("\t")[8]) == 1.234568e-12  # field 9 is what the pipeline's awk reads
    assert lib.kgwas_lmm_format_assoc(b"1", b"r", b"5", 0, b"A", b"C", 0.5, 1.0, 0.5, None, 0) == len("1\tr\t5\t0\tA\tC\t0.500\t1.000000e+00\t5.000000e-01\n")


def test_not_positive_semi_definite_is_refused_before_the_device():
    K = np.eye(5)
    K[0, 1] = K[1, 0] = 1.5  # eigenvalue -0.5
    h = C.c_void_p()
    rc = lib.kgwas_lmm_create(5, ptr(K), 0, 1e-5, 1e5, 0, C.byref(h))
    assert rc == capi.KGWAS_ERR_FORMAT and _err(rc) == "Kinship matrix is not positive semi-definite"
    for bad in ((0.0, 1e5), (1e-5, 1e-5), (1e-5, float("inf"))):
        assert lib.kgwas_lmm_create(5, ptr(np.eye(5)), 0, bad[0], bad[1], 0, C.byref(h)) == capi.KGWAS_ERR_ARG
    assert lib.kgwas_lmm_create(2, ptr(np.eye(2)), 0, 1e-5, 1e5, 0, C.byref(h)) == capi.KGWAS_ERR_ARG


def test_kinship_size_mismatch_in_run_files(tmp_path):
    base = tmp_path / "b"
    (tmp_path / "b.fam").write_text("".join("f i%d 0 0 0 %d.5\n" % (i, i) for i in range(6)))
    (tmp_path / "b.bim").write_text("0\tA\t0\t0\t0\t1\n")
    (tmp_path / "b.bed").write_bytes(bytes([0x6C, 0x1B, 0x01, 0x0F, 0x03]))
    kin = tmp_path / "k.txt"
    kin.write_text("\n".join("\t".join("1" if r == c else "0" for c in range(5)) for r in range(5)) + "\n")
    bases = (C.c_char_p * 1)(str(base).encode())
    outs = (C.c_char_p * 1)(str(tmp_path / "o.assoc.txt").encode())
    rc = lib.kgwas_lmm_run_files(str(kin).encode(), 1, bases, outs, 1, 0.0, 1.0, 1e-5, 1e5, 0, 0, None)
    assert rc == capi.KGWAS_ERR_FORMAT and "5 rows" in _err(rc) and "6 individuals" in _err(rc)
    assert not os.path.exists(tmp_path / "o.assoc.txt")


def test_symbols_exported():
    for s in ("kgwas_sym_eigen", "kgwas_lmm_create", "kgwas_lmm_null", "kgwas_lmm_test_bed", "kgwas_lmm_run_files",
              "kgwas_lmm_get_stats", "kgwas_lmm_destroy"):
        assert s in capi.SYMBOLS and hasattr(lib, s)
