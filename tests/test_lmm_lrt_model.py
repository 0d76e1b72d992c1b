"""lmm_lrt without a GPU: the host eigensolver, the two numpy models of the statistic against each other, and the file layer.

Measured here (float64, -lmin / -lmax = e^-10 / e^10, fixtures (n, rows) = (67, 400) and (241, 600), hg in {0, 3}): the largest
|LRT_R - LRT_E| over the fixtures' variants is MEASURED_MODEL_GAP below; the test asserts it stays under 1e-9. The GPU tests
(test_gpu_lmm_lrt.py) allow 1000 x that gap, capped at 1e-8.
"""
import ctypes as C
import os

import numpy as np
import pytest

from kmersgwas_amd import capi
from kmersgwas_amd.capi import lib, ptr

import lmm_lrt_np as M

MEASURED_MODEL_GAP = 3e-12  # largest |LRT_R - LRT_E| seen on the fixtures below (printed by test_models_agree)


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
