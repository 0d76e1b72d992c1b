"""lmm_lrt -c without a GPU: what the tool and the file layer refuse (before the kinship file is opened and before any device
work), the covariates parser (kgwas_lmm_read_covariates) and the usage text."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from kmersgwas_amd import capi
from kmersgwas_amd.capi import lib, ptr

BIN = os.path.join(os.path.dirname(os.path.abspath(capi.__file__)), "bin", "lmm_lrt")
N = 12


def _fam(tmp_path, n=N, missing=()):
    base = str(tmp_path / "B")
    rng = np.random.default_rng(2)
    open(base + ".fam", "w").write("".join("f%d i%d 0 0 0 %s\n" % (i, i, "-9" if i in missing else "%.4f" % rng.normal()) for i in range(n)))
    return base


def _cov(tmp_path, text):
    p = str(tmp_path / "covar.txt")
    open(p, "w").write(text)
    return p


def _rows(columns):
    return "".join(" ".join(str(v) for v in r) + "\n" for r in zip(*columns))


def _run(tmp_path, args):
    """The kinship file does not exist: a refusal that comes first never looks for it. Returns (status, stderr, outdir)."""
    outdir = str(tmp_path / "out")
    r = subprocess.run([BIN] + args + ["-k", str(tmp_path / "none.kinship"), "-outdir", outdir], capture_output=True, text=True, timeout=60)
    return r.returncode, r.stderr, outdir


ONE = [1] * N
Z = [0.5 * i * i - i for i in range(N)]


@pytest.mark.parametrize("option,args", [
    ("--columns", ["-bfile", "B", "--columns", "LIST"]),
    ("--pheno_columns", ["--kmers_table", "T", "--kmers_len", "31", "-p", "PHENO", "--pheno_columns", "LIST"]),
])
@pytest.mark.parametrize("mode", ["2", "4"])
def test_covariates_are_refused_with_several_columns(tmp_path, option, args, mode):
    status, err, outdir = _run(tmp_path, ["-lmm", mode, "-c", "COV"] + args)
    assert status == 1, err
    assert ("-c" in err or "-lmm 4" in err) and option in err, err
    assert "find file" not in err and "can't open" not in err, "a file was looked for before the refusal: " + err
    assert not os.path.exists(outdir)


REFUSALS = [
    ("wrong row count", _rows([ONE[:-1], Z[:-1]]), ["11 rows", "12 individuals"]),
    ("a non-number", _rows([ONE, Z]).replace("1 4.0", "1 four", 1), ["'four' is no number"]),
    ("ragged rows", _rows([ONE, Z]).replace("1 4.0\n", "1 4.0 2\n", 1), ["row 5", "3 fields"]),
    ("too many columns", _rows([ONE] + [[(i * (k + 3)) % 7 + 0.1 * k for i in range(N)] for k in range(8)]), ["9 columns", "at most 8"]),
    ("no constant", _rows([Z, [(-1) ** i for i in range(N)]]), ["do not span the constant", "column of 1s"]),
    ("rank", _rows([ONE, Z, [2 * z + 3 for z in Z]]), ["rank-deficient", "column 3"]),
]


@pytest.mark.parametrize("mode", ["2", "4"])
@pytest.mark.parametrize("name,text,needles", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_malformed_covariates_are_refused_before_the_kinship_file(tmp_path, name, text, needles, mode):
    assert "1 4.0\n" in _rows([ONE, Z])
    base = _fam(tmp_path)
    status, err, outdir = _run(tmp_path, ["-bfile", base, "-lmm", mode, "-c", _cov(tmp_path, text)])
    assert status == 1, err
    for needle in needles:
        assert needle in err, err
    assert "kinship" not in err and "HIP" not in err and "hip" not in err, err
    assert not os.path.exists(os.path.join(outdir, "result.assoc.txt"))


def test_too_few_individuals_are_refused(tmp_path):
    """12 .fam lines, 3 without a phenotype and 4 with an NA: 5 are left for q = 4, one short of q + 2"""
    base = _fam(tmp_path, missing=(0, 1, 2))
    cols = [ONE, Z, [i % 3 for i in range(N)], [(i * i) % 5 for i in range(N)]]
    text = _rows(cols).split("\n")
    for r in (3, 4, 5, 6):
        text[r] = text[r].rsplit(" ", 1)[0] + " NA"
    status, err, outdir = _run(tmp_path, ["-bfile", base, "-lmm", "2", "-c", _cov(tmp_path, "\n".join(text))])
    assert status == 1 and "5 individuals are too few for 4 covariate columns" in err and "kinship" not in err, err


def test_a_missing_covariates_file_is_named(tmp_path):
    base = _fam(tmp_path)
    status, err, _ = _run(tmp_path, ["-bfile", base, "-lmm", "2", "-c", str(tmp_path / "nope.txt")])
    assert status == 1 and "can't open covariates file" in err and "nope.txt" in err


def test_table_route_refuses_na_and_a_wrong_row_count(tmp_path):
    """through the C ABI, with a table and a kinship file that do not exist: the covariates are refused first"""
    ph = tmp_path / "pheno.txt"
    ph.write_text("accession_id\tv\n" + "".join("acc%d\t%.3f\n" % (i, 0.37 * i * i % 5) for i in range(N)))
    args = lambda cov: (str(tmp_path / "none.kinship").encode(), cov.encode(), str(tmp_path / "T").encode(), 31, str(ph).encode(), 1, 5, 0.01, 10,
                        1e-5, 1e5, 0, 0, str(tmp_path / "o.assoc.txt").encode(), None)
    text = _rows([ONE, Z]).replace("1 4.0\n", "1 NA\n", 1)
    assert lib.kgwas_lmm_run_table_cov(*args(_cov(tmp_path, text))) == capi.KGWAS_ERR_FORMAT
    msg = lib.kgwas_last_error().decode()
    assert "row 5 has an NA" in msg and "--kmers_table" in msg, msg
    assert lib.kgwas_lmm_run_table_cov(*args(_cov(tmp_path, _rows([ONE[:-2], Z[:-2]])))) == capi.KGWAS_ERR_FORMAT
    msg = lib.kgwas_last_error().decode()
    assert "10 rows" in msg and "the phenotype file has 12 individuals" in msg, msg
    assert lib.kgwas_lmm_run_table_cov(*args(_cov(tmp_path, _rows([Z])))) == capi.KGWAS_ERR_ARG
    assert "do not span the constant" in lib.kgwas_last_error().decode()
    # and with well-formed covariates the next thing looked for is the table
    assert lib.kgwas_lmm_run_table_cov(*args(_cov(tmp_path, _rows([ONE, Z])))) != capi.KGWAS_OK
    assert "covariates" not in lib.kgwas_last_error().decode()


def _read(path, n_expected=0, cap_rows=64, cap_cols=8):
    values, keep, q = np.full(cap_rows * cap_cols, -7.0), np.full(cap_rows, 9, np.uint8), C.c_uint32(77)
    rc = lib.kgwas_lmm_read_covariates(path.encode(), n_expected, values.size, ptr(values), ptr(keep), C.byref(q))
    return rc, q.value, values, keep


def test_read_covariates(tmp_path):
    p = _cov(tmp_path, "1 0.5\t-2e3\r\n1   NA 7\r\n\r\n 1 3 NA\n1 -0.25 1e-3")
    rc, q, values, keep = _read(p)
    assert rc == capi.KGWAS_OK and q == 3
    assert list(keep[:4]) == [1, 0, 0, 1] and keep[4] == 9
    v = values[:12].reshape(4, 3)
    np.testing.assert_array_equal(v[[0, 3]], [[1, 0.5, -2000.0], [1, -0.25, 0.001]])
    assert np.isnan(v[1, 1]) and np.isnan(v[2, 2]) and v[1, 2] == 7 and v[2, 1] == 3 and values[12] == -7.0
    assert _read(p, n_expected=4)[0] == capi.KGWAS_OK
    assert _read(p, n_expected=5)[0] == capi.KGWAS_ERR_FORMAT and "4 rows, expected 5" in lib.kgwas_last_error().decode()
    # q is reported, and nothing is written, when the values do not fit
    values, q = np.full(11, -7.0), C.c_uint32(0)
    assert lib.kgwas_lmm_read_covariates(p.encode(), 0, 11, ptr(values), None, C.byref(q)) == capi.KGWAS_OK and q.value == 3 and (values == -7.0).all()
    for text, needle in (("1 2\n1\n", "row 2 has 1 fields, row 1 has 2"), ("1 2\n1 x3\n", "'x3' is no number"), ("1 inf\n", "'inf' is no number"),
                         ("1 nan\n", "is no number"), ("1 2 3 4 5 6 7 8 9\n", "9 columns"), ("\n \n", "no rows")):
        assert _read(_cov(tmp_path, text))[0] == capi.KGWAS_ERR_FORMAT, text
        assert needle in lib.kgwas_last_error().decode(), (text, lib.kgwas_last_error().decode())
    assert _read(str(tmp_path / "nope"))[0] == capi.KGWAS_ERR_IO
    assert lib.kgwas_lmm_read_covariates(None, 0, 0, None, None, None) == capi.KGWAS_ERR_ARG


def test_usage_names_the_option():
    r = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "-c FILE" in r.stderr and "column of 1s" in r.stderr and "[-c COVARIATES]" in r.stderr


def test_symbols_exported():
    for s in ("kgwas_lmm_set_covariates", "kgwas_lmm_read_covariates", "kgwas_lmm_run_files_cov", "kgwas_lmm_run_table_cov"):
        assert s in capi.SYMBOLS and hasattr(lib, s)
    assert lib.kgwas_abi_version() == 15
