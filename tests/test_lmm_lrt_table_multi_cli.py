"""lmm_lrt --kmers_table --pheno_columns without a GPU: the new entry points, the refusals of the tool (each with exit 1, its
message and no output file) and the device error of a well-formed command line on a machine without a GPU."""
import os
import subprocess

import numpy as np
import pytest

from kmersgwas_amd import capi
from kmersgwas_amd.capi import lib
from oracle import oracle_np as onp

import lmm_table_np as T

BIN = os.path.join(os.path.dirname(os.path.abspath(capi.__file__)), "bin", "lmm_lrt")
S, S_F = 12, 14


@pytest.fixture
def files(tmp_path):
    """A table of 14 accessions, a phenotype file of 12 of them (three columns), their kinship matrix and a list of the columns."""
    rng = np.random.default_rng(2)
    pick = rng.permutation(S_F)[:S]
    rows = T.table_from_bits(T.random_bits(60, S, 2, 0.2, 0.8), S_F, pick, 2)
    names = ["acc%d" % i for i in range(S_F)]
    base = str(tmp_path / "tab")
    onp.write_table(base, names, T.K_LEN, rows[:, 0], rows[:, 1:])
    ph = tmp_path / "ph.tsv"
    ph.write_text("accession_id\ta\tb\tc\n" + "".join("%s\t%.4f\t%.4f\t%.4f\n" % (names[c], rng.normal(60, 9), rng.normal(), rng.normal())
                                                        for c in pick))
    G = (rng.random((200, S)) < 0.4).astype(np.float64)
    K = 1.0 - (G.T @ (1 - G) + (1 - G).T @ G) / 200
    kin = tmp_path / "ph.kinship"
    kin.write_text("\n".join("\t".join("%.17g" % v for v in r) for r in K) + "\n")
    lst = tmp_path / "cols.txt"
    lst.write_text("1\tp0\n3\tp2\n2\tp1\n")
    return {"T": base, "P": str(ph), "K": str(kin), "L": str(lst), "out": str(tmp_path / "out"), "tmp": tmp_path}


def run(files, args):
    cmd = [BIN, "-lmm", "2", "-outdir", files["out"]] + [files.get(a, a) if a in ("T", "P", "K", "L") else a for a in args]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=120)


def no_output(files):
    return not os.path.exists(files["out"]) or not os.listdir(files["out"])


GOOD = ["--kmers_table", "T", "--kmers_len", "31", "-p", "P", "-k", "K", "--mac", "2", "-maf", "0.05", "--pheno_columns", "L"]


def test_entry_points():
    """The two entry points exist (they do not before this route was built), under the unchanged version number."""
    assert capi.ABI_VERSION == 15 and lib.kgwas_abi_version() == 15
    for s in ("kgwas_lmm_test_table_multi", "kgwas_lmm_run_table_multi"):
        assert s in capi.SYMBOLS and hasattr(lib, s)


def test_argument_errors_of_the_library():
    Y = np.zeros((2, 4))
    col = np.arange(4, dtype=np.uint64)
    none12 = [None] * 12
    # a NULL handle, with and without columns (n_pheno == 0), and best_n == 0
    assert lib.kgwas_lmm_test_table_multi(None, 2, capi.ptr(Y), None, capi.ptr(col), 4, 1, 0.0, 10, *none12) == capi.KGWAS_ERR_ARG
    assert lib.kgwas_lmm_test_table_multi(None, 0, None, None, capi.ptr(col), 4, 1, 0.0, 10, *none12) == capi.KGWAS_ERR_ARG
    assert lib.kgwas_lmm_test_table_multi(None, 2, capi.ptr(Y), None, capi.ptr(col), 4, 1, 0.0, 0, *none12) == capi.KGWAS_ERR_ARG
    cols = np.array([1, 2], np.uint32)
    outs = (capi.C.c_char_p * 2)(b"o1", b"o2")
    good = lambda **kw: dict(dict(k=b"k", t=b"t", p=b"p", n=2, cols=capi.ptr(cols), outs=outs, best=10), **kw)  # noqa: E731

    def call(a):
        return lib.kgwas_lmm_run_table_multi(a["k"], a["t"], 31, a["p"], a["n"], a["cols"], a["outs"], 5, 0.05, a["best"], 1e-5, 1e5, 0, 0, None)

    for bad in (dict(k=None), dict(t=None), dict(p=None), dict(cols=None), dict(outs=None), dict(n=0), dict(best=0)):
        assert call(good(**bad)) == capi.KGWAS_ERR_ARG, bad
    assert call(good(outs=(capi.C.c_char_p * 2)(b"o1", None))) == capi.KGWAS_ERR_ARG
    assert call(good(cols=capi.ptr(np.array([1, 0], np.uint32)))) == capi.KGWAS_ERR_ARG
    assert call(good()) != capi.KGWAS_OK  # (the files do not exist)


def test_needs_the_table(files):
    r = run(files, ["-bfile", "B", "-k", "K", "--pheno_columns", "L"])
    assert r.returncode == 1 and "option 'pheno_columns' needs --kmers_table" in r.stderr, r.stderr
    assert no_output(files)


@pytest.mark.parametrize("extra", [["-n", "2"], ["-o", "res"], ["-n", "1", "-o", "res"]])
def test_excludes_n_and_o(files, extra):
    r = run(files, GOOD + extra)
    assert r.returncode == 1 and "--pheno_columns excludes -n and -o" in r.stderr, r.stderr
    assert no_output(files)


def test_columns_stays_refused_in_table_mode(files):
    for extra in (["--columns", "L"], ["--columns", "L", "--pheno_columns", "L"]):
        r = run(files, GOOD[:-2] + extra)
        assert r.returncode == 1 and "--kmers_table excludes -bfile, --bfiles and --columns" in r.stderr, r.stderr
        assert no_output(files)


@pytest.mark.parametrize("text,msg", [
    ("1 p0\n", "a line is not 'col<TAB>name': 1 p0"),
    ("1\tp0\nx\tp1\n", "a line is not 'col<TAB>name': x\tp1"),
    ("1\t\n", "a line is not 'col<TAB>name'"),
    ("1\tp0\tmore\n", "a line is not 'col<TAB>name'"),
    ("1234567\tp0\n", "a line is not 'col<TAB>name'"),
    ("0\tp0\n", "phenotype columns start at 1: 0\tp0"),
    ("1\tp0\n2\tp0\n", "the name 'p0' is given twice"),
    ("\n\n", "lists no column"),
    ("", "lists no column"),
])
def test_bad_lists(files, text, msg):
    lst = files["tmp"] / "bad.txt"
    lst.write_text(text)
    args = list(GOOD)
    args[args.index("L")] = str(lst)
    r = run(files, args)
    assert r.returncode == 1 and msg in r.stderr and str(lst) in r.stderr, r.stderr
    assert no_output(files)


def test_missing_list(files):
    args = list(GOOD)
    args[args.index("L")] = str(files["tmp"] / "absent.txt")
    r = run(files, args)
    assert r.returncode == 1 and "can't open " + str(files["tmp"] / "absent.txt") in r.stderr, r.stderr
    assert no_output(files)


def test_column_beyond_the_file(files):
    lst = files["tmp"] / "far.txt"
    lst.write_text("1\tp0\n4\tp3\n")
    args = list(GOOD)
    args[args.index("L")] = str(lst)
    r = run(files, args)
    assert r.returncode == 1 and "has no phenotype column 4" in r.stderr, r.stderr
    assert no_output(files)


@pytest.mark.parametrize("args,msg", [
    (["--best", "0"], "--best 0"),
    (["--best", "x"], "is not a whole number"),
    (["--kmers_len", "32"], "kmer length has to be between 10-31"),
    (["-maf", "abc"], "failed to parse"),
])
def test_bad_values(files, args, msg):
    base = list(GOOD)
    if args[0] in base:
        i = base.index(args[0])
        del base[i:i + 2]
    r = run(files, base + args)
    assert r.returncode == 1 and msg in r.stderr, r.stderr
    assert no_output(files)


def test_a_value_that_a_fam_reads_as_missing_is_refused(files):
    """in the LAST listed column, after the others were converted: still no output"""
    lines = open(files["P"]).read().split("\n")
    f = lines[3].split("\t")
    lines[3] = "\t".join([f[0], f[1], "-9.0", f[3]])
    ph = files["tmp"] / "minus9.tsv"
    ph.write_text("\n".join(lines))
    args = list(GOOD)
    args[args.index("P")] = str(ph)
    r = run(files, args)
    assert r.returncode == 1 and "a .fam reads as missing" in r.stderr and f[0] in r.stderr, r.stderr
    assert no_output(files)


def test_well_formed_command_line(files, have_gpu):
    """Without a GPU: the device error and exit code 3 of every tool here, after every file was read, and no output. With one
    the same line runs and writes one result and one log per listed column."""
    r = run(files, GOOD)
    if have_gpu:
        assert r.returncode == 0, r.stderr
        assert sorted(os.listdir(files["out"])) == sorted("p%d.%s.txt" % (k, e) for k in range(3) for e in ("assoc", "log"))
        for k in range(3):
            lines = open(os.path.join(files["out"], "p%d.assoc.txt" % k)).read().split("\n")
            assert lines[0].startswith("chr\trs\t") and len(lines) > 10 and all(len(l.split("\t")[1]) == 31 for l in lines[1:-1])
            assert "phenotype_column\t%d\n" % (1, 2, 3)[k] in open(os.path.join(files["out"], "p%d.log.txt" % k)).read()
    else:
        assert r.returncode == 3 and "no HIP device available: libkgwas has no CPU fallback" in r.stderr, r.stderr
        assert no_output(files)


def test_help_names_the_option():
    r = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--pheno_columns" in r.stderr
