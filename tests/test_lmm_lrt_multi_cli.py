"""lmm_lrt --columns: the argument errors. Each exits 1 with its message before the kinship file is opened (the -k given here does
not exist) and before any device is touched."""
import os
import subprocess

import pytest

from kmersgwas_amd import capi

BIN = os.path.join(os.path.dirname(os.path.abspath(capi.__file__)), "bin", "lmm_lrt")


def run(tmp_path, args, listing="1\tA\n2\tB\n"):
    lst = tmp_path / "columns.txt"
    lst.write_text(listing)
    cmd = [BIN, "-lmm", "2", "-k", str(tmp_path / "no_such.kinship"), "-outdir", str(tmp_path / "out")]
    r = subprocess.run(cmd + [x if x != "LIST" else str(lst) for x in args], capture_output=True, text=True, timeout=60)
    assert not os.path.exists(tmp_path / "out" / "A.assoc.txt")
    return r


@pytest.mark.parametrize("args", [
    ["-bfile", "B", "--columns", "LIST", "--bfiles", "LIST"],
    ["--columns", "LIST", "--bfiles", "LIST"],
    ["-bfile", "B", "--columns", "LIST", "-n", "2"],
    ["--columns", "LIST"],
    ["-bfile", "B", "--columns", "LIST", "-o", "NAME"],
])
def test_combinations(tmp_path, args):
    r = run(tmp_path, args)
    assert r.returncode == 1 and "--columns needs -bfile and excludes --bfiles, -n and -o" in r.stderr, r.stderr


@pytest.mark.parametrize("listing", ["1\tA\n2 B\n", "1\tA\n\tB\n", "1\tA\n2\t\n", "1\tA\nx2\tB\n", "1\tA\n-2\tB\n", "1\tA\n2\tB\tC\n"])
def test_malformed_line(tmp_path, listing):
    r = run(tmp_path, ["-bfile", "B", "--columns", "LIST"], listing)
    assert r.returncode == 1 and "a line is not 'col<TAB>name'" in r.stderr, r.stderr


def test_duplicate_name(tmp_path):
    r = run(tmp_path, ["-bfile", "B", "--columns", "LIST"], "1\tA\n2\tB\n3\tA\n")
    assert r.returncode == 1 and "the name 'A' is given twice" in r.stderr, r.stderr


def test_column_zero(tmp_path):
    r = run(tmp_path, ["-bfile", "B", "--columns", "LIST"], "1\tA\n0\tB\n")
    assert r.returncode == 1 and "phenotype columns start at 1" in r.stderr, r.stderr


def test_empty_list_and_missing_file(tmp_path):
    r = run(tmp_path, ["-bfile", "B", "--columns", "LIST"], "\n")
    assert r.returncode == 1 and "lists no column" in r.stderr, r.stderr
    r = run(tmp_path, ["-bfile", "B", "--columns", str(tmp_path / "absent.txt")])
    assert r.returncode == 1 and "can't open" in r.stderr, r.stderr


def test_well_formed_list_reaches_the_files(tmp_path):
    """The same command with a good list gets past the argument checks: it fails on the .fam that is not there, still exit 1."""
    r = run(tmp_path, ["-bfile", str(tmp_path / "B"), "--columns", "LIST"])
    assert r.returncode == 1 and "can't open fam file" in r.stderr, r.stderr
