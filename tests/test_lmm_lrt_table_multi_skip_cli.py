"""lmm_lrt --pattern_skip without a GPU: the refusals of the tool (each a non-zero exit, its message, no output directory and no
file looked for), the value parsing, and the new entry points with their argument checks."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from kmersgwas_amd import capi
from kmersgwas_amd.capi import lib

BIN = os.path.join(os.path.dirname(os.path.abspath(capi.__file__)), "bin", "lmm_lrt")
TABLE = ["--kmers_table", "absent_table", "--kmers_len", "31", "-p", "absent_pheno", "-k", "absent_kinship"]
MULTI = TABLE + ["--pheno_columns", "absent_list"]
FIELDS = ["slots", "patterns_cached", "patterns_dead", "rows_skipped", "rows_collided", "rows_rejected", "rows_rotated"]


def run(tmp_path, args, named=True):
    out = str(tmp_path / "out")
    r = subprocess.run([BIN, "-lmm", "2", "-outdir", out] + (["-o", "res"] if named else []) + args, capture_output=True, text=True,
                       timeout=120)
    assert not os.path.exists(out), "an output directory was made"
    assert "Couldn't find file" not in r.stderr and "can't open" not in r.stderr, r.stderr
    return r


def test_pattern_skip_needs_pheno_columns(tmp_path):
    """with -n (or neither) the option is refused, and the message names the option that goes with one column"""
    for args in (TABLE, TABLE + ["-n", "2"], ["-bfile", "B", "-k", "K"], ["--bfiles", "LIST", "-k", "K"]):
        r = run(tmp_path, args + ["--pattern_skip", "64"])
        assert r.returncode == 1 and "--pattern_skip goes with --pheno_columns" in r.stderr and "--pattern_cache" in r.stderr, r.stderr


def test_pattern_skip_needs_the_table(tmp_path):
    r = run(tmp_path, ["-bfile", "B", "-k", "K", "--pheno_columns", "absent_list", "--pattern_skip", "64"], named=False)
    assert r.returncode == 1 and "needs --kmers_table" in r.stderr, r.stderr


def test_pattern_cache_with_pheno_columns_stays_refused(tmp_path):
    for extra in ([], ["--pattern_skip", "64"]):
        r = run(tmp_path, MULTI + ["--pattern_cache", "64"] + extra, named=False)
        assert r.returncode == 1 and "--pattern_cache is not built for --pheno_columns: the cache goes with one phenotype column (-n)" in r.stderr


@pytest.mark.parametrize("value", ["0", "00", "1.5", "-1", "x", "", "64MiB", "1048577"])
def test_pattern_skip_takes_a_whole_number(tmp_path, value):
    r = run(tmp_path, MULTI + ["--pattern_skip", value], named=False)
    assert r.returncode == 1 and "of --pattern_skip is not a whole number within 1..1048576" in r.stderr, r.stderr


def test_pattern_skip_needs_a_value(tmp_path):
    r = run(tmp_path, MULTI + ["--pattern_skip"], named=False)
    assert r.returncode == 1 and "is missing an argument" in r.stderr, r.stderr


@pytest.mark.parametrize("value", ["1", "64", "1048576"])
def test_a_good_value_gets_as_far_as_the_files(tmp_path, value):
    """the option itself is taken: the next thing the tool misses is its first input file"""
    out = str(tmp_path / "out")
    r = subprocess.run([BIN, "-lmm", "2", "-outdir", out] + MULTI + ["--pattern_skip", value], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "Couldn't find file: absent_table.names" in r.stderr and not os.path.exists(out), r.stderr


def test_help_names_the_option():
    r = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--pattern_skip MIB" in r.stderr and "--pattern_cache MIB | --pattern_skip MIB" in r.stderr


def test_entry_points():
    assert capi.ABI_VERSION == 15 and lib.kgwas_abi_version() == 15
    for s in ("kgwas_lmm_test_table_multi_skip", "kgwas_lmm_run_table_multi_skip"):
        assert s in capi.SYMBOLS and hasattr(lib, s)
    assert [k for k, _ in capi.LmmSkipStats._fields_] == FIELDS and C.sizeof(capi.LmmSkipStats) == 56
    Y = np.zeros((2, 4))
    ks = capi.LmmSkipStats(*([7] * 7))
    assert lib.kgwas_lmm_test_table_multi_skip(None, 2, capi.ptr(Y), None, None, 4, 1, 0.0, 10, *([None] * 12), 4096,
                                               C.byref(ks)) == capi.KGWAS_ERR_ARG
    cols = np.array([1, 2], np.uint32)
    outs = (C.c_char_p * 2)(b"o1", b"o2")
    run_args = (b"k", b"t", 31, b"p", 2, capi.ptr(cols), outs, 5, 0.05, 10, 1e-5, 1e5, 0, 0, None)
    assert lib.kgwas_lmm_run_table_multi_skip(*run_args, 0, C.byref(ks)) == capi.KGWAS_ERR_ARG
    assert b"cache_mib is 0" in lib.kgwas_last_error()
    assert lib.kgwas_lmm_run_table_multi_skip(None, *run_args[1:], 64, None) == capi.KGWAS_ERR_ARG
    no_best = run_args[:9] + (0,) + run_args[10:]
    assert lib.kgwas_lmm_run_table_multi_skip(*no_best, 64, None) == capi.KGWAS_ERR_ARG
    assert not os.path.exists("o1") and not os.path.exists("o2")
    assert ks.as_dict() == {k: 7 for k in FIELDS}, "a refused call wrote the counters"
