"""lmm_lrt --pattern_cache without a GPU: the refusals of the tool (each a non-zero exit, its message, no output directory and no
file looked for), the new entry points and their argument checks, and the fixtures of test_gpu_lmm_lrt_table_unique.py: numpy
asserts what they are for."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from kmersgwas_amd import capi
from kmersgwas_amd.capi import lib

import lmm_table_np as T
import lmm_unique_np as Q

BIN = os.path.join(os.path.dirname(os.path.abspath(capi.__file__)), "bin", "lmm_lrt")
TABLE = ["--kmers_table", "absent_table", "--kmers_len", "31", "-p", "absent_pheno", "-k", "absent_kinship"]


def run(tmp_path, args):
    out = str(tmp_path / "out")
    r = subprocess.run([BIN, "-lmm", "2", "-outdir", out, "-o", "res"] + args, capture_output=True, text=True, timeout=120)
    assert not os.path.exists(out), "an output directory was made"
    assert "Couldn't find file" not in r.stderr and "can't open" not in r.stderr, r.stderr
    return r


def test_pattern_cache_needs_the_table(tmp_path):
    for args in (["-bfile", "B", "-k", "K"], ["--bfiles", "LIST", "-k", "K"], ["-bfile", "B", "--columns", "LIST", "-k", "K"]):
        r = run(tmp_path, args + ["--pattern_cache", "64"])
        assert r.returncode == 1 and "option 'pattern_cache' needs --kmers_table" in r.stderr, r.stderr


def test_pattern_cache_excludes_pheno_columns(tmp_path):
    r = run(tmp_path, TABLE + ["--pheno_columns", "absent_list", "--pattern_cache", "64"])
    assert r.returncode == 1 and "--pattern_cache is not built for --pheno_columns" in r.stderr, r.stderr


@pytest.mark.parametrize("value", ["0", "00", "1.5", "-1", "x", "", "64MiB"])
def test_pattern_cache_takes_a_whole_number(tmp_path, value):
    r = run(tmp_path, TABLE + ["--pattern_cache", value])
    assert r.returncode == 1 and "of --pattern_cache is not a whole number within 1.." in r.stderr, r.stderr


def test_pattern_cache_needs_a_value(tmp_path):
    r = run(tmp_path, TABLE + ["--pattern_cache"])
    assert r.returncode == 1 and "is missing an argument" in r.stderr, r.stderr


def test_a_good_value_gets_as_far_as_the_files(tmp_path):
    """the option itself is taken: the next thing the tool misses is its first input file"""
    out = str(tmp_path / "out")
    r = subprocess.run([BIN, "-lmm", "2", "-outdir", out] + TABLE + ["--pattern_cache", "64"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "Couldn't find file: absent_table.names" in r.stderr and not os.path.exists(out), r.stderr


def test_help_names_the_option():
    r = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--pattern_cache MIB" in r.stderr


def test_entry_points():
    assert capi.ABI_VERSION == 15 and lib.kgwas_abi_version() == 15
    for s in ("kgwas_lmm_test_table_unique", "kgwas_lmm_run_table_unique"):
        assert s in capi.SYMBOLS and hasattr(lib, s)
    assert [k for k, _ in capi.LmmUniqueStats._fields_] == ["slots", "patterns_cached", "rows_from_cache", "rows_collided", "rows_rejected",
                                                            "rows_rotated"]
    assert C.sizeof(capi.LmmUniqueStats) == 48
    y = np.zeros(4)
    us = capi.LmmUniqueStats(*([7] * 6))
    assert lib.kgwas_lmm_test_table_unique(None, capi.ptr(y), None, None, 4, 1, 0.0, 10, *([None] * 9), 4096, C.byref(us)) == capi.KGWAS_ERR_ARG
    run_args = (b"k", None, b"t", 31, b"p", 1, 5, 0.05, 10, 1e-5, 1e5, 0, 0, b"o", None)
    assert lib.kgwas_lmm_run_table_unique(*run_args, 0, C.byref(us)) == capi.KGWAS_ERR_ARG
    assert b"cache_mib is 0" in lib.kgwas_last_error()
    assert lib.kgwas_lmm_run_table_unique(None, None, b"t", 31, b"p", 1, 5, 0.05, 10, 1e-5, 1e5, 0, 0, b"o", None, 64, None) == capi.KGWAS_ERR_ARG
    assert lib.kgwas_lmm_run_table_unique(b"k", None, b"t", 31, b"p", 1, 5, 0.05, 0, 1e-5, 1e5, 0, 0, b"o", None, 64, None) == capi.KGWAS_ERR_ARG
    assert us.as_dict() == {k: 7 for k, _ in capi.LmmUniqueStats._fields_}, "a refused call wrote the counters"


@pytest.mark.parametrize("S,S_f", Q.PANELS + [Q.WIDE])
def test_repeated_pattern_fixture(S, S_f):
    """The tables of test_gpu_lmm_lrt_table_unique.py: 3000 rows of about 300 patterns; what the cache must meet in them is there
    at every piece and chunk the GPU tests run."""
    bits = Q.repeated_bits(S)
    assert bits.shape == (Q.ROWS, S)
    tested = Q.tested_of(bits, S)
    words = 1 + (S_f + 63) // 64
    distinct = Q.assert_fixture(bits, tested, words, sub_chunks=S != 5)
    all_patterns = len(np.unique(np.packbits(bits, axis=1), axis=0))
    print("S=%d: %d rows, %d patterns, %d tested rows of %d distinct patterns" % (S, Q.ROWS, all_patterns, int(tested.sum()), distinct))
    assert distinct <= all_patterns <= Q.PATTERNS
    if S >= 64:
        assert distinct > 3 * 64, "too few patterns to fill a cache of 64 slots"
        assert (S + 15) // 16 == {64: 4, 67: 5, 241: 16, 1135: 71}[S]  # dwords of a code row
    # the column map: the identity, or a shuffled choice among more columns
    pick = Q.pick_of(S, S_f)
    assert len(set(pick.tolist())) == S and (S_f == S or (pick != np.arange(S)).any())
    assert Q.min_count_of(S) == (1 if S == 5 else int(lib.kgwas_min_count(S, Q.MAF, 5)))
