"""lmm_lrt -lmm 4 without a GPU: what the tool refuses (before any file is opened or any device work starts) and the bytes of the
14-column line (kgwas_lmm_format_assoc4)."""
import ctypes as C
import os
import subprocess

import pytest

from kmersgwas_amd import capi
from kmersgwas_amd.capi import lib

BIN = os.path.join(os.path.dirname(os.path.abspath(capi.__file__)), "bin", "lmm_lrt")
HEADER4 = "chr\trs\tps\tn_miss\tallele1\tallele0\taf\tbeta\tse\tl_remle\tl_mle\tp_wald\tp_lrt\tp_score\n"


def _run(tmp_path, args):
    """The tool on files that do not exist: a refusal that comes first never looks for them. Returns (status, stderr, outdir)."""
    outdir = str(tmp_path / "out")
    r = subprocess.run([BIN] + args + ["-k", str(tmp_path / "none.kinship"), "-outdir", outdir], capture_output=True, text=True, timeout=60)
    return r.returncode, r.stderr, outdir


@pytest.mark.parametrize("option,args", [
    ("--columns", ["-bfile", "B", "--columns", "LIST"]),
    ("--kmers_table", ["--kmers_table", "T", "--kmers_len", "31", "-p", "PHENO"]),
    ("--pheno_columns", ["--kmers_table", "T", "--kmers_len", "31", "-p", "PHENO", "--pheno_columns", "LIST"]),
])
def test_lmm4_is_refused_outside_the_bed_routes(tmp_path, option, args):
    status, err, outdir = _run(tmp_path, ["-lmm", "4"] + args)
    assert status == 1, err
    assert "-lmm 4" in err and option in err, err
    assert "find file" not in err and "can't open" not in err, "a file was looked for before the refusal: " + err
    assert not os.path.exists(outdir)


@pytest.mark.parametrize("mode", ["1", "3", "0", "5", "two"])
@pytest.mark.parametrize("route", [["-bfile", "B", "-o", "W"], ["--kmers_table", "T", "--kmers_len", "31", "-p", "PHENO"]])
def test_other_modes_stay_refused(tmp_path, mode, route):
    status, err, outdir = _run(tmp_path, ["-lmm", mode] + route)
    assert status == 1, err
    assert "only -lmm 2" in err and "-lmm " + mode in err and "-lmm 4" in err, err
    assert not os.path.exists(outdir)


def test_missing_mode_is_refused(tmp_path):
    status, err, outdir = _run(tmp_path, ["-bfile", "B"])
    assert status == 1 and "only -lmm 2" in err and not os.path.exists(outdir)


def test_usage_names_the_mode():
    r = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "-lmm 4" in r.stderr and "p_wald" in r.stderr and "p_score" in r.stderr


def _format4(*a):
    buf = C.create_string_buffer(1024)
    need = lib.kgwas_lmm_format_assoc4(*a, buf, 1024)
    return buf.raw[:need].decode()


def _format2(*a):
    buf = C.create_string_buffer(512)
    need = lib.kgwas_lmm_format_assoc(*a, buf, 512)
    return buf.raw[:need].decode()


def test_assoc4_formatting():
    assert _format4(None, None, None, 0, None, None, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0) == HEADER4
    assert len(HEADER4.rstrip("\n").split("\t")) == 14
    line = _format4(b"3", b"ACGT_12", b"77", 3, b"A", b"C", 0.12345, -1.23456789, 0.0123456789, 2.5, 123.456789, 1.23456789e-12, 9.87654321e-11, 0.5)
    assert line == "3\tACGT_12\t77\t3\tA\tC\t0.123\t-1.234568e+00\t1.234568e-02\t2.500000e+00\t1.234568e+02\t1.234568e-12\t9.876543e-11\t5.000000e-01\n"
    # columns 1-7, l_mle and p_lrt have the bytes of the -lmm 2 line
    f4 = line.rstrip("\n").split("\t")
    f2 = _format2(b"3", b"ACGT_12", b"77", 3, b"A", b"C", 0.12345, 123.456789, 9.87654321e-11).rstrip("\n").split("\t")
    assert f4[:7] == f2[:7] and f4[10] == f2[7] and f4[12] == f2[8]
    # the bytes needed are returned without a buffer, and nothing is written into one that is too small
    assert lib.kgwas_lmm_format_assoc4(b"3", b"ACGT_12", b"77", 3, b"A", b"C", 0.12345, -1.23456789, 0.0123456789, 2.5, 123.456789, 1.23456789e-12,
                                       9.87654321e-11, 0.5, None, 0) == len(line)
    small = C.create_string_buffer(b"\x7f" * 8, 8)
    lib.kgwas_lmm_format_assoc4(b"3", b"ACGT_12", b"77", 3, b"A", b"C", 0.1, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, small, 8)
    assert small.raw == b"\x7f" * 8
    assert lib.kgwas_lmm_format_assoc4(b"3", None, b"77", 3, b"A", b"C", 0.1, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, None, 0) == 0


def test_assoc4_formatting_of_a_p_below_the_normal_doubles():
    """a p that underflows is printed as a number that parses back (a subnormal or 0), never as nan"""
    for p in (0.0, 4.9406564584124654e-324, 1.5e-310, 2.2250738585072014e-308):
        f = _format4(b"1", b"r", b"5", 0, b"A", b"C", 0.5, 1.0, 0.1, 1.0, 1.0, p, p, p).rstrip("\n").split("\t")
        assert len(f) == 14
        for k in (11, 12, 13):
            back = float(f[k])
            assert "nan" not in f[k].lower() and "inf" not in f[k].lower() and back == float("%.6e" % p), (p, f[k])
            assert 0.0 <= back <= 2.3e-308
    assert _format4(b"1", b"r", b"5", 0, b"A", b"C", 0.5, 1.0, 0.1, 1.0, 1.0, 0.0, 0.0, 4.9406564584124654e-324) == \
        "1\tr\t5\t0\tA\tC\t0.500\t1.000000e+00\t1.000000e-01\t1.000000e+00\t1.000000e+00\t0.000000e+00\t0.000000e+00\t4.940656e-324\n"


def test_symbols_exported():
    for s in ("kgwas_lmm_null_reml", "kgwas_lmm_test_bed_all", "kgwas_lmm_run_files_all", "kgwas_lmm_format_assoc4", "kgwas_fdist_tail"):
        assert s in capi.SYMBOLS and hasattr(lib, s)
    assert lib.kgwas_abi_version() == 15
