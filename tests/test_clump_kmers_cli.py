"""clump_kmers without a GPU: the refusals of the tool - each exit 1 with its message, no output file, and the table never looked
for -, the threshold's text, and the argument checks of kgwas_kmers_ld and kgwas_clump_kmers_run, which come before any device
call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kmersgwas_amd as kg
from kmersgwas_amd import capi
from kmersgwas_amd.capi import lib
from oracle import oracle_np as onp

import lmm_table_np as T

BIN = os.path.join(os.path.dirname(os.path.abspath(capi.__file__)), "bin", "clump_kmers")
K = 31
HEAD9 = "chr\trs\tps\tn_miss\tallele1\tallele0\taf\tl_mle\tp_lrt\n"
GOOD = "ACGT" * 7 + "ACG"


def line9(rs, p="1.000000e-05"):
    return "0\t%s\t0\t0\t0\t1\t0.300\t1.000000e+00\t%s\n" % (rs, p)


def run(tmp_path, args, assoc_text=None):
    out = tmp_path / "clumps.txt"
    cmd = [BIN, "-o", str(out)] + args
    if assoc_text is not None:
        (tmp_path / "in.assoc.txt").write_text(assoc_text)
        cmd += ["--assoc", str(tmp_path / "in.assoc.txt"), "--kmers_table", "absent_table", "--kmers_len", str(K)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert not out.exists() and not os.path.exists(str(out) + ".log.txt"), "an output file was written"
    assert "absent_table" not in r.stderr, "the table was looked for: " + r.stderr
    return r


def test_missing_options(tmp_path):
    r = run(tmp_path, ["--kmers_table", "absent_tab", "--kmers_len", "31"])
    assert r.returncode == 1 and "option --assoc is missing" in r.stderr, r.stderr
    r = run(tmp_path, ["--assoc", "absent_assoc", "--kmers_len", "31"])
    assert r.returncode == 1 and "option --kmers_table is missing" in r.stderr, r.stderr
    r = run(tmp_path, ["--assoc", "absent_assoc", "--kmers_table", "absent_table", "--kmers_len", "31"])
    assert r.returncode == 1 and "Couldn't find file: absent_assoc" in r.stderr, r.stderr
    r = run(tmp_path, ["--assoc", "absent_assoc", "--kmers_table", "absent_table", "--kmers_len", "31", "--r3", "1"])
    assert r.returncode == 1 and "Option 'r3' does not exist" in r.stderr, r.stderr


@pytest.mark.parametrize("value", ["0", "1.0000001", "0.1234567", "abc", "0.0", "-0.5", "1e-1", "2", "", "."])
def test_r2_text_is_refused(tmp_path, value):
    r = run(tmp_path, ["--r2", value], HEAD9 + line9(GOOD))
    assert r.returncode == 1 and "--r2 '%s' is not a decimal number" % value in r.stderr, r.stderr


def test_r2_text_is_read_digit_by_digit():
    for text, tm in (("0.8", 800000), ("1", 1000000), ("1.000000", 1000000), ("0.000001", 1), (".25", 250000), ("0.123456", 123456), ("0.3", 300000)):
        out = C.c_uint32(0)
        assert lib.kgwas_r2_millionths(text.encode(), C.byref(out)) == capi.KGWAS_OK and out.value == tm, text
    assert [kg.r2_millionths(v) for v in (0.8, 0.3, 1, 1.0, 0.25, "0.7")] == [800000, 300000, 1000000, 1000000, 250000, 700000]
    with pytest.raises(kg.KgwasError):
        kg.r2_millionths(0.0)


def test_kmers_len(tmp_path):
    r = run(tmp_path, ["--assoc", "absent_assoc", "--kmers_table", "absent_tab", "--kmers_len", "9"])
    assert r.returncode == 1 and "kmer length has to be between 10-31" in r.stderr, r.stderr


def test_assoc_refusals(tmp_path):
    cases = [
        ("chr\trs\tps\tp_wald\n0\t%s\t0\t0.5\n" % GOOD, "the header has no column 'p_lrt'"),
        ("chr\tsnp\tp_lrt\n0\t%s\t0.5\n" % GOOD, "the header has no column 'rs'"),
        (HEAD9 + line9(GOOD) + line9(GOOD[:-1]), "line 3: k-mer '%s' has length 30, not 31" % GOOD[:-1]),
        (HEAD9 + line9(GOOD[:-1] + "N"), "line 2: k-mer '%sN' has a letter other than A, C, G, T" % GOOD[:-1]),
        (HEAD9 + line9(GOOD) + line9("C" * 31) + line9(GOOD), "line 4: duplicate k-mer '%s' (the k-mer of line 2)" % GOOD),
        (HEAD9 + line9("A" * 31) + line9("T" * 31), "line 3: duplicate k-mer"),  # its reverse complement: the same k-mer of the table
        (HEAD9 + line9(GOOD) + "0\t%s\t0\t0\n" % ("C" * 31), "line 3: too few fields (4, the header has 9)"),
        (HEAD9 + line9(GOOD, "NA"), "line 2: p_lrt 'NA' is not a number"),
        (HEAD9 + line9(GOOD, "nan"), "line 2: p_lrt 'nan' is not a number"),
        (HEAD9 + line9(GOOD, "1e-5x"), "line 2: p_lrt '1e-5x' is not a number"),
    ]
    for text, msg in cases:
        r = run(tmp_path, [], text)
        assert r.returncode == 1 and msg in r.stderr, (msg, r.stderr)


def test_a_good_file_gets_as_far_as_the_table(tmp_path):
    out = tmp_path / "clumps.txt"
    (tmp_path / "in.assoc.txt").write_text(HEAD9 + line9(GOOD) + line9("C" * 31, "3e-9"))
    r = subprocess.run([BIN, "-o", str(out), "--assoc", str(tmp_path / "in.assoc.txt"), "--kmers_table", "absent_table", "--kmers_len", "31",
                        "--r2", "0.5", "--p_max", "1e-3"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "absent_table" in r.stderr and not out.exists(), r.stderr


def test_an_accession_listed_twice(tmp_path):
    """a real table of three rows and a phenotype file that names one of its accessions twice: refused before any device call"""
    rows = T.table_from_bits(T.random_bits(3, 5, 1, 0.2, 0.8), 6, np.arange(5), 1)
    base = str(tmp_path / "tab")
    onp.write_table(base, ["acc%d" % i for i in range(6)], K, rows[:, 0], rows[:, 1:])
    ph = tmp_path / "twice.tsv"
    ph.write_text("accession_id\tv\n" + "".join("acc%d\t%d\n" % (c, i) for i, c in enumerate((4, 1, 3, 1, 0))))
    (tmp_path / "in.assoc.txt").write_text(HEAD9 + line9(T.kmer_text(rows[1, 0])) + line9(T.kmer_text(rows[0, 0]), "3e-9"))
    out = tmp_path / "clumps.txt"
    r = subprocess.run([BIN, "-o", str(out), "--assoc", str(tmp_path / "in.assoc.txt"), "--kmers_table", base, "--kmers_len", str(K), "-p", str(ph)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "%s lists the accession acc1 twice" % ph in r.stderr, r.stderr
    assert not out.exists() and not os.path.exists(str(out) + ".log.txt"), "an output file was written"


def test_entry_points_and_argument_checks():
    for s in ("kgwas_r2_millionths", "kgwas_kmers_ld", "kgwas_clump_kmers_run"):
        assert s in capi.SYMBOLS and hasattr(lib, s)
    assert [k for k, _ in capi.ClumpStats._fields_] == ["hits_read", "hits_used", "clumps", "largest_clump", "linked_pairs", "accessions",
                                                         "search_ms", "ld_ms", "clump_ms"]
    assert C.sizeof(capi.ClumpStats) == 72
    bits, adj, n1 = np.zeros((4, 129), np.uint64), np.zeros((4, 1), np.uint32), np.zeros(4, np.uint32)
    p = capi.ptr
    bad = [
        (None, 4, 1, 64, 500000, p(adj), "null argument"),
        (p(bits), 4, 1, 64, 500000, None, "null argument"),
        (p(bits), 4, 129, 8193, 500000, p(adj), "8193 accessions"),
        (p(bits), 4, 1, 0, 500000, p(adj), "0 accessions"),
        (p(bits), 4, 1, 64, 0, p(adj), "r2_millionths must be within 1..1000000"),
        (p(bits), 4, 1, 64, 1000001, p(adj), "r2_millionths must be within 1..1000000"),
        (p(bits), 4, 1, 65, 500000, p(adj), "words_per_row is too small"),
        (p(bits), (1 << 20) + 1, 1, 64, 500000, p(adj), "1048577 k-mers"),
    ]
    for b, n_kmers, words, n_acc, tm, a, msg in bad:
        assert lib.kgwas_kmers_ld(b, n_kmers, words, n_acc, tm, 0, 0, a, p(n1)) == capi.KGWAS_ERR_ARG, msg
        assert msg in lib.kgwas_last_error().decode(), lib.kgwas_last_error()
    with pytest.raises(kg.KgwasError) as e:
        kg.kmers_ld(np.zeros((3, 129), np.uint64), 8193, "0.8")
    assert e.value.code == capi.KGWAS_ERR_ARG
    st = capi.ClumpStats()
    for args in ((None, 31, None, b"a", 800000, 1.0, 0, 0, b"o"), (b"t", 31, None, None, 800000, 1.0, 0, 0, b"o"), (b"t", 31, None, b"a", 800000, 1.0, 0, 0, None),
                 (b"t", 31, None, b"a", 0, 1.0, 0, 0, b"o"), (b"t", 31, None, b"a", 800000, float("nan"), 0, 0, b"o")):
        assert lib.kgwas_clump_kmers_run(*args, C.byref(st)) == capi.KGWAS_ERR_ARG
