"""proxy_kmers without a GPU: the refusals of the tool - each exit 1 with its message, no output file, and the table never looked
for -, the two formats of --leads, the usage text, and the argument checks of kgwas_kmers_ld_proxies and kgwas_proxy_kmers_run,
which come before any device call."""
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

BIN = os.path.join(os.path.dirname(os.path.abspath(capi.__file__)), "bin", "proxy_kmers")
K = 31
GOOD = "ACGT" * 7 + "ACG"
CLUMP_HEAD = "rs\tp_lrt\tclump\tlead\tr2\tn1\tn11\n"


def run(tmp_path, args, leads_text=None):
    out = tmp_path / "proxies.txt"
    cmd = [BIN, "-o", str(out)] + args
    if leads_text is not None:
        (tmp_path / "leads.txt").write_text(leads_text)
        cmd += ["--leads", str(tmp_path / "leads.txt"), "--kmers_table", "absent_table", "--kmers_len", str(K)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert not out.exists() and not os.path.exists(str(out) + ".log.txt"), "an output file was written"
    assert "absent_table" not in r.stderr, "the table was looked for: " + r.stderr
    return r


def test_missing_options(tmp_path):
    r = run(tmp_path, ["--kmers_table", "absent_tab", "--kmers_len", "31"])
    assert r.returncode == 1 and "option --leads is missing" in r.stderr, r.stderr
    r = run(tmp_path, ["--leads", "absent_leads", "--kmers_len", "31"])
    assert r.returncode == 1 and "option --kmers_table is missing" in r.stderr, r.stderr
    r = run(tmp_path, ["--leads", "absent_leads", "--kmers_table", "absent_tab"])
    assert r.returncode == 1 and "option --kmers_len is missing" in r.stderr, r.stderr
    r = run(tmp_path, ["--leads", "absent_leads", "--kmers_table", "absent_table", "--kmers_len", "31", "--r3", "1"])
    assert r.returncode == 1 and "Option 'r3' does not exist" in r.stderr, r.stderr


def test_a_missing_leads_file(tmp_path):
    r = run(tmp_path, ["--leads", "absent_leads", "--kmers_table", "absent_table", "--kmers_len", "31"])
    assert r.returncode == 1 and "Couldn't find file: absent_leads" in r.stderr, r.stderr
    (tmp_path / "leads.txt").write_text(GOOD + "\n")
    r = run(tmp_path, ["--leads", str(tmp_path / "leads.txt"), "--kmers_table", "absent_table", "--kmers_len", "31", "-p", "absent_pheno"])
    assert r.returncode == 1 and "Couldn't find file: absent_pheno" in r.stderr, r.stderr


@pytest.mark.parametrize("value", ["0", "1.0000001", "0.1234567", "abc", "0.0", "-0.5", "1e-1", "2", "", "."])
def test_r2_text_is_refused(tmp_path, value):
    r = run(tmp_path, ["--r2", value], GOOD + "\n")
    assert r.returncode == 1 and "--r2 '%s' is not a decimal number" % value in r.stderr, r.stderr


@pytest.mark.parametrize("klen", ["9", "32"])
def test_kmers_len(tmp_path, klen):
    r = run(tmp_path, ["--leads", "absent_leads", "--kmers_table", "absent_tab", "--kmers_len", klen])
    assert r.returncode == 1 and "kmer length has to be between 10-31" in r.stderr, r.stderr


def test_leads_refusals(tmp_path):
    member = "0.5\t1\t%s\t0.9\t3\t3\n"
    cases = [
        (GOOD + "\n" + "C" * 31 + "\n" + GOOD + "\n", "line 3: duplicate k-mer '%s' (the k-mer of line 1)" % GOOD),
        ("A" * 31 + "\n" + "T" * 31 + "\n", "line 2: duplicate k-mer"),  # its reverse complement: the same k-mer of the table
        (GOOD + "\n" + GOOD[:-1] + "\n", "line 2: k-mer '%s' has length 30, not 31" % GOOD[:-1]),
        (GOOD[:-1] + "N\n", "line 1: k-mer '%sN' has a letter other than A, C, G, T" % GOOD[:-1]),
        (GOOD + "\t1\n", "line 1: 2 fields: a list of leads has one k-mer per line"),
        ("\n\n", "no lead k-mer"),
        (CLUMP_HEAD, "no lead k-mer"),
        (CLUMP_HEAD + ("C" * 31 + "\t") + member % GOOD[:-1], "line 2: k-mer '%s' has length 30, not 31" % GOOD[:-1]),
        (CLUMP_HEAD + ("C" * 31 + "\t") + member % (GOOD[:-1] + "X"), "line 2: k-mer '%sX' has a letter other than A, C, G, T" % GOOD[:-1]),
        (CLUMP_HEAD + "C" * 31 + "\t0.5\t1\n", "line 2: 3 fields, a clump_kmers line has 7"),
    ]
    for text, msg in cases:
        r = run(tmp_path, [], text)
        assert r.returncode == 1 and msg in r.stderr, (msg, r.stderr)


def good_as_far_as_the_table(tmp_path, text):
    out = tmp_path / "proxies.txt"
    (tmp_path / "leads.txt").write_text(text)
    r = subprocess.run([BIN, "-o", str(out), "--leads", str(tmp_path / "leads.txt"), "--kmers_table", "absent_table", "--kmers_len", "31", "--r2", "0.5",
                        "--max_per_lead", "3"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "absent_table" in r.stderr and not out.exists(), r.stderr


def test_a_good_list_gets_as_far_as_the_table(tmp_path):
    good_as_far_as_the_table(tmp_path, GOOD + "\n\n" + "C" * 31 + "\r\n" + "G" * 30 + "A")


def test_a_clump_kmers_output_is_recognised(tmp_path):
    """its header makes it one: the members' own k-mers (column rs) are not leads, so two members of one lead are no duplicate, and a
    member k-mer that would be refused in a list (here one of the lead's letters, short) is not looked at"""
    line = "%s\t1e-9\t%d\t%s\t1.000000\t4\t4\n"
    text = CLUMP_HEAD + line % (GOOD, 1, GOOD) + line % ("C" * 31, 1, GOOD) + line % ("ACGT", 2, "G" * 31) + line % ("T" * 31, 1, GOOD)
    good_as_far_as_the_table(tmp_path, text)
    # the same lines without the header are a list with 7 fields a line
    r = run(tmp_path, [], text[len(CLUMP_HEAD):])
    assert r.returncode == 1 and "line 1: 7 fields: a list of leads has one k-mer per line" in r.stderr, r.stderr


def test_an_accession_listed_twice(tmp_path):
    """a real table of three rows and a phenotype file that names one of its accessions twice: refused before any device call"""
    rows = T.table_from_bits(T.random_bits(3, 5, 1, 0.2, 0.8), 6, np.arange(5), 1)
    base = str(tmp_path / "tab")
    onp.write_table(base, ["acc%d" % i for i in range(6)], K, rows[:, 0], rows[:, 1:])
    ph = tmp_path / "twice.tsv"
    ph.write_text("accession_id\tv\n" + "".join("acc%d\t%d\n" % (c, i) for i, c in enumerate((4, 1, 3, 1, 0))))
    (tmp_path / "leads.txt").write_text(T.kmer_text(rows[1, 0]) + "\n")
    out = tmp_path / "proxies.txt"
    r = subprocess.run([BIN, "-o", str(out), "--leads", str(tmp_path / "leads.txt"), "--kmers_table", base, "--kmers_len", str(K), "-p", str(ph)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "%s lists the accession acc1 twice" % ph in r.stderr, r.stderr
    assert not out.exists() and not os.path.exists(str(out) + ".log.txt"), "an output file was written"


def test_usage_text():
    r = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0
    for word in ("--kmers_table", "--kmers_len", "--leads", "--pheno", "--r2", "--max_per_lead", "--output", "--device", "clump_kmers output"):
        assert word in r.stdout, word


def test_entry_points_and_argument_checks():
    for s in ("kgwas_kmers_ld_proxies", "kgwas_proxy_kmers_run"):
        assert s in capi.SYMBOLS and hasattr(lib, s)
    assert [k for k, _ in capi.ProxyStats._fields_] == ["accessions", "leads", "rows_read", "pairs_tested", "proxies_found", "proxies_kept",
                                                         "drain_rounds", "search_ms", "kernel_ms", "copy_ms", "total_ms"]
    assert C.sizeof(capi.ProxyStats) == 88 and C.sizeof(capi.ProxyRecord) == 32 and kg.PROXY_RECORD.itemsize == 32
    assert [(k, kg.PROXY_RECORD.fields[k][1]) for k in kg.PROXY_RECORD.names] == [("row", 0), ("kmer", 8), ("lead", 16), ("n1", 20), ("n11", 24), ("pad", 28)]
    leads, bits, rec, n = np.zeros((4, 129), np.uint64), np.zeros((4, 129), np.uint64), np.zeros(8, kg.PROXY_RECORD), C.c_uint64(7)
    p = capi.ptr
    bad = [
        (None, 4, p(bits), 4, 1, 64, 500000, p(rec), 8, C.byref(n), "null argument"),
        (p(leads), 4, None, 4, 1, 64, 500000, p(rec), 8, C.byref(n), "null argument"),
        (p(leads), 4, p(bits), 4, 1, 64, 500000, None, 8, C.byref(n), "null argument"),
        (p(leads), 4, p(bits), 4, 1, 64, 500000, p(rec), 8, None, "null argument"),
        (p(leads), 4, p(bits), 4, 129, 8193, 500000, p(rec), 8, C.byref(n), "8193 accessions"),
        (p(leads), 4, p(bits), 4, 1, 0, 500000, p(rec), 8, C.byref(n), "0 accessions"),
        (p(leads), 4097, p(bits), 4, 1, 64, 500000, p(rec), 8, C.byref(n), "4097 leads"),
        (p(leads), 0, p(bits), 4, 1, 64, 500000, p(rec), 8, C.byref(n), "0 leads"),
        (p(leads), 4, p(bits), 4, 1, 64, 0, p(rec), 8, C.byref(n), "r2_millionths must be within 1..1000000"),
        (p(leads), 4, p(bits), 4, 1, 64, 1000001, p(rec), 8, C.byref(n), "r2_millionths must be within 1..1000000"),
        (p(leads), 4, p(bits), 4, 1, 65, 500000, p(rec), 8, C.byref(n), "words_per_row is too small"),
    ]
    for a, L, b, R, words, n_acc, tm, r, cap, n_out, msg in bad:
        assert lib.kgwas_kmers_ld_proxies(a, L, b, R, words, n_acc, tm, 0, r, cap, n_out) == capi.KGWAS_ERR_ARG, msg
        assert msg in lib.kgwas_last_error().decode(), lib.kgwas_last_error()
    # no rows: nothing to do, and no device is asked for
    assert lib.kgwas_kmers_ld_proxies(p(leads), 4, None, 0, 1, 64, 500000, 0, None, 0, C.byref(n)) == capi.KGWAS_OK and n.value == 0
    with pytest.raises(kg.KgwasError) as e:
        kg.kmers_ld_proxies(np.zeros((3, 129), np.uint64), np.zeros((3, 129), np.uint64), 8193, "0.8")
    assert e.value.code == capi.KGWAS_ERR_ARG
    with pytest.raises(ValueError):
        kg.kmers_ld_proxies(np.zeros((3, 2), np.uint64), np.zeros((3, 3), np.uint64), 64, "0.8")
    st = capi.ProxyStats()
    for args in ((None, 31, None, b"l", 800000, 5, 0, b"o"), (b"t", 31, None, None, 800000, 5, 0, b"o"), (b"t", 31, None, b"l", 800000, 5, 0, None),
                 (b"t", 31, None, b"l", 0, 5, 0, b"o"), (b"t", 31, None, b"l", 1000001, 5, 0, b"o"), (b"t", 33, None, b"l", 800000, 5, 0, b"o")):
        assert lib.kgwas_proxy_kmers_run(*args, C.byref(st)) == capi.KGWAS_ERR_ARG
