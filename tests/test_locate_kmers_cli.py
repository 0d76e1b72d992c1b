"""locate_kmers without a GPU: the refusals of the tool - each exit 1 with its message, no output file, and for the refusals of the
--kmers file the reference never looked for -, the three formats of --kmers, the usage text, and the argument checks of
kgwas_locate_kmers_bases and kgwas_locate_kmers_run, which come before any device call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kmersgwas_amd as kg
from kmersgwas_amd import capi
from kmersgwas_amd.capi import lib

BIN = os.path.join(os.path.dirname(os.path.abspath(capi.__file__)), "bin", "locate_kmers")
K = 31
GOOD = "ACGT" * 7 + "ACG"
ASSOC9 = "chr\trs\tps\tn_miss\tallele1\tallele0\taf\tl_mle\tp_lrt\n"
ASSOC14 = "chr\trs\tps\tn_miss\tallele1\tallele0\taf\tbeta\tse\tl_remle\tl_mle\tp_wald\tp_lrt\tp_score\n"
CLUMP_HEAD = "rs\tp_lrt\tclump\tlead\tr2\tn1\tn11\n"
PROXY_HEAD = "lead\tkmer\tr2\tphase\tn1\tn11\trow\n"


def run(tmp_path, args, kmers_text=None):
    out = tmp_path / "located.txt"
    cmd = [BIN, "-o", str(out)] + args
    if kmers_text is not None:
        (tmp_path / "kmers.txt").write_text(kmers_text)
        cmd += ["--kmers", str(tmp_path / "kmers.txt"), "--reference", "absent_reference", "--kmers_len", str(K)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert not out.exists() and not os.path.exists(str(out) + ".log.txt"), "an output file was written"
    return r


def refused_before_the_reference(tmp_path, args, kmers_text):
    r = run(tmp_path, args, kmers_text)
    assert "absent_reference" not in r.stderr, "the reference was looked for: " + r.stderr
    return r


def test_missing_options(tmp_path):
    r = run(tmp_path, ["--kmers", "absent_kmers", "--kmers_len", "31"])
    assert r.returncode == 1 and "option --reference is missing" in r.stderr, r.stderr
    r = run(tmp_path, ["--reference", "absent_ref", "--kmers_len", "31"])
    assert r.returncode == 1 and "option --kmers is missing" in r.stderr, r.stderr
    r = run(tmp_path, ["--reference", "absent_ref", "--kmers", "absent_kmers"])
    assert r.returncode == 1 and "option --kmers_len is missing" in r.stderr, r.stderr
    r = run(tmp_path, ["--reference", "absent_ref", "--kmers", "absent_kmers", "--kmers_len", "31", "--x", "1"])
    assert r.returncode == 1 and "Option 'x' does not exist" in r.stderr, r.stderr


def test_missing_files(tmp_path):
    r = run(tmp_path, ["--reference", "absent_ref", "--kmers", "absent_kmers", "--kmers_len", "31"])
    assert r.returncode == 1 and "Couldn't find file: absent_kmers" in r.stderr and "absent_ref" not in r.stderr, r.stderr
    # a good k-mers file gets as far as the reference
    r = run(tmp_path, [], GOOD + "\n\n" + "C" * 31 + "\r\n" + "G" * 30 + "A")
    assert r.returncode == 1 and "Couldn't find file: absent_reference" in r.stderr, r.stderr


@pytest.mark.parametrize("args,msg", [(["--kmers_len", "0"], "kmer length has to be between 1-31"), (["--kmers_len", "32"], "kmer length has to be between 1-31"),
                                      (["--kmers_len", "31", "--mismatches", "2"], "--mismatches is 0 or 1"),
                                      (["--kmers_len", "1", "--mismatches", "1"], "--mismatches is 0 or 1"),
                                      (["--kmers_len", "31", "--mismatches", "x"], "Argument 'x' failed to parse"),
                                      (["--kmers_len", "31", "--max_per_kmer", "-1"], "Argument '-1' failed to parse")])
def test_option_values(tmp_path, args, msg):
    r = run(tmp_path, ["--reference", "absent_ref", "--kmers", "absent_kmers"] + args)
    assert r.returncode == 1 and msg in r.stderr, r.stderr


def test_kmers_file_refusals(tmp_path):
    line9 = "0\t%s\t0\t0\t0\t1\t0.300\t1.000000e+00\t1.5e-9\n"
    cases = [
        (GOOD + "\n" + "C" * 31 + "\n" + GOOD + "\n", "line 3: duplicate k-mer '%s' (the k-mer of line 1)" % GOOD),
        ("A" * 31 + "\n" + "T" * 31 + "\n", "line 2: duplicate k-mer"),  # its reverse complement: the same k-mer
        (GOOD + "\n" + GOOD[:-1] + "\n", "line 2: k-mer '%s' has length 30, not 31" % GOOD[:-1]),
        (GOOD[:-1] + "N\n", "line 1: k-mer '%sN' has a letter other than A, C, G, T" % GOOD[:-1]),
        (GOOD[:-1] + "a\n", "has a letter other than A, C, G, T"),
        (GOOD + "\t1\n", "line 1: 2 fields: a list of k-mers has one k-mer per line"),
        ("\n\n", "no k-mer"),
        ("", "no k-mer"),
        (ASSOC9, "no k-mer"),
        (PROXY_HEAD, "no k-mer"),
        (ASSOC9 + line9 % GOOD + line9 % GOOD, "line 3: duplicate k-mer '%s' (the k-mer of line 2)" % GOOD),
        (ASSOC9 + line9 % GOOD[:-1], "line 2: k-mer '%s' has length 30, not 31" % GOOD[:-1]),
        (ASSOC9 + "0\t" + GOOD + "\t0\n", "line 2: too few fields (3, the header has 9)"),
        (ASSOC14 + "0\n", "line 2: too few fields (1, the header has 14)"),
        (CLUMP_HEAD + GOOD + "\t1e-9\t1\t" + GOOD + "\t1.000000\t4\t4\n" + GOOD[:-1] + "X\t1e-9\t1\t" + GOOD + "\t1.000000\t4\t4\n",
         "line 3: k-mer '%sX' has a letter other than A, C, G, T" % GOOD[:-1]),
        (PROXY_HEAD + GOOD + "\t" + GOOD[:-1] + "\t1.000000\t+\t4\t4\t0\n", "line 2: k-mer '%s' has length 30, not 31" % GOOD[:-1]),
        (PROXY_HEAD + GOOD + "\n", "line 2: too few fields (1, the header has 7)"),
    ]
    for text, msg in cases:
        r = refused_before_the_reference(tmp_path, [], text)
        assert r.returncode == 1 and msg in r.stderr, (msg, r.stderr)


@pytest.mark.parametrize("text", [
    ASSOC9 + "".join("0\t%s\t0\t0\t0\t1\t0.300\t1.000000e+00\t1e-%d\n" % (w, i) for i, w in enumerate((GOOD, "C" * 31))),
    ASSOC14 + "".join("0\t%s\t0\t0\t0\t1\t0.3\t0.1\t0.1\t1.0\t1.0\t1e-3\t1e-%d\t1e-3\n" % (w, i) for i, w in enumerate((GOOD, "C" * 31))),
    CLUMP_HEAD + GOOD + "\t1e-9\t1\t" + GOOD + "\t1.000000\t4\t4\n" + "C" * 31 + "\t1e-9\t1\t" + GOOD + "\t0.900000\t4\t4\n",
    # a proxy_kmers output: its column kmer, distinct values - the second line's k-mer again (here as its reverse complement) is no duplicate
    PROXY_HEAD + "XX\t" + GOOD + "\t1.000000\t+\t4\t4\t0\n" + "XX\t" + "G" * 31 + "\t1.0\t+\t4\t4\t7\n" + "YY\t" + "C" * 31 + "\t1.0\t+\t4\t4\t7\n",
])
def test_the_three_formats_get_as_far_as_the_reference(tmp_path, text):
    r = run(tmp_path, ["--mismatches", "0", "--max_per_kmer", "0"], text)
    assert r.returncode == 1 and "Couldn't find file: absent_reference" in r.stderr, r.stderr


def test_reference_refusals_that_need_no_device(tmp_path):
    (tmp_path / "kmers.txt").write_text(GOOD + "\n")
    for data, msg in ((b"", ": not FASTA"), (b"ACGT\n>x\n", ": not FASTA")):
        ref = tmp_path / "ref.fa"
        ref.write_bytes(data)
        r = run(tmp_path, ["--reference", str(ref), "--kmers", str(tmp_path / "kmers.txt"), "--kmers_len", str(K)])
        assert r.returncode == 1 and str(ref) + msg in r.stderr, r.stderr


def test_usage_text():
    r = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0
    for word in ("--reference", "--kmers", "--kmers_len", "--mismatches", "--max_per_kmer", "--output", "--device", "proxy_kmers output", "clump_kmers output"):
        assert word in r.stdout, word


def test_entry_points_and_argument_checks():
    for s in ("kgwas_locate_kmers_bases", "kgwas_locate_kmers_run"):
        assert s in capi.SYMBOLS and hasattr(lib, s)
    assert [k for k, _ in capi.LocateStats._fields_] == ["contigs", "bases", "windows_tested", "kmers", "hits_found", "hits_kept", "kmers_without_hit",
                                                          "kmers_with_one_hit", "drain_rounds", "parse_ms", "copy_ms", "kernel_ms", "total_ms"]
    assert C.sizeof(capi.LocateStats) == 104 and C.sizeof(capi.LocateRecord) == 16 and kg.LOCATE_RECORD.itemsize == 16
    assert [(k, kg.LOCATE_RECORD.fields[k][1]) for k in kg.LOCATE_RECORD.names] == [("pos", 0), ("kmer", 8), ("strand", 12), ("mismatches", 13), ("offset", 14),
                                                                                     ("pad", 15)]
    bases, rec, n = np.frombuffer(b"ACGTACGTAC", np.uint8), np.zeros(8, kg.LOCATE_RECORD), C.c_uint64(7)
    p = capi.ptr

    def codes(*v):
        return np.asarray(v, np.uint64)

    two = codes(0b000110, 0b111111)  # ACG, TTT
    bad = [
        (None, 10, p(two), 2, 3, 1, p(rec), 8, C.byref(n), "null argument"),
        (p(bases), 10, None, 2, 3, 1, p(rec), 8, C.byref(n), "null argument"),
        (p(bases), 10, p(two), 2, 3, 1, None, 8, C.byref(n), "null argument"),
        (p(bases), 10, p(two), 2, 3, 1, p(rec), 8, None, "null argument"),
        (p(bases), 10, p(two), 2, 0, 0, p(rec), 8, C.byref(n), "k-mers of 1 to 31 bases"),
        (p(bases), 10, p(two), 2, 32, 0, p(rec), 8, C.byref(n), "k-mers of 1 to 31 bases"),
        (p(bases), 10, p(two), 2, 3, 2, p(rec), 8, C.byref(n), "mismatches must be 0 or 1"),
        (p(bases), 10, p(codes(0, 3)), 2, 1, 1, p(rec), 8, C.byref(n), "at least 2 bases"),
        (p(bases), 10, p(two), 0, 3, 1, p(rec), 8, C.byref(n), "0 k-mers"),
        (p(bases), 10, p(two), (1 << 20) + 1, 3, 1, p(rec), 8, C.byref(n), "1048577 k-mers"),
        (p(bases), 10, p(codes(0b000110, 0b1000000)), 2, 3, 1, p(rec), 8, C.byref(n), "code 1 has bits at or above 2 * kmer_len"),
        (p(bases), 10, p(codes(0b000110, 0b011011)), 2, 3, 1, p(rec), 8, C.byref(n), "the queries 0 and 1 are the same k-mer"),  # ACG, CGT
        (p(bases), 10, p(codes(0b000110, 0b000110)), 2, 3, 0, p(rec), 8, C.byref(n), "the queries 0 and 1 are the same k-mer"),
    ]
    for b, nb, c, nk, k, d, r, cap, n_out, msg in bad:
        assert lib.kgwas_locate_kmers_bases(b, nb, 0, c, nk, k, d, 0, r, cap, n_out) == capi.KGWAS_ERR_ARG, msg
        assert msg in lib.kgwas_last_error().decode(), lib.kgwas_last_error()
    with pytest.raises(kg.KgwasError) as e:
        kg.locate_kmers_bases(b"ACGT", kg.kmer_codes(["ACG", "CGT"], 3), 3)
    assert e.value.code == capi.KGWAS_ERR_ARG
    with pytest.raises(TypeError):
        kg.locate_kmers_bases(np.zeros(4, np.int32), two, 3)
    assert kg.kmer_codes(["ACG", "TTT"], 3).tolist() == two.tolist()
    with pytest.raises(ValueError):
        kg.kmer_codes(["ACN"], 3)
    st = capi.LocateStats()
    for args in ((None, b"k", 31, 1, 5, 0, b"o"), (b"r", None, 31, 1, 5, 0, b"o"), (b"r", b"k", 31, 1, 5, 0, None), (b"r", b"k", 0, 0, 5, 0, b"o"),
                 (b"r", b"k", 32, 1, 5, 0, b"o"), (b"r", b"k", 31, 2, 5, 0, b"o"), (b"r", b"k", 1, 1, 5, 0, b"o")):
        assert lib.kgwas_locate_kmers_run(*args, C.byref(st)) == capi.KGWAS_ERR_ARG


def test_the_run_checks_the_kmers_file_before_the_reference(tmp_path):
    kmers = tmp_path / "k.txt"
    kmers.write_text("ACGT\nACGTA\n")
    st = capi.LocateStats()
    rc = lib.kgwas_locate_kmers_run(b"absent_reference", os.fsencode(str(kmers)), 4, 1, 5, 0, os.fsencode(str(tmp_path / "o")), C.byref(st))
    assert rc == capi.KGWAS_ERR_FORMAT and "line 2: k-mer 'ACGTA' has length 5, not 4" in lib.kgwas_last_error().decode()
    kmers.write_text("ACGT\n")
    rc = lib.kgwas_locate_kmers_run(b"absent_reference", os.fsencode(str(kmers)), 4, 1, 5, 0, os.fsencode(str(tmp_path / "o")), C.byref(st))
    assert rc == capi.KGWAS_ERR_IO and lib.kgwas_last_error().decode() == "can't open file: absent_reference"
    rc = lib.kgwas_locate_kmers_run(b"r", b"absent_kmers", 4, 1, 5, 0, os.fsencode(str(tmp_path / "o")), C.byref(st))
    assert rc == capi.KGWAS_ERR_IO and "can't open k-mers file: absent_kmers" in lib.kgwas_last_error().decode()
    assert not (tmp_path / "o").exists()
