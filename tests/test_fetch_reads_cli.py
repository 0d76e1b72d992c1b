"""fetch_reads without a GPU: the refusals of the tool - each exit 1 with its message and no output file, and for the refusals of
the --kmers file the reads never looked for -, the usage text, and the argument checks of kgwas_fetch_reads_bases and
kgwas_fetch_reads_run, which come before any device call."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import kmersgwas_amd as kg
from kmersgwas_amd import capi
from kmersgwas_amd.capi import lib

BIN = os.path.join(os.path.dirname(os.path.abspath(capi.__file__)), "bin", "fetch_reads")
K = 31
GOOD = "ACGT" * 7 + "ACG"
FASTQ = b"@r0\n" + GOOD.encode() + b"\n+\n" + b"I" * 31 + b"\n"
FASTA = b">r0\n" + GOOD.encode() + b"\n"


def run(tmp_path, args, kmers_text=None, prefix=True):
    out = tmp_path / "out" / "kept"
    (tmp_path / "out").mkdir(exist_ok=True)
    cmd = [BIN] + (["-o", str(out)] if prefix else []) + args
    if kmers_text is not None:
        (tmp_path / "kmers.txt").write_text(kmers_text)
        cmd += ["--kmers", str(tmp_path / "kmers.txt"), "--kmers_len", str(K)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, stdin=subprocess.DEVNULL)
    assert glob.glob(str(tmp_path / "out" / "*")) == [], "an output file was written"
    return r


def test_missing_options(tmp_path):
    r = run(tmp_path, ["--kmers", "absent_kmers", "--kmers_len", "31"])
    assert r.returncode == 1 and "option --reads is missing" in r.stderr, r.stderr
    r = run(tmp_path, ["--reads", "absent_reads", "--kmers_len", "31"])
    assert r.returncode == 1 and "option --kmers is missing" in r.stderr, r.stderr
    r = run(tmp_path, ["--reads", "absent_reads", "--kmers", "absent_kmers"])
    assert r.returncode == 1 and "option --kmers_len is missing" in r.stderr, r.stderr
    r = run(tmp_path, ["--reads", "absent_reads", "--kmers", "absent_kmers", "--kmers_len", "31"], prefix=False)
    assert r.returncode == 1 and "option --output is missing" in r.stderr, r.stderr
    r = run(tmp_path, ["--reads", "absent_reads", "--kmers", "absent_kmers", "--kmers_len", "31", "--x", "1"])
    assert r.returncode == 1 and "Option 'x' does not exist" in r.stderr, r.stderr


@pytest.mark.parametrize("args,msg", [(["--kmers_len", "0"], "kmer length has to be between 1-31"), (["--kmers_len", "32"], "kmer length has to be between 1-31"),
                                      (["--kmers_len", "31", "--min_hits", "0"], "--min_hits is at least 1"),
                                      (["--kmers_len", "31", "--min_hits", "x"], "Argument 'x' failed to parse"),
                                      (["--kmers_len", "31", "--max_reads_per_kmer", "-1"], "Argument '-1' failed to parse"),
                                      (["--kmers_len", "31", "--device", "1024"], "--device (at most 1023) out of range"),
                                      (["--kmers_len", "31", "--mates", "-"], "standard input cannot be one of two files")])
def test_option_values(tmp_path, args, msg):
    r = run(tmp_path, ["--reads", "absent_reads", "--kmers", "absent_kmers"] + args)
    assert r.returncode == 1 and msg in r.stderr, r.stderr


def test_a_bad_kmers_file_is_refused_before_the_reads_are_looked_for(tmp_path):
    cases = [
        (GOOD + "\n" + "C" * 31 + "\n" + GOOD + "\n", "line 3: duplicate k-mer '%s' (the k-mer of line 1)" % GOOD),
        ("A" * 31 + "\n" + "T" * 31 + "\n", "line 2: duplicate k-mer"),
        (GOOD + "\n" + GOOD[:-1] + "\n", "line 2: k-mer '%s' has length 30, not 31" % GOOD[:-1]),
        (GOOD[:-1] + "N\n", "has a letter other than A, C, G, T"),
        (GOOD + "\t1\n", "line 1: 2 fields: a list of k-mers has one k-mer per line"),
        ("", "no k-mer"),
        ("lead\tkmer\tr2\tphase\tn1\tn11\trow\n" + GOOD + "\n", "line 2: too few fields (1, the header has 7)"),
    ]
    for text, msg in cases:
        r = run(tmp_path, ["--reads", "absent_reads"], text)
        assert r.returncode == 1 and msg in r.stderr and "absent_reads" not in r.stderr, (msg, r.stderr)


def test_missing_files(tmp_path):
    r = run(tmp_path, ["--reads", "absent_reads", "--kmers", "absent_kmers", "--kmers_len", "31"])
    assert r.returncode == 1 and "Couldn't find file: absent_kmers" in r.stderr and "absent_reads" not in r.stderr, r.stderr
    r = run(tmp_path, ["--reads", "absent_reads"], GOOD + "\n")
    assert r.returncode == 1 and "Couldn't find file: absent_reads" in r.stderr, r.stderr
    (tmp_path / "r.fq").write_bytes(FASTQ)
    r = run(tmp_path, ["--reads", str(tmp_path / "r.fq"), "--mates", "absent_mates"], GOOD + "\n")
    assert r.returncode == 1 and "Couldn't find file: absent_mates" in r.stderr, r.stderr


def test_reads_refusals_that_need_no_device(tmp_path):
    (tmp_path / "r.fq").write_bytes(FASTQ)
    (tmp_path / "m.fa").write_bytes(FASTA)
    (tmp_path / "x.txt").write_bytes(b"ACGT\n")
    r = run(tmp_path, ["--reads", str(tmp_path / "r.fq"), "--mates", str(tmp_path / "m.fa")], GOOD + "\n")
    assert r.returncode == 1 and str(tmp_path / "m.fa") + ": the mates are FASTA, the reads are not" in r.stderr, r.stderr
    r = run(tmp_path, ["--reads", str(tmp_path / "m.fa"), "--mates", str(tmp_path / "r.fq")], GOOD + "\n")
    assert r.returncode == 1 and str(tmp_path / "r.fq") + ": the mates are FASTQ, the reads are not" in r.stderr, r.stderr
    r = run(tmp_path, ["--reads", str(tmp_path / "x.txt")], GOOD + "\n")
    assert r.returncode == 1 and str(tmp_path / "x.txt") + ": neither FASTA nor FASTQ" in r.stderr, r.stderr


def test_usage_text():
    r = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0
    for word in ("--reads", "--mates", "--kmers", "--kmers_len", "--min_hits", "--max_reads_per_kmer", "--output", "--device", "standard input",
                 "proxy_kmers output", "clump_kmers output"):
        assert word in r.stdout, word


def test_entry_points_and_argument_checks(tmp_path):
    for s in ("kgwas_fetch_reads_bases", "kgwas_fetch_reads_run"):
        assert s in capi.SYMBOLS and hasattr(lib, s)
    assert [k for k, _ in capi.FetchStats._fields_] == ["reads", "bases", "windows_tested", "kmers", "windows_hit", "reads_kept", "reads_written",
                                                         "pairs_written", "kmers_without_read", "drain_rounds", "parse_ms", "copy_ms", "kernel_ms", "total_ms"]
    assert C.sizeof(capi.FetchStats) == 112 and C.sizeof(capi.FetchRecord) == 24 and kg.FETCH_RECORD.itemsize == 24
    assert [(k, kg.FETCH_RECORD.fields[k][1]) for k in kg.FETCH_RECORD.names] == [("read", 0), ("n_hits", 8), ("first_pos", 12), ("kmer", 16), ("strand", 20),
                                                                                   ("pad", 21)]
    bases, rec, n, win = np.frombuffer(b"ACGTACGTA\n", np.uint8), np.zeros(8, kg.FETCH_RECORD), C.c_uint64(7), np.zeros(2, np.uint64)
    p = capi.ptr

    def codes(*v):
        return np.asarray(v, np.uint64)

    two = codes(0b000110, 0b111111)  # ACG, TTT
    bad = [
        (None, 10, p(two), 2, 3, 1, p(rec), 8, C.byref(n), "null argument"),
        (p(bases), 10, None, 2, 3, 1, p(rec), 8, C.byref(n), "null argument"),
        (p(bases), 10, p(two), 2, 3, 1, None, 8, C.byref(n), "null argument"),
        (p(bases), 10, p(two), 2, 3, 1, p(rec), 8, None, "null argument"),
        (p(bases), 10, p(two), 2, 0, 1, p(rec), 8, C.byref(n), "k-mers of 1 to 31 bases"),
        (p(bases), 10, p(two), 2, 32, 1, p(rec), 8, C.byref(n), "k-mers of 1 to 31 bases"),
        (p(bases), 10, p(two), 2, 3, 0, p(rec), 8, C.byref(n), "min_hits must be at least 1"),
        (p(bases), 10, p(two), 0, 3, 1, p(rec), 8, C.byref(n), "0 k-mers"),
        (p(bases), 10, p(two), (1 << 20) + 1, 3, 1, p(rec), 8, C.byref(n), "1048577 k-mers"),
        (p(bases), 10, p(codes(0b000110, 0b1000000)), 2, 3, 1, p(rec), 8, C.byref(n), "code 1 has bits at or above 2 * kmer_len"),
        (p(bases), 10, p(codes(0b000110, 0b011011)), 2, 3, 1, p(rec), 8, C.byref(n), "the queries 0 and 1 are the same k-mer"),  # ACG, CGT
        (p(bases), 10, p(codes(0b000110, 0b000110)), 2, 3, 1, p(rec), 8, C.byref(n), "the queries 0 and 1 are the same k-mer"),
    ]
    for b, nb, c, nk, k, m, r, cap, n_out, msg in bad:
        for w in (p(win), None):
            assert lib.kgwas_fetch_reads_bases(b, nb, c, nk, k, m, 0, r, cap, n_out, w) == capi.KGWAS_ERR_ARG, msg
            assert msg in lib.kgwas_last_error().decode(), lib.kgwas_last_error()
    with pytest.raises(kg.KgwasError) as e:
        kg.fetch_reads_bases(b"ACGT\n", kg.kmer_codes(["ACG", "CGT"], 3), 3)
    assert e.value.code == capi.KGWAS_ERR_ARG
    with pytest.raises(TypeError):
        kg.fetch_reads_bases(np.zeros(4, np.int32), two, 3)
    with pytest.raises(TypeError):
        kg.fetch_reads_bases("ACGT", two, 3)
    st = capi.FetchStats()
    o = os.fsencode(str(tmp_path / "o"))
    for args in ((None, None, b"k", 31, 1, 0, 0, o), (b"r", None, None, 31, 1, 0, 0, o), (b"r", None, b"k", 31, 1, 0, 0, None), (b"r", None, b"k", 0, 1, 0, 0, o),
                 (b"r", None, b"k", 32, 1, 0, 0, o), (b"r", b"m", b"k", 31, 0, 0, 0, o)):
        assert lib.kgwas_fetch_reads_run(*args, C.byref(st)) == capi.KGWAS_ERR_ARG
    assert glob.glob(str(tmp_path / "o*")) == []


def test_the_run_checks_the_kmers_file_before_the_reads(tmp_path):
    kmers = tmp_path / "k.txt"
    kmers.write_text("ACGT\nACGTA\n")
    st = capi.FetchStats()
    o = os.fsencode(str(tmp_path / "o"))
    rc = lib.kgwas_fetch_reads_run(b"absent_reads", None, os.fsencode(str(kmers)), 4, 1, 0, 0, o, C.byref(st))
    assert rc == capi.KGWAS_ERR_FORMAT and "line 2: k-mer 'ACGTA' has length 5, not 4" in lib.kgwas_last_error().decode()
    kmers.write_text("ACGT\n")
    rc = lib.kgwas_fetch_reads_run(b"absent_reads", None, os.fsencode(str(kmers)), 4, 1, 0, 0, o, C.byref(st))
    assert rc == capi.KGWAS_ERR_IO and lib.kgwas_last_error().decode() == "can't open file: absent_reads"
    rc = lib.kgwas_fetch_reads_run(b"r", None, b"absent_kmers", 4, 1, 0, 0, o, C.byref(st))
    assert rc == capi.KGWAS_ERR_IO and "can't open k-mers file: absent_kmers" in lib.kgwas_last_error().decode()
    assert glob.glob(str(tmp_path / "o*")) == []
