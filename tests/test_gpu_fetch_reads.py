"""fetch_reads, the tool, against fetch_np: the kept reads' bytes, the table of kept reads and the log's per-k-mer lines must be the
model's.

The inputs are 300 reads (or pairs) of 60 to 150 bases, some in lower case or with N, with the k-mers planted as spelled and
reverse-complemented; KGWAS_FETCH_PIECE_BYTES and KGWAS_FETCH_RECORDS are set so that the reader thread hands over several pieces
and a piece is drained in rounds."""
import os
import subprocess

import numpy as np
import pytest

import kmersgwas_amd as kg
from kmersgwas_amd import capi

import fetch_np as FN

pytestmark = pytest.mark.gpu
BIN = os.path.join(os.path.dirname(os.path.abspath(capi.__file__)), "bin", "fetch_reads")
K = 31
N_READS = 300
HEAD9 = "chr\trs\tps\tn_miss\tallele1\tallele0\taf\tl_mle\tp_lrt\n"
CLUMP_HEAD = "rs\tp_lrt\tclump\tlead\tr2\tn1\tn11\n"
PROXY_HEAD = "lead\tkmer\tr2\tphase\tn1\tn11\trow\n"
SMALL = {"KGWAS_FETCH_PIECE_BYTES": "4000", "KGWAS_FETCH_RECORDS": "5"}


def _run(cmd, rc=0, env=None, stdin=None):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, **(env or {})), stdin=stdin or subprocess.DEVNULL)
    assert r.returncode == rc, (r.returncode, r.stderr[-2000:])
    return r


def sequences(rng, words, plan):
    """N_READS sequences; plan(i) -> the words' indices planted in read i (odd positions in the list: reverse-complemented)."""
    seqs = []
    for i in range(N_READS):
        s = "".join(rng.choice(list("ACGT"), int(rng.integers(60, 151))))
        for j, w in enumerate(plan(i)):
            at = 2 + 40 * j
            if at + K <= len(s):
                s = s[:at] + (FN.revcomp(words[w]) if j % 2 else words[w]) + s[at + K:]
        if i % 17 == 3:
            s = s.lower()
        if i % 19 == 5:
            s = s[:36] + "N" + s[37:]  # (between two planted k-mers)
        seqs.append(s)
    return seqs


def fastq(names, seqs, eol="\n", final_newline=True):
    text = "".join("@%s%s%s%s+%s%s%s" % (n, eol, s, eol, eol, "I" * len(s), eol) for n, s in zip(names, seqs))
    return (text if final_newline else text[:-len(eol)]).encode()


def fasta(names, seqs, width=50):
    return "".join(">%s\n%s" % (n, "".join(s[i:i + width] + "\n" for i in range(0, len(s), width))) for n, s in zip(names, seqs))[:-1].encode()


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("fetch")
    rng = np.random.default_rng(31)
    words = []
    while len(words) < 12:
        w = "".join(rng.choice(list("ACGT"), K))
        if FN.canonical(w) not in {FN.canonical(x) for x in words}:
            words.append(w)
    # words 0-8 are planted, 9-11 occur nowhere; read i of file 1 holds word i % 9 when i % 4 == 0 (two of them when i % 8 == 0),
    # read i of file 2 when i % 6 == 0: pairs kept through mate 1 only, mate 2 only, both and neither
    s1 = sequences(rng, words, lambda i: [i % 9, (i + 1) % 9, i % 9][:3 if i % 8 == 0 else 1] if i % 4 == 0 else [])
    s2 = sequences(rng, words, lambda i: [(i + 2) % 9] * 2 if i % 6 == 0 else [])
    n1 = ["read%d%s" % (i, ("", " 1:N:0", "\tx")[i % 3]) for i in range(N_READS)]
    n2 = ["read%d/2" % i for i in range(N_READS)]
    files = {"fq1": fastq(n1, s1, final_newline=False), "fq2": fastq(n2, s2), "fa": fasta(n1, s1), "crlf": fastq(n1, s1, "\r\n"),
             "fq2_short": fastq(n2[:-1], s2[:-1])}
    for name, data in files.items():
        (d / name).write_bytes(data)
    return {"dir": d, "words": words, "files": files}


def kmers_file(case, fmt):
    words = case["words"]
    path = case["dir"] / ("kmers_%s.txt" % fmt)
    if fmt == "list":
        text = "".join(w + "\n" for w in words)
    elif fmt == "assoc":
        text = HEAD9 + "".join("0\t%s\t0\t0\t0\t1\t0.300\t1.000000e+00\t%.6e\n" % (w, 10.0 ** -(3 + i % 7)) for i, w in enumerate(words))
    elif fmt == "clump":
        text = CLUMP_HEAD + "".join("%s\t%.6e\t%d\t%s\t1.000000\t4\t4\n" % (w, 10.0 ** -(3 + i % 7), 1 + i // 3, words[i - i % 3]) for i, w in enumerate(words))
    else:  # a proxy_kmers output: the k-mers of its column kmer, some of them under several leads
        lines = ["%s\t%s\t1.000000\t+\t4\t4\t%d\n" % (words[0], w, i) for i, w in enumerate(words)]
        lines += ["%s\t%s\t0.900000\t-\t4\t4\t%d\n" % (words[1], w, i) for i, w in enumerate(words[:4])]
        text = PROXY_HEAD + "".join(lines)
    path.write_text(text)
    return str(path)


def check(case, name, reads, mates=None, fmt="list", extra=(), env=None, ext="fastq", min_hits=1, max_reads=0, stdin=False):
    prefix = str(case["dir"] / name)
    cmd = [BIN, "--reads", "-" if stdin else str(case["dir"] / reads), "--kmers", kmers_file(case, fmt), "--kmers_len", str(K), "-o", prefix] + list(extra)
    if mates:
        cmd += ["--mates", str(case["dir"] / mates)]
    with open(case["dir"] / reads, "rb") as f:
        r = _run(cmd, env=env, stdin=f if stdin else None)
    exp = FN.tool(case["files"][reads], case["words"], min_hits, case["files"][mates] if mates else None, max_reads)
    outs = [prefix + "_1." + ext, prefix + "_2." + ext] if mates else [prefix + "." + ext]
    for path, data in zip(outs, exp["reads"]):
        assert open(path, "rb").read() == data, path
    assert open(prefix + ".reads.tsv", "rb").read() == exp["tsv"]
    log = open(prefix + ".log.txt").read().split("\n")
    assert [l for l in log if l.startswith("kmer\t")] == exp["log"]
    assert "reads_kept\t%d" % len(exp["records"]) in log and "reads\t%d" % (N_READS * (2 if mates else 1)) in log
    assert sorted(os.path.basename(p) for p in outs + [prefix + ".reads.tsv", prefix + ".log.txt"]) == sorted(
        f for f in os.listdir(case["dir"]) if f.startswith(name + ".") or f.startswith(name + "_"))
    assert "[kgwas] fetch_reads: reads=" in r.stderr
    return exp, log


def test_fastq_single(case):
    exp, log = check(case, "single", "fq1", env=SMALL)
    assert len(exp["records"]) == 75 and len(exp["tsv"].split(b"\n")) == 77 and exp["reads"][0].endswith(b"\n")
    assert "kmers_without_read\t3" in log and "drain_rounds\t1" not in log and "drain_rounds\t0" not in log


def test_fastq_pairs(case):
    exp, log = check(case, "pairs", "fq1", mates="fq2", env=SMALL)
    mates_of = {}
    for r in exp["records"]:
        mates_of.setdefault(int(r["read"]) // 2, set()).add(int(r["read"]) % 2)
    assert {frozenset(v) for v in mates_of.values()} == {frozenset({0}), frozenset({1}), frozenset({0, 1})}  # through mate 1, mate 2, both
    assert "pairs_written\t%d" % len(mates_of) in log
    check(case, "min2pairs", "fq1", mates="fq2", extra=["--min_hits", "2"], min_hits=2)


def test_fasta_with_wrapped_lines(case):
    check(case, "wrapped", "fa", ext="fasta", env=SMALL)


def test_crlf_input(case):
    exp, _ = check(case, "crlf", "crlf")
    assert b"\r\n" in exp["reads"][0] and b"\r" not in exp["tsv"]


def test_standard_input(case):
    check(case, "stdin", "fq1", stdin=True)


@pytest.mark.parametrize("fmt", ["assoc", "clump", "proxy"])
def test_the_other_kmers_formats(case, fmt):
    check(case, "fmt_" + fmt, "fq1", fmt=fmt)


def test_max_reads_per_kmer(case):
    exp, log = check(case, "max1", "fq1", extra=["--max_reads_per_kmer", "1"], max_reads=1, env=SMALL)
    assert len(exp["tsv"].split(b"\n")) == 11 and "reads_written\t9" in log and "reads_kept\t75" in log
    check(case, "pairsmax1", "fq1", mates="fq2", extra=["--max_reads_per_kmer", "1"], max_reads=1)


def test_unequal_mate_counts_are_refused(case):
    prefix = str(case["dir"] / "unequal")
    for env in (None, SMALL):
        r = _run([BIN, "--reads", str(case["dir"] / "fq1"), "--mates", str(case["dir"] / "fq2_short"), "--kmers", kmers_file(case, "list"), "--kmers_len", str(K),
                  "-o", prefix], rc=1, env=env)
        assert str(case["dir"] / "fq1") + " has more records than " + str(case["dir"] / "fq2_short") in r.stderr, r.stderr
        assert [f for f in os.listdir(case["dir"]) if f.startswith("unequal")] == []


def test_the_python_mirror(case):
    prefix = str(case["dir"] / "mirror")
    st = kg.fetch_reads(str(case["dir"] / "fq1"), kmers_file(case, "list"), K, prefix, mates_path=str(case["dir"] / "fq2"), min_hits=1, max_reads_per_kmer=2)
    exp = FN.tool(case["files"]["fq1"], case["words"], 1, case["files"]["fq2"], 2)
    assert open(prefix + "_1.fastq", "rb").read() == exp["reads"][0] and open(prefix + "_2.fastq", "rb").read() == exp["reads"][1]
    assert open(prefix + ".reads.tsv", "rb").read() == exp["tsv"]
    written = [int(l.split("\t")[2]) for l in exp["log"]]
    assert written == [2] * 9 + [0] * 3
    assert st["reads"] == 2 * N_READS and st["kmers"] == 12 and st["reads_kept"] == len(exp["records"]) and st["pairs_written"] == sum(written)
    assert st["reads_written"] == len(exp["tsv"].split(b"\n")) - 2 and st["kmers_without_read"] == 3
