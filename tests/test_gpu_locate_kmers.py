"""locate_kmers, the tool, against locate_np: the output's bytes and the log's per-k-mer lines must be the model's.

The reference is some 60 kb in 5 contigs - one shorter than k, one all N, some with CRLF lines, lower case in places, a repeat, no
final newline. The k-mers are windows of it as they stand, with one base changed (the alternative allele), reverse-complemented,
and some that occur nowhere; they are given in each of the three formats of --kmers. KGWAS_LOCATE_PIECE_BYTES and
KGWAS_LOCATE_RECORDS are set so that the reader thread hands over several pieces and a piece is drained in rounds."""
import os
import subprocess

import numpy as np
import pytest

from kmersgwas_amd import capi

import locate_np as LN

pytestmark = pytest.mark.gpu
BIN = os.path.join(os.path.dirname(os.path.abspath(capi.__file__)), "bin", "locate_kmers")
K = 31
HEAD9 = "chr\trs\tps\tn_miss\tallele1\tallele0\taf\tl_mle\tp_lrt\n"
CLUMP_HEAD = "rs\tp_lrt\tclump\tlead\tr2\tn1\tn11\n"
PROXY_HEAD = "lead\tkmer\tr2\tphase\tn1\tn11\trow\n"
REPEATS = 12


def _run(cmd, rc=0, env=None):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, **(env or {})))
    assert r.returncode == rc, (r.returncode, r.stderr[-2000:])
    return r


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("locate")
    rng = np.random.default_rng(31)
    seq = lambda n: "".join(rng.choice(list("ACGT"), n))
    repeat = seq(40)
    chr1, chr2, chr5 = seq(25000), seq(20000), seq(15000)
    for i in range(REPEATS):  # a repeat: its k-mers occur 12 times in chr5
        at = 500 + 1100 * i
        chr5 = chr5[:at] + repeat + chr5[at + 40:]
    chr1 = chr1[:3000] + chr1[3000:3400].lower() + chr1[3400:9000] + "N" * 50 + chr1[9050:]
    contigs = [("chr1 the first", chr1, 60, "\r\n"), ("chr2", chr2, 70, "\n"), ("tiny", "ACGTACGT", 60, "\n"), ("gap\tall N", "N" * 3000, 100, "\r\n"),
               ("chr5", chr5, 61, "\n")]
    fasta = ""
    for name, s, width, eol in contigs:
        fasta += ">" + name + eol + "".join(s[i:i + width] + eol for i in range(0, len(s), width))
    fasta = fasta[:-1]  # no final newline
    ref = d / "ref.fa"
    ref.write_bytes(fasta.encode())
    model_contigs = LN.read_fasta(fasta.encode())
    assert [n for n, _ in model_contigs] == ["chr1", "chr2", "tiny", "gap", "chr5"] and model_contigs[0][1].decode() == chr1

    def change(w, j):
        return w[:j] + rng.choice([c for c in "ACGT" if c != w[j]]) + w[j + 1:]

    words = [repeat[3:3 + K]]  # the repeated k-mer
    for no, (s, p) in enumerate([(chr1, 100), (chr1, 3010), (chr1, 6990), (chr1, 13990), (chr2, 0), (chr2, 20000 - K), (chr2, 6980), (chr5, 15000 - K),
                                 (chr5, 9000), (chr1, 24000), (chr2, 10000), (chr5, 2000), (chr1, 20985), (chr2, 13980), (chr5, 3)]):
        w = s[p:p + K].upper()
        assert len(w) == K and "N" not in w
        w = (w, change(w, int(rng.integers(0, K))), LN.revcomp(w), LN.revcomp(change(w, int(rng.integers(0, K)))), change(w, 0), change(w, K - 1))[no % 6]
        words.append(w)
    words += [seq(K) for _ in range(5)]  # nowhere in the reference
    assert len({LN.canonical(w) for w in words}) == len(words)
    return {"dir": d, "ref": str(ref), "fasta": fasta.encode(), "words": words, "bases": sum(len(s) for _, s, _, _ in contigs)}


def kmers_file(case, fmt, words=None):
    words = case["words"] if words is None else words
    path = case["dir"] / ("kmers_%s_%d.txt" % (fmt, len(words)))
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
    return str(path), text


def locate_kmers(case, kmers, name, extra, env=None):
    out = str(case["dir"] / name)
    r = _run([BIN, "--reference", case["ref"], "--kmers", kmers, "--kmers_len", str(K), "-o", out] + extra, env=env)
    return out, r


def log_of(path):
    text = open(path + ".log.txt").read()
    per_kmer = "".join(l + "\n" for l in text.split("\n") if l.startswith("kmer\t")).encode()
    return per_kmer, dict(l.split("\t", 1) for l in text.split("\n") if "\t" in l and not l.startswith("kmer\t"))


@pytest.mark.parametrize("fmt", ["list", "assoc", "clump", "proxy"])
@pytest.mark.parametrize("d", [0, 1])
def test_formats_and_mismatches(case, fmt, d):
    path, text = kmers_file(case, fmt)
    exp_out, exp_log, counts, windows = LN.run(case["fasta"], text, K, d)
    out, r = locate_kmers(case, path, "out_%s_%d.txt" % (fmt, d), ["--mismatches", str(d)], env={"KGWAS_LOCATE_PIECE_BYTES": "7000", "KGWAS_LOCATE_RECORDS": "5"})
    assert open(out, "rb").read() == exp_out
    per_kmer, log = log_of(out)
    found = sum(f for _, f in counts)
    assert per_kmer == exp_log
    assert log["contigs"] == "5" and log["bases"] == str(case["bases"]) and log["windows_tested"] == str(windows) and log["kmers"] == str(len(counts))
    assert log["hits_found"] == log["hits_kept"] == str(found) and log["mismatches"] == str(d) and log["max_per_kmer"] == "100"
    assert log["kmers_without_hit"] == str(sum(f == 0 for _, f in counts)) and log["kmers_with_one_hit"] == str(sum(f == 1 for _, f in counts))
    assert int(log["drain_rounds"]) >= -(-found // 5) and log["reference"] == case["ref"] and log["kmers_file"] == path
    assert "[kgwas] locate_kmers: " in r.stderr and " hits_found=%d " % found in r.stderr
    # (stated on their own) the header's last column, the repeat, and what d = 1 adds
    head = open(out).readline().rstrip("\n").split("\t")
    assert (head[-1] == "p_lrt") == (fmt in ("assoc", "clump"))
    assert counts[0] == (REPEATS, REPEATS)
    lines = [l.split("\t") for l in exp_out.decode().split("\n")[1:-1]]
    assert {l[1] for l in lines} <= {"chr1", "chr2", "chr5"}
    if d == 0:
        assert all(l[4:8] == ["0", "0", ".", "."] for l in lines) and found == len(lines)
    else:
        assert any(l[4] == "1" and l[3] == "-" for l in lines) and any(l[4] == "1" and l[3] == "+" and l[6] != l[7] for l in lines)
        assert sum(f == 0 for _, f in counts) == 5  # only the k-mers from nowhere


def test_default_piece_and_buffer(case):
    path, text = kmers_file(case, "list")
    exp_out, exp_log, _, _ = LN.run(case["fasta"], text, K, 1)
    out, _ = locate_kmers(case, path, "default.txt", [])  # --mismatches 1 is the default
    assert open(out, "rb").read() == exp_out and log_of(out)[0] == exp_log and log_of(out)[1]["drain_rounds"] == "1"


def test_max_per_kmer(case):
    path, text = kmers_file(case, "assoc")
    exp_out, exp_log, counts, _ = LN.run(case["fasta"], text, K, 1, max_per_kmer=5)
    assert counts[0] == (5, REPEATS)
    out, _ = locate_kmers(case, path, "max5.txt", ["--max_per_kmer", "5"], env={"KGWAS_LOCATE_PIECE_BYTES": "9999", "KGWAS_LOCATE_RECORDS": "3"})
    assert open(out, "rb").read() == exp_out
    per_kmer, log = log_of(out)
    assert per_kmer == exp_log and log["max_per_kmer"] == "5"
    assert log["hits_kept"] == str(sum(k for k, _ in counts)) and log["hits_found"] == str(sum(f for _, f in counts))
    # 0: no limit
    exp_out, exp_log, counts, _ = LN.run(case["fasta"], text, K, 1, max_per_kmer=0)
    out, _ = locate_kmers(case, path, "max0.txt", ["--max_per_kmer", "0"])
    assert open(out, "rb").read() == exp_out and counts[0] == (REPEATS, REPEATS)


def test_no_kmer_hits(case):
    path, text = kmers_file(case, "list", case["words"][-5:])
    exp_out, exp_log, counts, _ = LN.run(case["fasta"], text, K, 1)
    assert counts == [(0, 0)] * 5
    out, _ = locate_kmers(case, path, "none.txt", [], env={"KGWAS_LOCATE_PIECE_BYTES": "7000"})
    assert open(out, "rb").read() == exp_out == b"kmer\tcontig\tpos\tstrand\tmismatches\toffset\tref\talt\n"
    per_kmer, log = log_of(out)
    assert per_kmer == exp_log and log["hits_found"] == "0" and log["kmers_without_hit"] == "5" and log["drain_rounds"] == "0"


def test_a_reference_refused_in_the_reader_thread(case):
    """a contig named twice far into the file: the refusal comes from the reader thread, and no output is left"""
    ref = case["dir"] / "twice.fa"
    ref.write_bytes(case["fasta"] + b"\n>chr2 again\nACGT\n")
    path, _ = kmers_file(case, "list")
    out = str(case["dir"] / "twice.txt")
    r = _run([BIN, "--reference", str(ref), "--kmers", path, "--kmers_len", str(K), "-o", out], rc=1, env={"KGWAS_LOCATE_PIECE_BYTES": "7000"})
    assert "the contig 'chr2' is given twice" in r.stderr and not os.path.exists(out) and not os.path.exists(out + ".log.txt")
