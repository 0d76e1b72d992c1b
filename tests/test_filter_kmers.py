"""filter_kmers on the CPU: the restatement (filter_kmers_np.py) pinned by hand-worked cases, kgwas_kmer_encode against it, and
every guard of the command-line tool - message, exit status and order - which all run before the device is touched."""
import os
import subprocess

import numpy as np
import pytest

import kmersgwas_amd as kg
from kmersgwas_amd import capi
from oracle import oracle_np as onp
import filter_kmers_np as fk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "kmersgwas_amd", "bin", "filter_kmers")
TERMINATE = "terminate called after throwing an instance of 'std::logic_error'\n  what():  %s\n"


# ---- the restatement, by hand ------------------------------------------------------------------------------------------------
def test_kmer2bits_by_hand():
    assert fk.kmer2bits("ACGT") == 0b00011011  # a palindrome: its own reverse complement
    assert fk.kmer2bits("AAAC") == 1
    assert fk.kmer2bits("GTTT") == 1  # given as the reverse complement of AAAC (code 191): the canonical code
    assert fk.kmer2bits("TTTT") == 0 and fk.kmer2bits("AAAA") == 0
    assert fk.kmer2bits("T") == 0 and fk.kmer2bits("G") == 1
    assert fk.kmer2bits("A" * 32) == 0 and fk.kmer2bits("C" * 32) == int("01" * 32, 2)
    with pytest.raises(fk.RefAbort):
        fk.kmer2bits("acgt")


def test_bits2kmer31_prints_the_low_2k_bits():
    assert fk.bits2kmer31(0b00011011, 4) == "ACGT"
    assert fk.bits2kmer31((0b111 << 8) | 0b00011011, 4) == "ACGT"
    assert fk.bits2kmer31(191, 4) == "GTTT"


@pytest.mark.parametrize("L,keys,want", [
    ([5, 5, 7], [5, 5, 5, 7, 7], [0, 1, 3]),  # duplicates in the list against duplicates in the table
    ([5], [5, 5, 5], [0]),                    # the list used up before the table ends
    ([3, 5], [5, 3], [0]),                    # a descent: set intersection would give both rows
    ([3, 5], [3, 5, 4, 5], [0, 1]),           # after the descent the list is used up
    ([3, 4, 5, 9], [5, 4, 9], [0, 2]),        # 4 was passed over at row 0 and is gone
    ([2, 4, 4], [4, 2, 4, 4], [0, 2]),        # p = 2 after row 0; row 1 (2 < 4) advances; row 2 uses L[2]
    ([1, 2], [], []),
    ([7], [1, 2, 3], []),
])
def test_merge_join_by_hand(L, keys, want):
    assert fk.merge_join(L, keys) == want


def test_lines_bytes_match_the_literal_lines():
    rng = np.random.default_rng(3)
    for S_f, k in ((1, 1), (63, 10), (64, 31), (65, 32), (130, 17)):
        rows = rng.integers(0, 1 << 63, size=(7, 1 + (S_f + 63) // 64), dtype=np.uint64)  # (padding bits set: never printed)
        assert fk.lines_bytes(rows, k, S_f) == "".join(fk.line_of(r, k, S_f) for r in rows).encode()


def test_expected_output_by_hand():
    rows = np.array([[27, 0b101], [27, 0b010], [100, 0b111]], np.uint64)
    emitted, out = fk.expected_output(["x", "y", "z"], 4, rows, [27])
    assert list(emitted) == [0]
    assert out == b"kmer\tx\ty\tz\nACGT\t1\t0\t1\n"


# ---- kgwas_kmer_encode ------------------------------------------------------------------------------------------------------
def test_kmer_encode_matches_the_restatement():
    rng = np.random.default_rng(11)
    for k in range(1, 33):
        for _ in range(40):
            w = "".join("ACGT"[i] for i in rng.integers(0, 4, size=k))
            assert kg.kmer2bits(w) == fk.kmer2bits(w), w
        pal = "".join("ACGT"[i] for i in rng.integers(0, 4, size=k // 2))
        pal = pal + "".join({"A": "T", "C": "G", "G": "C", "T": "A"}[c] for c in reversed(pal))
        if pal:
            assert kg.kmer2bits(pal) == fk.kmer2bits(pal) == fk.kmer2bits(pal[::-1].translate(str.maketrans("ACGT", "TGCA")))


@pytest.mark.parametrize("word,code", [("ACGN", capi.KGWAS_ERR_FORMAT), ("acgt", capi.KGWAS_ERR_FORMAT), ("A C", capi.KGWAS_ERR_FORMAT),
                                       ("", capi.KGWAS_ERR_ARG), ("A" * 33, capi.KGWAS_ERR_ARG)])
def test_kmer_encode_refuses(word, code):
    with pytest.raises(kg.KgwasError) as e:
        kg.kmer2bits(word)
    assert e.value.code == code
    if code == capi.KGWAS_ERR_FORMAT:
        assert e.value.msg == "Ilegal kmer"


# ---- the tool's guards ---------------------------------------------------------------------------------------------------------
def run_cli(args, cwd):
    return subprocess.run([BIN] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def make_case(tmp_path, kmers="ACGT\nAAAC\n", k=4, S_f=5, n_rows=6, body=None):
    base = str(tmp_path / "tab")
    names = ["acc%d" % i for i in range(S_f)]
    W = (S_f + 63) // 64
    keys = np.arange(n_rows, dtype=np.uint64) * np.uint64(3)
    onp.write_table(base, names, k, keys, np.zeros((n_rows, W), np.uint64))
    if body is not None:
        with open(base + ".table", "wb") as f:
            f.write(body)
    lst = str(tmp_path / "list.txt")
    with open(lst, "w") as f:
        f.write(kmers)
    return base, lst, str(tmp_path / "out.tsv")


def header16(prefix=0xDDCCBBAA, n_acc=5, k=4):
    return np.uint32(prefix).tobytes() + np.uint64(n_acc).tobytes() + np.uint32(k).tobytes()


def check_against_restatement(r, base, lst):
    kind, a, err = fk.restate(base, lst)
    if kind == "exit":
        assert r.returncode == a and r.stderr.decode() == err
    elif kind == "abort":
        assert r.returncode in (-6, 134) and r.stderr.decode() == err + TERMINATE % a
    else:  # pragma: no cover
        raise AssertionError("the restatement ran to the end")
    assert r.stdout == b""


def test_help(tmp_path):
    r = run_cli(["--help"], tmp_path)
    assert r.returncode == 0 and r.stdout == b""
    e = r.stderr.decode()
    assert e.startswith("Output the presence/absence patterns of set of k-mers from the k-mers table\nUsage:\n  filter_kmers [OPTION...]")
    for opt in ("-t, --kmers_table arg", "-k, --kmers_file arg", "-o, --output arg", "--help"):
        assert opt in e


@pytest.mark.parametrize("given,missing", [([], "kmers_table"), (["-t", "x"], "kmers_file"), (["-t", "x", "-k", "y"], "output"),
                                           (["-k", "y", "-o", "z"], "kmers_table")])
def test_missing_option(given, missing, tmp_path):
    r = run_cli(given, tmp_path)
    assert r.returncode == 1 and r.stdout == b""
    e = r.stderr.decode()
    assert e.startswith("%s is a required parameter\nOutput the presence/absence patterns" % missing)


def test_unknown_option(tmp_path):
    r = run_cli(["--bogus", "1"], tmp_path)
    assert r.returncode == 1 and r.stderr.decode().startswith("error parsing options: Option 'bogus' does not exist\n")


@pytest.mark.parametrize("drop", ["names", "table", "list", "names+list", "table+list"])
def test_missing_files_in_order(drop, tmp_path):
    base, lst, out = make_case(tmp_path)
    first = None
    for part in ("names", "table", "list"):
        if part in drop.split("+"):
            os.remove(lst if part == "list" else base + "." + part)
            first = first or (lst if part == "list" else base + "." + part)
    r = run_cli(["-t", base, "-k", lst, "-o", out], tmp_path)
    assert r.returncode == 1 and r.stderr.decode() == "Couldn't find file: %s\n" % first
    check_against_restatement(r, base, lst)
    assert not os.path.exists(out)


@pytest.mark.parametrize("kmers,stderr_head,what", [
    ("ACGT\nACG\n", "all kmers should be of the same size: ACG\n", "kmers of different size"),
    ("ACGT ACGTA", "all kmers should be of the same size: ACGTA\n", "kmers of different size"),
    ("ACGT\nACN\n", "all kmers should be of the same size: ACN\n", "kmers of different size"),  # length before characters
    ("ACGN\nACG\n", "", "Ilegal kmer"),  # the first word fails before the second is read
    ("ACGT\nacgt\n", "", "Ilegal kmer"),
    ("ACGT\tAC-T\n", "", "Ilegal kmer"),
])
def test_list_guards_abort(kmers, stderr_head, what, tmp_path):
    base, lst, out = make_case(tmp_path, kmers=kmers)
    r = run_cli(["-t", base, "-k", lst, "-o", out], tmp_path)
    assert r.returncode in (-6, 134)
    assert r.stderr.decode() == stderr_head + TERMINATE % what
    check_against_restatement(r, base, lst)
    assert not os.path.exists(out)


@pytest.mark.parametrize("kmers", ["", "  \n\t\n"])
def test_empty_list(kmers, tmp_path):
    base, lst, out = make_case(tmp_path, kmers=kmers, body=b"")  # the list is checked before the (too small) table
    r = run_cli(["-t", base, "-k", lst, "-o", out], tmp_path)
    assert r.returncode == 1 and r.stderr.decode() == "kmers file is empty\n" and r.stdout == b""
    check_against_restatement(r, base, lst)


@pytest.mark.parametrize("body", [b"", header16(), header16()[:10]])
def test_small_table_exits_1(body, tmp_path):
    base, lst, out = make_case(tmp_path, body=body)
    r = run_cli(["-t", base, "-k", lst, "-o", out], tmp_path)
    assert r.returncode == 1 and r.stderr.decode() == "table file is too small\n"
    check_against_restatement(r, base, lst)
    assert not os.path.exists(out)


@pytest.mark.parametrize("body,what", [
    (header16(prefix=0xDDCCBBAB) + bytes(16), "Incorrect prefix"),
    (header16(prefix=0xDDCCBBAB, n_acc=9, k=7) + bytes(3), "Incorrect prefix"),  # first of the four
    (header16(n_acc=6) + bytes(16), "number of accession in file not as defined in class"),
    (header16(n_acc=6, k=5) + bytes(3), "number of accession in file not as defined in class"),
    (header16(k=5) + bytes(16), "kmer length in table and in list are not the same"),
    (header16(k=5) + bytes(3), "kmer length in table and in list are not the same"),
    (header16() + bytes(24), "size of file not valid"),
    (header16() + bytes(1), "size of file not valid"),
])
def test_table_guards_abort(body, what, tmp_path):
    base, lst, out = make_case(tmp_path, body=body)
    r = run_cli(["-t", base, "-k", lst, "-o", out], tmp_path)
    assert r.returncode in (-6, 134)
    assert r.stderr.decode() == TERMINATE % what
    check_against_restatement(r, base, lst)
    assert not os.path.exists(out)


def test_names_split_on_any_whitespace(tmp_path):
    base, lst, out = make_case(tmp_path, S_f=5)
    with open(base + ".names", "w") as f:
        f.write("acc0 acc1\tacc2\n\nacc3\r\nacc4")  # five words
    with open(base + ".table", "r+b") as f:
        f.write(header16(n_acc=6))
    r = run_cli(["-t", base, "-k", lst, "-o", out], tmp_path)
    assert r.returncode in (-6, 134) and r.stderr.decode() == TERMINATE % "number of accession in file not as defined in class"


def test_unwritable_output(tmp_path):
    base, lst, _ = make_case(tmp_path, n_rows=6)
    out = str(tmp_path / "no_such_dir" / "out.tsv")
    r = run_cli(["-t", base, "-k", lst, "-o", out], tmp_path)
    assert r.returncode == 1 and r.stdout == b""
    assert r.stderr.decode() == "We have 6\ncan't open output file \n"


def test_words_longer_than_32_exit_1(tmp_path):
    base, lst, out = make_case(tmp_path, kmers="A" * 33 + "\n" + "A" * 33 + "\n", k=33)
    r = run_cli(["-t", base, "-k", lst, "-o", out], tmp_path)
    assert r.returncode == 1 and r.stdout == b""
    assert r.stderr.decode() == "filter_kmers: k-mers longer than 32 bases are not supported: %s\n" % ("A" * 33)
    assert not os.path.exists(out)


def test_bad_device_option(tmp_path):
    base, lst, out = make_case(tmp_path)
    r = run_cli(["-t", base, "-k", lst, "-o", out, "--device", "x"], tmp_path)
    assert r.returncode == 1 and r.stderr.decode().startswith("error parsing options: Argument 'x' failed to parse\n")
