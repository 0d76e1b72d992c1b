"""build_kmers_table on the CPU: the restatement (build_table_np.py) pinned by hand-worked cases, its literal form against its closed
form on random inputs, and every guard of the command-line tool - message, exit status and what is left on disk - which all run
before the device is touched."""
import os
import subprocess

import numpy as np
import pytest

import build_table_np as bt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "kmersgwas_amd", "bin", "build_kmers_table")
TERMINATE = "terminate called after throwing an instance of 'std::logic_error'\n  what():  %s\n"
F63, F62 = 1 << 63, 1 << 62


# ---- the restatement, by hand (k = 10: step 210, window 1 = keys 0..210, window 2 = 211..420, last threshold 1 050 210) -------
def test_step_by_hand():
    assert bt.step_of(10) == 210 and bt.step_of(10) * 5001 == 1050210
    assert bt.step_of(31) == ((1 << 62) - 1) // 5000 + 1
    x, w = bt.windows_of([0, 1, 210, 211, 420, 421, 5, 1050210, 1050211, 3], 210)
    assert list(w) == [1, 1, 1, 2, 2, 3, 3, 5001, 5002, 5002]


@pytest.mark.parametrize("all_words,acc,want", [
    ([7], [[7]], [[7, 1]]),                                        # a one-word file on both sides
    ([7], [[8]], [[7, 0]]),
    ([5, 300], [[300], [5]], [[5, 0b10], [300, 0b01]]),            # the last word of a file (held, then handed over once)
    ([5, 5, 9], [[5]], [[5, 1], [5, 0], [9, 0]]),                  # a duplicate in the all-k-mers file: the first insert wins
    ([5, 9], [[5, 5, 9, 9]], [[5, 1], [9, 1]]),                    # a duplicate in an accession's file changes nothing
    ([7, 300], [[300, 7]], [[7, 0], [300, 1]]),                    # a descent moves the accession's 7 into window 2: no match
    ([300, 7], [[300, 7]], [[300, 1], [7, 1]]),                    # a descent in both files: both 7s are in window 2
    ([7], [[5, 100, 7]], [[7, 1]]),                                # a descent back to a key of the same window
    ([7 | F63, 9 | F62 | F63], [[7 | F62], [9]], [[7, 0b01], [9, 0b10]]),  # the flag bits are masked, in both kinds of file
    ([5, 1050211, 6], [[2000000, 5], [5, 2000000]], [[5, 0b10]]),  # a key above step * 5001 ends a file's use
    ([5, 1050210], [[1050210]], [[5, 0], [1050210, 1]]),           # window 5001 itself is used
])
def test_literal_rows_by_hand(all_words, acc, want):
    for fn in (bt.literal_rows, bt.closed_rows):
        got = fn(np.array(all_words, np.uint64), [np.array(a, np.uint64) for a in acc], 10)
        assert got.tolist() == want, fn.__name__


def test_bits_of_accessions_64_and_up():
    acc = [np.array([9 if c in (0, 63, 64, 129) else 8], np.uint64) for c in range(130)]
    for fn in (bt.literal_rows, bt.closed_rows):
        got = fn(np.array([9], np.uint64), acc, 10)
        assert got.tolist() == [[9, 1 | 1 << 63, 1, 2]]


def test_trailing_bytes_and_table_bytes():
    w = bt.words_of_bytes(np.array([7, 9], "<u8").tobytes() + b"\x01\x02\x03")
    assert w.tolist() == [7, 9] and len(bt.words_of_bytes(b"\x01" * 7)) == 0
    rows = bt.literal_rows(w, [np.array([9], np.uint64)], 10)
    assert bt.table_bytes(rows, 1, 10) == (b"\xAA\xBB\xCC\xDD" + (1).to_bytes(8, "little") + (10).to_bytes(4, "little") +
                                           (7).to_bytes(8, "little") + bytes(8) + (9).to_bytes(8, "little") + (1).to_bytes(8, "little"))


def test_empty_file_aborts():
    with pytest.raises(bt.RefAbort) as e:
        bt.SortedFile([], "p")
    assert e.value.what == "sorted kmer file is empty: p"


def test_path_list_tokens():
    assert bt.read_accessions_path_list(b"a x\nb\ty\n\n c  z") == [("a", "x"), ("b", "y"), ("c", "z")]
    assert bt.read_accessions_path_list(b"a x b") == [("a", "x"), ("b", "x")]  # the failed extraction leaves the name as it was
    assert bt.read_accessions_path_list(b"a") == [("a", "")]


def random_case(rng, k):
    step = bt.step_of(k)
    top = min(step * 5001 + 3 * step, bt.MASK)
    style = rng.integers(0, 4)
    span = [top, step * 3, step // 2 + 2, 40][style]  # the whole key space / few windows / one window / many equal keys
    n = int(rng.integers(1, 60))
    pool = rng.integers(0, span, size=n, dtype=np.uint64, endpoint=True)

    def make(m, descents):
        w = np.sort(rng.choice(pool, size=m) if rng.random() < 0.8 else rng.integers(0, span, size=m, dtype=np.uint64, endpoint=True))
        for _ in range(descents):
            i, j = sorted(rng.integers(0, m, size=2))
            w[i:j + 1] = w[i:j + 1][::-1]
        return (w | (rng.integers(0, 4, size=m, dtype=np.uint64) << np.uint64(62))).astype(np.uint64)

    S = int(rng.choice([1, 2, 63, 64, 65, 130]))
    all_words = make(n, int(rng.integers(0, 3)) if rng.random() < 0.5 else 0)
    acc = [make(int(rng.integers(1, 40)), int(rng.integers(0, 3)) if rng.random() < 0.3 else 0) for _ in range(S)]
    return all_words, acc


def test_literal_equals_closed_form_on_random_cases():
    rng = np.random.default_rng(20240917)
    for i in range(120):
        k = int(rng.choice([10, 11, 15, 31]))
        all_words, acc = random_case(rng, k)
        assert bt.literal_rows(all_words, acc, k).tolist() == bt.closed_rows(all_words, acc, k).tolist(), (i, k)


# ---- the tool's guards ---------------------------------------------------------------------------------------------------------
def run_cli(args, cwd):
    return subprocess.run([BIN] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def make_case(tmp_path, S=3, all_bytes=None, acc_bytes=None, drop=None):
    """A list of S accessions acc0.. with one-word files, the all-k-mers file, the output base."""
    paths = []
    for c in range(S):
        p = str(tmp_path / ("acc%d.sorted" % c))
        with open(p, "wb") as f:
            f.write(np.array([5 + c], "<u8").tobytes() if acc_bytes is None or c not in acc_bytes else acc_bytes[c])
        paths.append(p)
    lst = str(tmp_path / "list.txt")
    with open(lst, "w") as f:
        for c, p in enumerate(paths):
            f.write("%s\tname%d\n" % (p, c))
    allk = str(tmp_path / "all.kmers")
    with open(allk, "wb") as f:
        f.write(np.array([5, 6, 7], "<u8").tobytes() if all_bytes is None else all_bytes)
    for c in drop or []:
        os.remove(paths[c])
    return lst, allk, str(tmp_path / "out")


def check_against_restatement(r, lst, k, allk, out):
    want = bt.restate(lst, k, allk)
    assert want["kind"] != "ok"
    if want["kind"] == "exit":
        assert r.returncode == want["status"] and r.stderr.decode() == want["stderr"]
    else:
        assert r.returncode in (-6, 134) and r.stderr.decode() == want["stderr"] + TERMINATE % want["what"]
    assert r.stdout == b""
    for ext in ("names", "table"):
        if want[ext] is None:
            assert not os.path.exists(out + "." + ext)
        else:
            with open(out + "." + ext, "rb") as f:
                assert f.read() == want[ext]


def test_help(tmp_path):
    r = run_cli(["--help"], tmp_path)
    assert r.returncode == 0 and r.stdout == b""
    e = r.stderr.decode()
    assert e.startswith("Build the k-mers table\nUsage:\n  build_kmers_table [OPTION...]")
    for opt in ("-l, --list_kmers_files arg", "-k, --kmers_len arg", "-a, --all_kmers arg", "-o, --output arg", "--help"):
        assert opt in e


@pytest.mark.parametrize("given,missing", [
    ([], "list_kmers_files"), (["-l", "x"], "kmers_len"), (["-l", "x", "-k", "31"], "all_kmers"),
    (["-l", "x", "-k", "31", "-a", "y"], "output"), (["-k", "31", "-a", "y", "-o", "z"], "list_kmers_files")])
def test_missing_option(given, missing, tmp_path):
    r = run_cli(given, tmp_path)
    assert r.returncode == 1 and r.stdout == b""
    assert r.stderr.decode().startswith("%s is a required parameter\nBuild the k-mers table\nUsage:" % missing)
    assert os.listdir(tmp_path) == []


def test_unknown_option_and_bad_number(tmp_path):
    r = run_cli(["--bogus", "1"], tmp_path)
    assert r.returncode == 1 and r.stderr.decode().startswith("error parsing options: Option 'bogus' does not exist\n")
    r = run_cli(["-l", "x", "-k", "ten", "-a", "y", "-o", "z"], tmp_path)
    assert r.returncode == 1 and r.stderr.decode().startswith("error parsing options: Argument 'ten' failed to parse\n")


@pytest.mark.parametrize("drop", ["list", "all", "list+all"])
def test_missing_input_files_in_order(drop, tmp_path):
    lst, allk, out = make_case(tmp_path)
    for part in drop.split("+"):
        os.remove(lst if part == "list" else allk)
    r = run_cli(["-l", lst, "-k", "9", "-a", allk, "-o", out], tmp_path)  # (the files are checked before the length)
    assert r.returncode == 1 and r.stderr.decode() == "Couldn't find file: %s\n" % (lst if "list" in drop else allk)
    check_against_restatement(r, lst, 9, allk, out)


@pytest.mark.parametrize("k", [9, 32, 0])
def test_kmer_length_out_of_range(k, tmp_path):
    lst, allk, out = make_case(tmp_path, drop=[1])  # (the length is checked before the accessions' paths)
    r = run_cli(["-l", lst, "-k", str(k), "-a", allk, "-o", out], tmp_path)
    assert r.returncode == 1 and r.stderr.decode() == "kmer length has to be between 10-31\n"
    check_against_restatement(r, lst, k, allk, out)


@pytest.mark.parametrize("drop,names", [([0], b"name0\n"), ([1], b"name0\nname1\n"), ([2], b"name0\nname1\nname2\n"),
                                        ([1, 2], b"name0\nname1\n")])
def test_missing_accession_path_leaves_partial_names(drop, names, tmp_path):
    lst, allk, out = make_case(tmp_path, drop=drop)
    r = run_cli(["-l", lst, "-k", "31", "-a", allk, "-o", out], tmp_path)
    assert r.returncode == 1 and r.stderr.decode() == "Couldn't find file: %s\n" % str(tmp_path / ("acc%d.sorted" % drop[0]))
    with open(out + ".names", "rb") as f:
        assert f.read() == names
    check_against_restatement(r, lst, 31, allk, out)


@pytest.mark.parametrize("all_bytes", [b"", b"\x01" * 7])
def test_empty_all_kmers_file_aborts(all_bytes, tmp_path):
    lst, allk, out = make_case(tmp_path, all_bytes=all_bytes, acc_bytes={0: b""})  # (the all-k-mers file is opened first)
    r = run_cli(["-l", lst, "-k", "31", "-a", allk, "-o", out], tmp_path)
    assert r.returncode in (-6, 134)
    assert r.stderr.decode() == "Create merger\n" + TERMINATE % ("sorted kmer file is empty: " + allk)
    check_against_restatement(r, lst, 31, allk, out)
    assert not os.path.exists(out + ".table")
    with open(out + ".names", "rb") as f:
        assert f.read() == b"name0\nname1\nname2\n"


@pytest.mark.parametrize("which,body", [(0, b""), (2, b""), (1, b"\x00" * 7)])
def test_empty_accession_file_aborts(which, body, tmp_path):
    lst, allk, out = make_case(tmp_path, acc_bytes={which: body, 2: b""} if which < 2 else {which: body})  # (the first one in list order)
    r = run_cli(["-l", lst, "-k", "10", "-a", allk, "-o", out], tmp_path)
    assert r.returncode in (-6, 134)
    assert r.stderr.decode() == "Create merger\n" + TERMINATE % ("sorted kmer file is empty: " + str(tmp_path / ("acc%d.sorted" % which)))
    check_against_restatement(r, lst, 10, allk, out)
    assert not os.path.exists(out + ".table")
