"""list_kmers_found_in_multiple_samples on the CPU: the restatement (list_kmers_np.py) pinned by hand-worked cases whose expected bytes
are written out here, its literal form against its closed form on random inputs, the strand rule at its edges, and every guard of the
command-line tool - message, exit status and what is left on disk - which all run before the device is touched."""
import os
import subprocess

import numpy as np
import pytest

import list_kmers_np as lk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = "list_kmers_found_in_multiple_samples"
BIN = os.path.join(ROOT, "kmersgwas_amd", "bin", TOOL)
TERMINATE = "terminate called after throwing an instance of 'std::logic_error'\n  what():  %s\n"
U = np.uint64
F1, F2, F3 = 1 << 62, 2 << 62, 3 << 62
NAN = float("nan")


def u(words):
    return np.array(words, U)


# ---- the restatement, by hand (k = 10: step 210, window 1 = keys 0..210, window 2 = 211..420, last threshold 1 050 210) -------
# two files, mac 2, p 0.5: key 5 passes (one file per strand), 9 is seen in non-canonical form only (fails on the canonical
# side), 12 in canonical form only (fails on the non-canonical side), 300 is in one file (below MAC)
HAND = [u([5 | F1, 9 | F2, 12 | F1, 300 | F3]), u([5 | F2, 9 | F2, 12 | F1])]
HAND_FILES = {
    "": (5).to_bytes(8, "little"),
    ".no_pass_kmers": b"kmer\tcount_all\tcanonical\tnon-canonical\tboth\nAAAAAAAAGC\t2\t0\t2\t0\nAAAAAAAATA\t2\t2\t0\t0\n",
    ".shareness": b"kmer appearance\tcount\n0\t0\n1\t0\n2\t1\n",
    ".stats.only_canonical": b"0\t0\t0\n1\t0\t0\n1\t1\t1\n",
    ".stats.only_non_canonical": b"0\t0\t0\n1\t0\t0\n1\t1\t1\n",
    ".stats.both": b"0\t0\t0\n0\t1\t0\n3\t0\t0\n",
}


@pytest.mark.parametrize("fn", [lk.literal, lk.closed])
def test_by_hand_two_files(fn):
    res = fn(HAND, 10, 2, 0.5)
    assert lk.files_of(res, 10) == HAND_FILES
    assert lk.counts_of(res) == (1, 2, 1)
    assert lk.summary_of(res) == "kmers lower than MAC:\t1\npassed kmers:\t1\npassed MAC bot not pass strand filter:\t2\n"


@pytest.mark.parametrize("fn", [lk.literal, lk.closed])
def test_by_hand_windows_duplicates_and_descents(fn):
    # a key twice in one file counts twice (and with flag 3 it passes on its own at mac 2)
    res = fn([u([7 | F3, 7 | F3]), u([8 | F1])], 10, 2, 0.5)
    assert res["passed"] == [7] and res["no_pass"] == [] and res["low"] == 1 and int(res["both"][2][2]) == 1
    # a descent moves file 0's 7 into window 2: (1, 7) and (2, 7) are two items of one word each; window 2 is written after window 1
    res = fn([u([300 | F3, 7 | F3]), u([7 | F3, 300 | F3])], 10, 1, 0.0)
    assert res["passed"] == [7, 7, 300] and int(res["shareness"][1]) == 2 and int(res["shareness"][2]) == 1
    # keys above step * 5001 = 1 050 210 end a file's use: the 5 behind one is never counted, flag 0 there is no error
    res = fn([u([5 | F3, 1050210 | F3, 1050211, 5 | F3]), u([2000000, 6 | F3])], 10, 0, 0.0)
    assert res["passed"] == [5, 1050210]


def test_undefined_behaviour_inputs_raise():
    for fn in (lk.literal, lk.closed):
        with pytest.raises(lk.RefUB) as e:
            fn([u([5 | F1]), u([6 | F1, 9])], 10, 1, 0.2)
        assert e.value.kind == "flag0" and e.value.file == 1
        with pytest.raises(lk.RefUB) as e:
            fn([u([5 | F1, 5 | F1, 5 | F2]), u([4 | F1])], 10, 1, 0.2)  # 5 is counted three times in two files
        assert e.value.kind == "above_n" and e.value.key == 5
        fn([u([5 | F1, 5 | F1]), u([4 | F1])], 10, 1, 0.2)  # twice in two files is within the matrices


# ---- the strand rule at its edges: one key in `n` files, `c` of them with flag 1, `m` with flag 2, the rest with flag 3 ---------
def one_key(n, c, m):
    return [u([77 | (F1 if i < c else F2 if i < c + m else F3)]) for i in range(n)]


@pytest.mark.parametrize("p,n,c,m,want", [
    (0.2, 5, 4, 1, True), (0.2, 5, 5, 0, False),     # 0.2 * 5 is 1.0 in double: one file on the weaker side is enough
    (0.2, 6, 5, 1, False), (0.2, 6, 4, 2, True),     # 0.2 * 6 is 1.2000000000000002: ceil 2
    (0.5, 3, 1, 2, False), (0.5, 3, 1, 1, True),     # ceil(1.5) = 2 on both sides needs a file with both forms
    (0.5, 5, 2, 3, False), (0.5, 5, 2, 2, True), (0.5, 7, 3, 3, True), (0.5, 7, 4, 3, False),
    (0.0, 4, 4, 0, True), (0.0, 1, 0, 1, True),      # ceil(0) = 0
    (1.0, 3, 0, 0, True), (1.0, 3, 1, 0, False), (1.0, 3, 0, 1, False),  # every file must hold both forms
    (1.5, 3, 0, 0, False), (1.5, 1, 0, 0, False),    # ceil(1.5 n) > n
    (-1.0, 3, 3, 0, True), (-1.0, 2, 0, 2, True),    # a negative bound
    (NAN, 3, 0, 0, False), (NAN, 1, 1, 0, False),    # NaN compares false
])
def test_strand_rule_edges(p, n, c, m, want):
    for fn in (lk.literal, lk.closed):
        res = fn(one_key(n, c, m), 10, 1, p)
        assert (res["passed"] == [77]) == want and (res["no_pass"] == [(77, n, c, m, n - c - m)]) == (not want)
        assert int(res["shareness"][n]) == int(want) and res["low"] == 0
    assert lk.passes(n, c, m, n - c - m, n + 1, p) is None  # below MAC whatever p


def random_case(rng, k, flags0=False):
    """Files with duplicates inside a file, descents, keys above the last threshold and all three flags."""
    step = lk.step_of(k)
    top = min(step * 5001 + 3 * step, lk.MASK)
    span = [top, step * 3, step // 2 + 2, 40][int(rng.integers(0, 4))]  # the whole key space / few windows / one window / many equal keys
    pool = rng.integers(0, span, size=int(rng.integers(1, 60)), dtype=U, endpoint=True)
    N = int(rng.choice([1, 2, 3, 63, 64, 65, 130]))
    acc = []
    for _ in range(N):
        m = int(rng.integers(1, 40))
        w = np.sort(rng.choice(pool, size=m) if rng.random() < 0.8 else rng.integers(0, span, size=m, dtype=U, endpoint=True))
        if rng.random() < 0.7:
            w = np.unique(w)  # (a duplicate inside a file can push a count above N: some files keep theirs)
        for _ in range(int(rng.integers(0, 3)) if rng.random() < 0.3 else 0):
            i, j = sorted(rng.integers(0, len(w), size=2))
            w[i:j + 1] = w[i:j + 1][::-1]
        acc.append((w | (rng.integers(0 if flags0 else 1, 4, size=len(w), dtype=U) << U(62))).astype(U))
    return acc


def outcome(fn, *args):
    try:
        return fn(*args)
    except lk.RefUB as e:
        return e.kind


def test_literal_equals_closed_form_on_random_cases():
    rng = np.random.default_rng(20241017)
    kinds = set()
    for i in range(70):
        k = int(rng.choice([10, 11, 15, 31]))
        acc = random_case(rng, k, flags0=i % 10 == 9)
        mac = int(rng.choice([0, 1, 2, 5, len(acc), len(acc) + 1]))
        p = float(rng.choice([0.0, 0.2, 0.5, 1.0, 1.5, -1.0, NAN]))
        a, b = outcome(lk.literal, acc, k, mac, p), outcome(lk.closed, acc, k, mac, p)
        if isinstance(a, str) or isinstance(b, str):
            assert isinstance(a, str) and isinstance(b, str), (i, a if isinstance(a, str) else b)
            kinds.add(a)
            continue
        assert lk.same(a, b), (i, k, mac, p)
        kinds.add("ok")
    assert "ok" in kinds and "above_n" in kinds


# ---- the tool's guards ---------------------------------------------------------------------------------------------------------
def run_cli(args, cwd):
    return subprocess.run([BIN] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def make_case(tmp_path, S=3, acc_bytes=None, drop=None, repeat=1):
    paths = []
    for c in range(S):
        p = str(tmp_path / ("acc%d.sorted" % c))
        with open(p, "wb") as f:
            f.write(np.array([(5 + c) | F3], "<u8").tobytes() if acc_bytes is None or c not in acc_bytes else acc_bytes[c])
        paths.append(p)
    lst = str(tmp_path / "list.txt")
    with open(lst, "w") as f:
        f.write("".join("%s\tname%d\n" % (p, c) for c, p in enumerate(paths)) * repeat)
    for c in drop or []:
        os.remove(paths[c])
    return lst, str(tmp_path / "out")


def outputs(out):
    return sorted(e for e in lk.EXTS if os.path.exists(out + e))


def check_against_restatement(r, lst, k, mac, p, out):
    want = lk.restate(lst, k, mac, p)
    assert want["kind"] != "ok"
    if want["kind"] == "exit":
        assert r.returncode == want["status"] and r.stderr.decode() == want["stderr"]
    else:
        assert r.returncode in (-6, 134) and r.stderr.decode() == TERMINATE % want["what"]
    assert r.stdout == b"" and outputs(out) == []


def test_help(tmp_path):
    r = run_cli(["--help"], tmp_path)
    assert r.returncode == 0 and r.stdout == b""
    e = r.stderr.decode()
    assert e.startswith("Combines and filters information from all samples k-mers lists to one sorted k-mers list\nUsage:\n  " + TOOL + " [OPTION...]")
    for opt in ("-l, --list_kmers_files arg", "-k, --kmers_len arg", "--mac arg", "-p, --min_strand_percent arg", "-o, --output arg", "--device arg", "--help"):
        assert opt in e


FULL = ["-l", "x", "--mac", "5", "-k", "31", "-p", "0.2", "-o", "z"]


@pytest.mark.parametrize("given,missing", [
    ([], "list_kmers_files"), (FULL[:2], "mac"), (FULL[:4], "kmers_len"), (FULL[:6], "min_strand_percent"), (FULL[:8], "output"),
    (FULL[2:], "list_kmers_files"), (FULL[:2] + FULL[4:], "mac"), (["-k", "31", "-o", "z"], "list_kmers_files")])
def test_missing_option(given, missing, tmp_path):
    r = run_cli(given, tmp_path)
    assert r.returncode == 1 and r.stdout == b""
    assert r.stderr.decode().startswith("%s is a required parameter\nCombines and filters information" % missing)
    assert os.listdir(tmp_path) == []


def test_unknown_option_and_bad_numbers(tmp_path):
    r = run_cli(["--bogus", "1"], tmp_path)
    assert r.returncode == 1 and r.stderr.decode().startswith("error parsing options: Option 'bogus' does not exist\n")
    for i, bad in ((3, "five"), (3, "-5"), (5, "ten"), (7, "a fifth")):
        r = run_cli(FULL[:i] + [bad] + FULL[i + 1:], tmp_path)
        assert r.returncode == 1 and r.stderr.decode().startswith("error parsing options: Argument '%s' failed to parse\n" % bad)
    assert os.listdir(tmp_path) == []


def test_missing_list_file_is_checked_before_the_length(tmp_path):
    lst, out = make_case(tmp_path)
    os.remove(lst)
    r = run_cli(["-l", lst, "--mac", "1", "-k", "9", "-p", "0.2", "-o", out], tmp_path)
    assert r.returncode == 1 and r.stderr.decode() == "Couldn't find file: %s\n" % lst
    check_against_restatement(r, lst, 9, 1, 0.2, out)


@pytest.mark.parametrize("k", [9, 32, 0])
def test_kmer_length_out_of_range(k, tmp_path):
    lst, out = make_case(tmp_path, drop=[1])  # (the length is checked before the accessions' paths)
    r = run_cli(["-l", lst, "--mac", "1", "-k", str(k), "-p", "0.2", "-o", out], tmp_path)
    assert r.returncode == 1 and r.stderr.decode() == "kmer length has to be between 10-31\n"
    check_against_restatement(r, lst, k, 1, 0.2, out)


@pytest.mark.parametrize("drop", [[0], [1], [2], [1, 2]])
def test_missing_accession_path(drop, tmp_path):
    lst, out = make_case(tmp_path, drop=drop)
    r = run_cli(["-l", lst, "--mac", "1", "-k", "31", "-p", "0.2", "-o", out], tmp_path)
    assert r.returncode == 1 and r.stderr.decode() == "Couldn't find file: %s\n" % str(tmp_path / ("acc%d.sorted" % drop[0]))
    check_against_restatement(r, lst, 31, 1, 0.2, out)


@pytest.mark.parametrize("empty,drop,first", [([0], [], "empty0"), ([2], [], "empty2"), ([1, 2], [], "empty1"),
                                               ([0], [1], "empty0"),    # an empty file before a missing one: the abort comes first
                                               ([2], [1], "missing1")])  # a missing file before an empty one
def test_empty_files_abort_as_they_are_opened(empty, drop, first, tmp_path):
    lst, out = make_case(tmp_path, acc_bytes={c: b"\x00" * (7 if c == 1 else 0) for c in empty}, drop=drop)
    r = run_cli(["-l", lst, "--mac", "1", "-k", "10", "-p", "0.2", "-o", out], tmp_path)
    path = str(tmp_path / ("acc%s.sorted" % first[-1]))
    if first.startswith("empty"):
        assert r.returncode in (-6, 134) and r.stderr.decode() == TERMINATE % ("sorted kmer file is empty: " + path)
    else:
        assert r.returncode == 1 and r.stderr.decode() == "Couldn't find file: %s\n" % path
    check_against_restatement(r, lst, 10, 1, 0.2, out)


def test_a_million_files_are_refused_before_the_device(tmp_path):
    lst, out = make_case(tmp_path, S=2, repeat=1 << 19)  # 2^20 paths: the packed 20-bit counters of the reference would overflow
    r = run_cli(["-l", lst, "--mac", "1", "-k", "31", "-p", "0.2", "-o", out], tmp_path)
    assert r.returncode in (-6, 134) and r.stderr.decode() == TERMINATE % (lk.TOO_MANY_WHAT % (1 << 20))
    assert r.stdout == b"" and outputs(out) == []


def test_fails_loudly_without_a_gpu(tmp_path, have_gpu):
    if have_gpu:
        pytest.skip("a HIP device is present")
    import kmersgwas_amd as kg
    lst, out = make_case(tmp_path)
    r = run_cli(["-l", lst, "--mac", "1", "-k", "31", "-p", "0.2", "-o", out], tmp_path)
    assert r.returncode == 3 and r.stderr.decode() == TOOL + ": no HIP device available: libkgwas has no CPU fallback\n"
    assert r.stdout == b"" and outputs(out) == []
    with pytest.raises(kg.KgwasError) as e:
        kg.list_kmers_found_in_multiple_samples([str(tmp_path / "acc0.sorted")], 31, 1, 0.2, out)
    assert e.value.code == kg.capi.KGWAS_ERR_DEVICE and outputs(out) == []


def test_library_guards_come_before_the_device(tmp_path):
    """The library's own refusals do not need a device: a null-free argument check, the file count, an empty file."""
    import kmersgwas_amd as kg
    lst, out = make_case(tmp_path, acc_bytes={1: b""})
    paths = [str(tmp_path / ("acc%d.sorted" % c)) for c in range(3)]
    with pytest.raises(kg.KgwasError) as e:
        kg.list_kmers_found_in_multiple_samples(paths, 31, 1, 0.2, out)
    assert e.value.code == kg.capi.KGWAS_ERR_FORMAT and e.value.msg == "sorted kmer file is empty: " + paths[1]
    with pytest.raises(kg.KgwasError) as e:
        kg.list_kmers_found_in_multiple_samples(paths[:1], 32, 1, 0.2, out)
    assert e.value.code == kg.capi.KGWAS_ERR_ARG
    with pytest.raises(kg.KgwasError) as e:
        kg.list_kmers_found_in_multiple_samples(paths[:1] * (1 << 20), 31, 1, 0.2, out)
    assert e.value.code == kg.capi.KGWAS_ERR_FORMAT and e.value.msg == lk.TOO_MANY_WHAT % (1 << 20)
    assert outputs(out) == []
