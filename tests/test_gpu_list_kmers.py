"""list_kmers_found_in_multiple_samples on the GPU (list_kernels.hip, list_kmers.cpp, bin/list_kmers_found_in_multiple_samples) against
the restatement (list_kmers_np.py): every output file of the library call and of the tool byte for byte, the returned counts and the
summary lines.

KGWAS_LIST_PIECE_WORDS forces small pieces (runs of whole windows), KGWAS_LIST_BUCKET_WORDS small key-range buckets and LDS tables,
KGWAS_LIST_BLOCK_WORDS small read blocks, so that runs of a key, window edges, empty slices, descents and full tables meet piece, bucket
and block boundaries. Small cases are checked against the literal form as well as the closed form (which test_list_kmers.py pins to it)."""
import os
import subprocess

import numpy as np
import pytest

import kmersgwas_amd as kg
import list_kmers_np as lk
from test_list_kmers import F1, F2, F3, NAN, TERMINATE, random_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "kmersgwas_amd", "bin", "list_kmers_found_in_multiple_samples")
U = np.uint64
HOOKS = ("KGWAS_LIST_PIECE_WORDS", "KGWAS_LIST_BUCKET_WORDS", "KGWAS_LIST_BLOCK_WORDS")
SMALL = (37, 8, 16)


def write_inputs(d, acc):
    os.makedirs(d, exist_ok=True)
    paths = []
    for c, w in enumerate(acc):
        p = os.path.join(d, "a%d.sorted" % c)
        np.asarray(w, "<u8").tofile(p)
        paths.append(p)
    lst = os.path.join(d, "list.txt")
    with open(lst, "w") as f:
        f.write("".join("%s\tacc_%d\n" % (p, c) for c, p in enumerate(paths)))
    return paths, lst


def read_outputs(out):
    files = {}
    for e in lk.EXTS:
        with open(out + e, "rb") as f:
            files[e] = f.read()
    return files


def assert_files(got, want, what):
    for e in lk.EXTS:
        assert len(got[e]) == len(want[e]) and got[e] == want[e], "%s: <o>%s differs" % (what, e)


def check(tmp_path, acc, k, mac, p, hooks=(None,), cli=True, tag="x", literal=None):
    """The library (once per entry of hooks: None = defaults, or (piece, bucket, block) words) and the tool (with the first entry)
    on these inputs against the restatement; returns the restatement's result."""
    acc = [np.asarray(a, U) for a in acc]
    d = str(tmp_path / tag)
    paths, lst = write_inputs(d, acc)
    want = lk.restate(lst, k, mac, p)
    if literal is None:
        literal = sum(len(a) for a in acc) <= 30000 and len(acc) <= 130  # (5001 windows x N calls in Python)
    if literal and want["kind"] == "ok":
        assert lk.same(lk.literal(acc, k, mac, p), want["res"]), "the closed form differs from the literal form"
    old = {v: os.environ.get(v) for v in HOOKS}
    for n, h in enumerate(hooks):
        env = {v: str(x) for v, x in zip(HOOKS, h or ()) if x}
        try:
            for v in HOOKS:
                os.environ.pop(v, None)
            os.environ.update(env)
            out = os.path.join(d, "lib%d" % n)
            if want["kind"] == "ok":
                assert kg.list_kmers_found_in_multiple_samples(paths, k, mac, p, out) == want["counts"], (tag, h)
            else:
                with pytest.raises(kg.KgwasError) as e:
                    kg.list_kmers_found_in_multiple_samples(paths, k, mac, p, out)
                assert e.value.code == kg.capi.KGWAS_ERR_FORMAT and e.value.msg == want["what"], (tag, h)
        finally:
            for v, val in old.items():
                os.environ.pop(v, None)
                if val is not None:
                    os.environ[v] = val
        if want["kind"] == "ok":
            assert_files(read_outputs(out), want["files"], "library (%s, hooks %s)" % (tag, h))
    if cli:
        out = os.path.join(d, "cli")
        e2 = {v: val for v, val in os.environ.items() if v not in HOOKS}
        e2.update({v: str(x) for v, x in zip(HOOKS, hooks[0] or ()) if x})
        r = subprocess.run([BIN, "-l", lst, "-k", str(k), "--mac", str(mac), "-p", repr(float(p)), "-o", out], capture_output=True, timeout=600,
                           env=e2)
        assert r.stdout == b""
        err = r.stderr.decode()
        if want["kind"] == "ok":
            assert r.returncode == 0, err[-2000:]
            assert err.startswith(want["stderr"] + "[kgwas] seconds:") and len(err.splitlines()) == 4
            assert_files(read_outputs(out), want["files"], "tool (%s)" % tag)
        else:
            assert r.returncode in (-6, 134) and err == TERMINATE % want["what"]
    return want


def flagged(rng, w):
    return (np.asarray(w, U) | (rng.integers(1, 4, size=len(w), dtype=U) << U(62))).astype(U)


def sorted_case(rng, N, k, n_keys, per_acc):
    """N sorted files without duplicates whose keys come from a pool spread over the 2k-bit key space (a multiplicity of about
    N * per_acc / n_keys), some files wholly inside a short stretch of it (so many of their slices are empty)."""
    top = (1 << (2 * k)) - 1
    pool = np.unique(rng.integers(0, top, size=n_keys, dtype=U, endpoint=True))
    acc = []
    for c in range(N):
        m = int(rng.integers(1, 2 * per_acc))
        w = np.unique(np.concatenate([rng.choice(pool, size=m), rng.integers(0, top, size=max(1, m // 8), dtype=U, endpoint=True)]))
        if c % 7 == 3:
            i = int(rng.integers(0, len(pool)))
            w = np.unique(rng.choice(pool[i:i + 5], size=m))
        acc.append(flagged(rng, w))
    return acc


@pytest.mark.parametrize("k", [10, 31])
@pytest.mark.parametrize("N", [1, 2, 3, 63, 64, 65, 130])
def test_file_counts_and_lengths(N, k, tmp_path):
    rng = np.random.default_rng(1000 * k + N)
    acc = sorted_case(rng, N, k, 400, 60)
    if k == 10:  # keys above the last threshold end a file's use (k = 10: step * 5001 = 1 050 210); flag 0 there is no error
        acc[0] = np.concatenate([acc[0][acc[0] & U(lk.MASK) <= 1050210], np.array([1050211, 1050300 | F1], U)])
    want = check(tmp_path, acc, k, min(5, N), 0.2, hooks=(SMALL, None, (5, 3, 2)), tag="w")
    assert want["kind"] == "ok" and sum(want["counts"]) > 0
    if N >= 63:
        assert want["counts"][0] > 0 and want["counts"][2] > 0


def test_runs_and_window_edges_at_every_boundary(tmp_path):
    """k = 10 (step 210: window 1 = keys 0..210, window 2 = 211..420): key 100 in all files behind 0..4 other words (its run straddles
    read blocks and buckets), 210 and 211 as neighbours, a file that lies in window 3 alone (a whole-file slice, empty slices before and
    after), files whose last word is exactly a threshold (420, 1 050 210)."""
    rng = np.random.default_rng(5)
    acc = []
    for i in range(5):
        acc.append(flagged(rng, list(range(1, i + 1)) + [100, 210, 211, 300 + i, 420]))
    acc.append(flagged(rng, [421, 500, 630]))
    acc.append(flagged(rng, [100, 210, 1050210]))
    acc.append(flagged(rng, [211]))
    hooks = (None, (4, 2, 2), (6, 3, 1), (3, 1, 2), (100, 4, 3), (16, 64, 5), (1, 1, 1))
    for mac, p in ((1, 0.0), (5, 0.2), (7, 0.5)):
        want = check(tmp_path, acc, 10, mac, p, hooks=hooks, tag="edges_%d" % mac, cli=mac == 5)
        assert want["kind"] == "ok"
    assert int(want["res"]["only_canonical"][6].sum()) == 3  # (100, 210 and 211, in six files each)


# k = 10: a descent inside one file (its words after it count for the window of the running maximum)
DESCENTS = {
    "same_window": [[5, 100, 7], [7, 100]],
    "into_the_next_window": [[300, 7, 650], [7, 300, 650], [7, 650]],
    "several_per_file": [[40, 30, 20, 10, 230, 225, 220, 640, 35, 430], [35, 30, 640, 210], [10, 20, 30, 35, 220, 430, 640]],
    # pieces of a few words: the descent is in one piece, the pieces before and after it are counted on the device
    "one_piece_of_many": [[10, 20, 220, 230, 650, 640, 860, 870, 1100], [10, 220, 640, 650, 870, 1100], [20, 230, 640, 860, 1100]],
}


@pytest.mark.parametrize("name", sorted(DESCENTS))
def test_descents_by_hand(name, tmp_path):
    rng = np.random.default_rng(3)
    acc = [flagged(rng, a) for a in DESCENTS[name]]
    want = check(tmp_path, acc, 10, 2, 0.0, hooks=(None, (6, 4, 2), (1, 1, 1), (8, 2, 3), (40, 3, 4)), tag=name)
    assert want["kind"] == "ok"
    if name == "into_the_next_window":  # file 0's 7 is an item of window 2: written after window 1's 7, counted apart from it
        assert want["res"]["passed"] == [7, 300, 650]


def test_random_cases_with_descents_and_duplicates(tmp_path):
    rng = np.random.default_rng(78)
    kinds = set()
    for i in range(40):
        k = int(rng.choice([10, 11, 15, 31]))
        acc = random_case(rng, k, flags0=i % 13 == 12)
        mac = int(rng.choice([0, 1, 2, 5, len(acc), len(acc) + 1]))
        p = float(rng.choice([0.0, 0.2, 0.5, 1.0, 1.5, -1.0, NAN]))
        h = [None, (1, 1, 1), (7, 2, 3), (50, 8, 7), (400, 64, 64), (5, 100, 2)][int(rng.integers(0, 6))]
        kinds.add(check(tmp_path, acc, k, mac, p, hooks=(h,), tag="r%d" % i, cli=i % 8 == 0, literal=False)["kind"])
    assert kinds == {"ok", "abort"}


def test_duplicates_inside_a_file(tmp_path):
    # 7 twice in file 0: counted twice (with file 1's: three times in three files)
    acc = [np.array([7 | F1, 7 | F3, 9 | F1], U), np.array([7 | F2, 9 | F3], U), np.array([11 | F3], U)]
    want = check(tmp_path, acc, 10, 3, 0.5, hooks=(None, SMALL, (2, 1, 1)), tag="dup")
    assert want["res"]["passed"] == [7] and want["counts"] == (1, 0, 2) and int(want["res"]["only_canonical"][3][1]) == 1
    # a fourth 7 is more than there are files: the reference would write outside its matrices
    acc[2] = np.array([7 | F3, 11 | F3], U)
    want = check(tmp_path, acc, 10, 3, 0.5, hooks=(None, SMALL, (2, 1, 1)), tag="dup_above")
    assert want["kind"] == "abort" and want["what"] == lk.ABOVE_N_WHAT % ("AAAAAAAACT", 3)


def test_flag_zero(tmp_path):
    rng = np.random.default_rng(8)
    acc = [flagged(rng, [5, 9, 300]), np.array([5 | F1, 9, 300 | F2], U), flagged(rng, [9, 400])]
    want = check(tmp_path, acc, 10, 1, 0.0, hooks=(None, SMALL, (2, 1, 1)), tag="flag0")
    assert want["kind"] == "abort" and want["what"].endswith("a1.sorted")
    # beyond window 5001 (k = 10: keys above 1 050 210) a word is never used, whatever its flag
    acc[1] = np.array([5 | F1, 300 | F2, 1050211, 1050212], U)
    want = check(tmp_path, acc, 10, 1, 0.0, hooks=(None, SMALL, (2, 1, 1)), tag="flag0_unused")
    assert want["kind"] == "ok" and want["counts"] == (4, 0, 0)


def test_many_words_in_a_tiny_key_range(tmp_path):
    """130 files share the same 50 keys: 6500 words in buckets aimed at 8, with tables of 64 slots."""
    rng = np.random.default_rng(10)
    keys = np.sort(rng.integers(0, 1 << 62, size=50, dtype=U))
    keys[10:20] = keys[10] + np.arange(10, dtype=U)  # (ten of them neighbours)
    acc = [flagged(rng, keys) for _ in range(130)]
    want = check(tmp_path, acc, 31, 5, 0.2, hooks=((100000, 8, 16), (100000, 1, 7), None), tag="tiny")
    assert want["kind"] == "ok" and sum(want["counts"]) == 50 and int(want["res"]["only_canonical"][130].sum()) == 50


def test_a_full_table_goes_through_the_host(tmp_path):
    """20 000 distinct keys in one bucket's range: more than an LDS table holds, so the piece is counted by the host's loop; with small
    pieces only the pieces that overflow are."""
    rng = np.random.default_rng(11)
    keys = np.unique(rng.integers(0, 1 << 62, size=20000, dtype=U))
    acc = [flagged(rng, keys[0::2]), flagged(rng, keys[1::2])]
    want = check(tmp_path, acc, 31, 1, 0.0, hooks=((1 << 20, 1 << 20, 4096), (6000, 1 << 20, 512)), tag="full", literal=False)
    assert want["kind"] == "ok" and want["counts"] == (len(keys), 0, 0)


def test_hot_statistics_cells(tmp_path):
    """200 000 singletons with flag 1 in 4 files: every key adds to the cells [1][1], [1][0], [1][0]; then 100 000 keys in exactly two
    files each, once with flag 1 and once with flag 2: cells [2][1], [2][1], [2][0]."""
    rng = np.random.default_rng(12)
    keys = np.unique(rng.integers(0, 1 << 62, size=200000, dtype=U))
    n = len(keys)
    want = check(tmp_path, [keys[i::4] | U(F1) for i in range(4)], 31, 1, 0.0, tag="single", literal=False, cli=False)
    r = want["res"]
    assert want["counts"] == (n, 0, 0) and int(r["only_canonical"][1][1]) == n and int(r["only_non_canonical"][1][0]) == n
    assert int(r["both"][1][0]) == n and int(r["shareness"][1]) == n
    half = keys[:n // 2]
    want = check(tmp_path, [half[0::2] | U(F1), half[0::2] | U(F2), half[1::2] | U(F2), half[1::2] | U(F1)], 31, 2, 0.5, tag="pairs",
                 literal=False, cli=False)
    r = want["res"]
    assert want["counts"] == (len(half), 0, 0) and int(r["only_canonical"][2][1]) == len(half) and int(r["both"][2][0]) == len(half)
    assert int(r["shareness"][2]) == len(half)


@pytest.mark.parametrize("mac", [0, 1, 5, 12, 13])
def test_mac_and_strand_percent(mac, tmp_path):
    """One shared input of N = 12 files (mac = N and N + 1 among the cases) under every strand bound."""
    rng = np.random.default_rng(13)
    acc = sorted_case(rng, 12, 31, 60, 30)
    for p in (0.2, 0.5, 0.0, 1.0, 1.5, -1.0, NAN):
        want = check(tmp_path, acc, 31, mac, p, hooks=((4096, 64, 256),), tag="m%d_%s" % (mac, p), cli=p in (0.2, NAN), literal=p == 0.2)
        assert want["kind"] == "ok"
        n_pass, n_no_pass, low = want["counts"]
        if mac == 13 or (p != p or p == 1.5) and mac > 0:
            assert n_pass == 0
        if p in (0.0, -1.0):
            assert n_no_pass == 0


def test_large_case_default_pieces(tmp_path):
    """1135 accessions of about 2000 words each, keys drawn from 20 000 distinct values at k = 31, default piece, bucket and block
    sizes; the Python wrapper returns the counts the tool prints."""
    rng = np.random.default_rng(2025)
    pool = np.unique(rng.integers(0, 1 << 62, size=20000, dtype=U))
    acc = []
    for _ in range(1135):
        w = np.unique(rng.choice(pool, size=2000))
        acc.append(np.where(w <= pool[500], w | U(F1), flagged(rng, w)))  # (the lowest keys in canonical form only: they fail the strand rule)
    want = check(tmp_path, acc, 31, 5, 0.2, tag="large", literal=False)
    assert want["kind"] == "ok" and want["counts"][0] > 0 and want["counts"][1] > 0


def test_which_pieces_take_the_host_loop(tmp_path):
    """KGWAS_TRACE=1 adds a line that says how many pieces the device and the host's loop counted: sorted files never take the host's
    loop, a descent takes it for its own piece only, a table that fills for the pieces that fill it."""
    rng = np.random.default_rng(14)
    keys = np.unique(rng.integers(0, 1 << 62, size=9000, dtype=U))
    cases = {
        "sorted": ([flagged(rng, keys[rng.random(len(keys)) < 0.3]) for _ in range(9)], (2000, 64, 100)),
        "descent": ([flagged(rng, a) for a in DESCENTS["one_piece_of_many"]], (6, 4, 2)),
        "full": ([flagged(rng, keys[0::2]), flagged(rng, keys[1::2])], (1 << 20, 1 << 20, 4096)),
    }
    for name, (acc, h) in cases.items():
        paths, lst = write_inputs(str(tmp_path / name), acc)
        env = dict(os.environ, KGWAS_TRACE="1", **{v: str(x) for v, x in zip(HOOKS, h)})
        r = subprocess.run([BIN, "-l", lst, "-k", "31" if name != "descent" else "10", "--mac", "1", "-p", "0", "-o", str(tmp_path / name / "o")],
                           capture_output=True, timeout=600, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        trace = [l for l in r.stderr.decode().splitlines() if l.startswith("[kgwas] list:")]
        assert len(trace) == 1
        n = {kv.split("=")[0]: int(kv.split("=")[1]) for kv in trace[0].split()[2:]}
        if name == "sorted":
            assert n["host_pieces"] == 0 and n["device_pieces"] > 3 and n["device_words"] == sum(len(a) for a in acc)
        elif name == "descent":
            assert n["host_pieces"] == 1 and n["device_pieces"] >= 2
        else:
            assert n["host_pieces"] == 1 and n["device_pieces"] == 0
