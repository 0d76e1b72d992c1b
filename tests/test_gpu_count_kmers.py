"""count_kmers_with_strand on the GPU (count_kernels.hip, count_kmers.cpp, bin/count_kmers_with_strand) against the restatements of
its rules (count_kmers_np.py, pinned by test_count_kmers.py): the output file byte for byte and all eight counters, nothing less.

KGWAS_COUNT_PASS_WORDS forces small key-range passes, KGWAS_COUNT_PIECE_BYTES small upload pieces (and with them small read blocks and
device segments), so that reads and runs of equal words meet the edges of encode tiles (4096 positions), of a lane's stretch (16), of
upload pieces, of the reduce kernels' tiles (2048 words) and of key ranges."""
import os
import subprocess

import numpy as np
import pytest

import kmersgwas_amd as kg
import count_kmers_np as ck
from test_count_kmers import BIN, CX, F1, F2, F3, HAND, HAND_BYTES, random_reads

pytestmark = pytest.mark.gpu
U = np.uint64
HOOKS = ("KGWAS_COUNT_PASS_WORDS", "KGWAS_COUNT_PIECE_BYTES")
TILE, LANE = 4096, 16


class hooks:
    def __init__(self, pass_words=None, piece_bytes=None):
        self.new = dict(zip(HOOKS, (pass_words, piece_bytes)))

    def __enter__(self):
        self.old = {v: os.environ.get(v) for v in HOOKS}
        for v, x in self.new.items():
            os.environ.pop(v, None)
            if x:
                os.environ[v] = str(x)

    def __exit__(self, *a):
        for v, x in self.old.items():
            os.environ.pop(v, None)
            if x is not None:
                os.environ[v] = x


def acgt(rng, n):
    return bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=n)])


def assert_same(got_counts, out, want, what=""):
    with open(out, "rb") as f:
        got = f.read()
    exp = ck.file_bytes(want)
    assert tuple(got_counts) == tuple(want["counts"]), (what, got_counts, want["counts"])
    assert len(got) == len(exp) and got == exp, "%s: the file differs" % what


def check_bases(tmp_path, stream, k, ci, cx, want=None, tag="b", **hk):
    """The bases entry on a byte stream against the closed form (or `want`)."""
    stream = np.frombuffer(bytes(stream), np.uint8)
    if want is None:
        want = ck.closed_stream(stream, k, ci, cx)
    out = str(tmp_path / (tag + ".sorted"))
    with hooks(**hk):
        counts = kg.count_kmers(stream, k, ci, cx, out)
    assert_same(counts, out, want, tag)
    return want, out


def fastq_of(reads, crlf=False):
    nl = b"\r\n" if crlf else b"\n"
    return b"".join(b"@r%d" % i + nl + r + nl + b"+" + nl + b"@" * len(r) + nl for i, r in enumerate(reads))


def fasta_of(reads, width=60):
    return b"".join(b">s%d\n" % i + b"".join(r[j:j + width] + b"\n" for j in range(0, len(r), width)) for i, r in enumerate(reads))


def test_by_hand(tmp_path):
    for n, ((reads, k, ci, words, c012), raw) in enumerate(zip(HAND, HAND_BYTES)):
        want = ck.literal(reads, k, ci, CX)
        out = str(tmp_path / ("h%d" % n))
        counts = kg.count_kmers(ck.stream_of(reads), k, ci, CX, out)
        assert counts == want["counts"] and counts[:3] == c012
        assert open(out, "rb").read() == raw


@pytest.mark.parametrize("k", [1, 10, 15, 16, 17, 31])
def test_kmer_lengths(tmp_path, k):
    rng = np.random.default_rng(100 + k)
    reads = random_reads(rng, 60, 120, p_other=0.02)
    for ci, cx in ((1, CX), (2, CX), (1, 1)):
        want = ck.literal(reads, k, ci, cx) if k > 1 or ci == 1 else None
        check_bases(tmp_path, ck.stream_of(reads), k, ci, cx, want=want, tag="k%d_%d_%d" % (k, ci, cx))


@pytest.mark.parametrize("k", [1, 2, 16, 31])
def test_read_lengths_around_k(tmp_path, k):
    rng = np.random.default_rng(k)
    reads = [acgt(rng, n) for n in (k - 1, k, k + 1, k - 1, k, k + 1, 0)]
    want, _ = check_bases(tmp_path, ck.stream_of(reads), k, 1, CX, want=ck.literal(reads, k, 1, CX))
    assert want["counts"][7] == 2 * (1 + 2)
    check_bases(tmp_path, reads[1], k, 1, CX, tag="no_separator_behind")  # the stream ends with the read's last base
    check_bases(tmp_path, b"", k, 1, CX, tag="empty")
    check_bases(tmp_path, b"NNNN\n\n", k, 1, CX, tag="no_base")


@pytest.mark.parametrize("k", [10, 31])
def test_reads_at_tile_and_lane_edges(tmp_path, k):
    """One read per encode tile edge whose first window starts d positions from the edge, and one whose last window does, for
    every d within +-k; the offsets run through all places of a lane's stretch of 16 as well."""
    rng = np.random.default_rng(7 * k)
    L = 2 * k + 5
    stream = bytearray(b"N" * ((4 * k + 4) * TILE + TILE))
    reads = []
    for n, d in enumerate(range(-k, k + 1)):
        r1, r2 = acgt(rng, L), acgt(rng, L)
        e1, e2 = (2 * n + 1) * TILE, (2 * n + 2) * TILE
        stream[e1 + d:e1 + d + L] = r1              # first window at e1 + d
        stream[e2 + d - (L - k):e2 + d + k] = r2    # last window at e2 + d
        reads += [r1, r2]
    want = ck.closed(reads, k, 1, CX)
    assert want["counts"][7] == len(reads) * (L - k + 1)
    check_bases(tmp_path, stream, k, 1, CX, want=want)
    # a stream of bases only, with a few separators: windows at every position of every lane, tile after tile
    s = bytearray(acgt(rng, 3 * TILE + 5))
    for p in (TILE - 1, TILE + k, 2 * TILE, 2 * TILE + LANE - 1, 3 * TILE - k):
        s[p] = ord("N")
    check_bases(tmp_path, s, k, 1, CX, tag="dense")


@pytest.mark.parametrize("k,piece", [(10, 64), (31, 64), (31, 1000)])
def test_files_across_upload_pieces(tmp_path, k, piece):
    """The files entry with small pieces: a FASTA record far longer than a piece goes through the pieces in parts, so windows start
    at every offset from a piece's edge; FASTQ reads longer than a piece, and several to a piece, from several threads."""
    rng = np.random.default_rng(k + piece)
    long_read = bytearray(acgt(rng, 5000))
    for p in rng.integers(0, 5000, size=12):
        long_read[p] = ord("N")
    fa_reads = [bytes(long_read), acgt(rng, k), acgt(rng, k - 1), b"", acgt(rng, 700)]
    fq_reads = [acgt(rng, int(n)) for n in rng.integers(k - 1, 160, size=300)]
    fa, fq, fq2 = tmp_path / "a.fa", tmp_path / "b.fq", tmp_path / "c.fq"
    fa.write_bytes(fasta_of(fa_reads))
    fq.write_bytes(fastq_of(fq_reads))
    fq2.write_bytes(fastq_of(fq_reads[:50], crlf=True)[:-2])  # CRLF, no final newline
    files = [str(fa), str(fq), str(fq2)]
    reads = [r for f in files for r in ck.read_fastx(open(f, "rb").read())]
    assert reads == fa_reads + fq_reads + fq_reads[:50]
    want = ck.closed(reads, k, 1, CX)
    out = str(tmp_path / "files.sorted")
    with hooks(piece_bytes=piece):
        counts = kg.count_kmers(files, k, 1, CX, out)
    assert_same(counts, out, want, "files")
    # FASTQ and FASTA mixed in one call = the bases entry on the reader's stream
    _, out_b = check_bases(tmp_path, ck.stream_of(reads), k, 1, CX, want=want, tag="stream")
    assert open(out, "rb").read() == open(out_b, "rb").read()


def test_files_format_errors(tmp_path):
    good, bad, trunc, empty = (tmp_path / n for n in ("g.fq", "bad.txt", "t.fq", "e.fa"))
    good.write_bytes(fastq_of([b"ACGTACGTACGTAAC"]))
    bad.write_bytes(b"ACGT\n")
    trunc.write_bytes(fastq_of([b"ACGTACGTACGTAAC", b"ACGTACGTACGTAAG"])[:-17])
    empty.write_bytes(b"")
    out = str(tmp_path / "o")
    with pytest.raises(kg.KgwasError) as e:
        kg.count_kmers([str(good), str(bad)], 10, 1, CX, out)
    assert e.value.code == kg.capi.KGWAS_ERR_FORMAT and e.value.msg == "%s: neither FASTA nor FASTQ" % bad
    assert not os.path.exists(out)  # every input is looked at before the output is created
    with pytest.raises(kg.KgwasError) as e:
        kg.count_kmers([str(good), str(tmp_path / "gone")], 10, 1, CX, out)
    assert e.value.code == kg.capi.KGWAS_ERR_IO and not os.path.exists(out)
    with pytest.raises(kg.KgwasError) as e:
        kg.count_kmers([str(trunc)], 10, 1, CX, out)
    assert e.value.code == kg.capi.KGWAS_ERR_FORMAT and e.value.msg == "%s: the last FASTQ record has fewer than four lines" % trunc
    with pytest.raises(kg.KgwasError) as e:
        kg.count_kmers(str(good), 10, 3, 2, out)
    assert e.value.code == kg.capi.KGWAS_ERR_ARG
    for k in (0, 32):
        with pytest.raises(kg.KgwasError) as e:
            kg.count_kmers(str(good), k, 1, CX, out)
        assert e.value.code == kg.capi.KGWAS_ERR_ARG
    assert kg.count_kmers([str(empty), str(good), str(empty)], 10, 1, CX, out) == ck.literal([b"ACGTACGTACGTAAC"], 10, 1, CX)["counts"]
    assert kg.count_kmers([str(empty)], 10, 1, CX, out) == (0,) * 8 and os.path.getsize(out) == 0


@pytest.mark.parametrize("with_t", [False, True])
def test_a_run_longer_than_a_grid_stride(tmp_path, with_t):
    """200 000 A's: 199 970 equal sort words, far more than a reduce tile, with orient 0 only; a T read beside them adds the other
    orientation to the same key (flag 3). Random reads around them."""
    rng = np.random.default_rng(5)
    k = 31
    reads = [acgt(rng, 150) for _ in range(100)] + [b"A" * 200000] + [acgt(rng, 150) for _ in range(100)]
    if with_t:
        reads.insert(50, b"T" * 50000)
    want, _ = check_bases(tmp_path, ck.stream_of(reads), k, 2, CX)
    assert int(want["words"][0]) == (F3 if with_t else F1) and want["counts"][0] == 1  # key 0 alone is counted twice or more
    want, _ = check_bases(tmp_path, ck.stream_of(reads), k, 1, 200000 - k + 1, tag="cx")
    assert (int(want["words"][0]) & ~F3 == 0) == (not with_t)  # cx = the A windows: the T read's windows put the key above it


def test_counts_at_ci_and_cx(tmp_path):
    rng = np.random.default_rng(9)
    k, ci, cx = 15, 3, 5
    base = [acgt(rng, k + 6) for _ in range(4)]
    reads = base[0:1] * (ci - 1) + base[1:2] * ci + base[2:3] * cx + base[3:4] * (cx + 1)
    want = ck.literal(reads, k, ci, cx)
    assert want["counts"][0] == 2 * 7 and want["counts"][1] == 4 * 7
    check_bases(tmp_path, ck.stream_of(reads), k, ci, cx, want=want)
    for c1, c2 in ((1, CX), (1, 1), (ci, ci), (cx, cx), (cx + 1, cx + 1), (cx + 2, CX)):
        check_bases(tmp_path, ck.stream_of(reads), k, c1, c2, want=ck.literal(reads, k, c1, c2), tag="c%d_%d" % (c1, c2))


@pytest.mark.parametrize("k", [4, 10])
def test_palindromes(tmp_path, k):
    rng = np.random.default_rng(k)
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    reads = []
    for _ in range(300):
        h = acgt(rng, k // 2)
        reads.append(acgt(rng, 3) + h + h.translate(comp)[::-1] + acgt(rng, 3))  # a palindrome in the middle
    want = ck.literal(reads, k, 1, CX)
    def is_palindrome(key):
        c = [(key >> (2 * (k - 1 - i))) & 3 for i in range(k)]
        return all(c[i] == 3 - c[k - 1 - i] for i in range(k))
    pal = [w for w in want["words"] if is_palindrome(w & ~F3)]
    assert len(pal) >= (10 if k == 4 else 200) and all(w >> 62 == 2 for w in pal)  # a palindrome only ever gets the second flag
    check_bases(tmp_path, ck.stream_of(reads), k, 1, CX, want=want)


def run_tool(args, env=None, stdin=None):
    e = {v: x for v, x in os.environ.items() if v not in HOOKS}
    e.update(env or {})
    r = subprocess.run([BIN] + args, input=stdin, capture_output=True, timeout=300, env=e)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r


def trace_of(r):
    line = [l for l in r.stderr.decode().splitlines() if l.startswith("[kgwas] count:")][0]
    return {kv.split("=")[0]: kv.split("=")[1] for kv in line.split()[2:]}


def test_passes(tmp_path):
    """Small passes give the single pass's file: ~60 000 windows in passes of 4096 words; keys that ARE range boundaries (the
    boundaries are sampled keys, and every key here is in the file); a skewed input - every read begins with the same 12 bases and
    k = 12, so one key holds more words than a pass: its range is cut down to that key, which is decided without a sort."""
    rng = np.random.default_rng(21)
    k = 12
    uniform = [acgt(rng, 100) for _ in range(680)]
    head = acgt(rng, 12)
    skewed = [head + acgt(rng, 8) for _ in range(7000)]
    for name, reads, ci in (("uniform", uniform, 1), ("skewed", skewed, 1), ("skewed2", skewed + uniform, 2)):
        fq = tmp_path / (name + ".fq")
        fq.write_bytes(fastq_of(reads))
        want = ck.closed(reads, k, ci, CX)
        assert 55000 < want["counts"][7] < 130000
        single = str(tmp_path / (name + ".single"))
        counts = kg.count_kmers(str(fq), k, ci, CX, single)
        assert_same(counts, single, want, name)
        out = str(tmp_path / (name + ".passes"))
        r = run_tool(["-i", str(fq), "-k", str(k), "--ci", str(ci), "-o", out], env={"KGWAS_TRACE": "1", "KGWAS_COUNT_PASS_WORDS": "4096"})
        t = trace_of(r)
        assert int(t["passes"]) > 10 and int(t["pass_words"]) == 4096 and int(t["windows"]) == want["counts"][7]
        if name != "uniform":
            assert int(t["splits"]) > 0 and int(t["big_keys"]) == 1
        assert open(out, "rb").read() == open(single, "rb").read()
        assert r.stdout == ck.summary_of(want["counts"])
        r1 = run_tool(["-i", str(fq), "-k", str(k), "--ci", str(ci), "-o", out], env={"KGWAS_TRACE": "1"})
        assert int(trace_of(r1)["passes"]) == 1 and int(trace_of(r1)["splits"]) == 0
        # through the library as well, with small pieces on top
        with hooks(pass_words=1000, piece_bytes=256):
            assert kg.count_kmers(str(fq), k, ci, CX, out) == want["counts"]
        assert open(out, "rb").read() == open(single, "rb").read()


def test_device_pointer(tmp_path):
    import torch
    rng = np.random.default_rng(3)
    reads = random_reads(rng, 200, 150, p_other=0.01)
    stream = ck.stream_of(reads)
    want, out_h = check_bases(tmp_path, stream, 17, 1, CX)
    t = torch.frombuffer(bytearray(stream), dtype=torch.uint8)
    for name, x in (("dev", t.cuda()), ("dev_unaligned", torch.cat([t[:3], t]).cuda()[3:]), ("host_tensor", t)):
        out = str(tmp_path / name)
        assert kg.count_kmers(x, 17, 1, CX, out) == want["counts"], name
        assert open(out, "rb").read() == open(out_h, "rb").read(), name


def test_tool_stdin_list_and_summary(tmp_path):
    rng = np.random.default_rng(8)
    k = 21
    genome = acgt(rng, 3000)
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    reads = [genome[p:p + 100] for p in rng.integers(0, 2900, size=400)]
    reads = [r if i % 2 else r.translate(comp)[::-1] for i, r in enumerate(reads)]  # both strands, so that flag 3 occurs
    fqs = []
    for i in range(3):
        p = tmp_path / ("r%d.f%s" % (i, "a" if i == 1 else "q"))
        part = reads[i::3]
        p.write_bytes(fasta_of(part, 70) if i == 1 else fastq_of(part))
        fqs.append(str(p))
    lst = tmp_path / "files.txt"
    lst.write_text("".join(f + "\n" for f in fqs))
    for ci, cx in ((2, CX), (1, 3)):
        want = ck.closed(reads, k, ci, cx)
        if cx == CX:
            assert want["counts"][0] > 1000 and want["counts"][6] > 100 and want["counts"][4] > 0 and want["counts"][5] > 0
        else:
            assert 0 < want["counts"][0] < 1000  # (a coverage of 13: --cx 3 drops most keys)
        out = str(tmp_path / "list.sorted")
        cmd = ["-k", str(k), "-o", out] + ([] if (ci, cx) == (2, CX) else ["--ci", str(ci), "--cx", str(cx)])  # (--ci defaults to 2)
        r = run_tool(["-l", str(lst)] + cmd)
        assert r.stdout == ck.summary_of(want["counts"])
        assert open(out, "rb").read() == ck.file_bytes(want)
        assert len(r.stderr.decode().splitlines()) == 1 and r.stderr.startswith(b"[kgwas] seconds:")
        out2 = str(tmp_path / "stdin.sorted")
        r = run_tool(["-i", "-"] + cmd[:1] + [str(k), "-o", out2] + cmd[4:], stdin=fastq_of(reads))
        assert r.stdout == ck.summary_of(want["counts"])
        assert open(out2, "rb").read() == ck.file_bytes(want)


def test_chain_reads_to_table(tmp_path):
    """Reads -> sorted k-mer files -> list -> table -> filter_kmers: the table's keys and bits against a brute-force pass over the
    reads. Three accessions of one random 20 kb genome with a few substitutions each."""
    rng = np.random.default_rng(77)
    k, N = 31, 3
    genome = np.frombuffer(acgt(rng, 20000), np.uint8)
    files, per_acc = [], []
    for a in range(N):
        g = genome.copy()
        pos = rng.integers(0, len(g), size=8)
        g[pos] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=8)]
        g = bytes(g)
        reads = [g[p:p + 150] for p in rng.integers(0, len(g) - 150, size=1600)]
        comp = bytes.maketrans(b"ACGT", b"TGCA")
        reads = [r if i % 2 else r.translate(comp)[::-1] for i, r in enumerate(reads)]  # both strands
        fq = tmp_path / ("acc%d.fq" % a)
        fq.write_bytes(fastq_of(reads))
        out = str(tmp_path / ("acc%d.sorted" % a))
        want = ck.closed(reads, k, 2, CX)
        assert_same(kg.count_kmers(str(fq), k, 2, CX, out), out, want, "accession %d" % a)
        files.append(out)
        per_acc.append({int(w) & ~F3: int(w) >> 62 for w in want["words"]})
    # list_kmers' rule on these sets: in at least mac = 2 files, and with percent 0.2 of 2 or 3 files one file per strand side
    listed = []
    for key in sorted(set().union(*per_acc)):
        fl = [d[key] for d in per_acc if key in d]
        if len(fl) >= 2 and sum(f in (1, 3) for f in fl) >= 1 and sum(f in (2, 3) for f in fl) >= 1:
            listed.append(key)
    assert len(listed) > 15000 and len(set().union(*per_acc)) > len(listed)
    allk = str(tmp_path / "all.kmers")
    kg.list_kmers_found_in_multiple_samples(files, k, 2, 0.2, allk)
    assert np.fromfile(allk, "<u8").tolist() == listed
    base = str(tmp_path / "tab")
    assert kg.build_kmers_table(allk, files, ["acc%d" % a for a in range(N)], k, base) == len(listed)
    table = kg.KmersTable(base, k)
    rows = table.read_rows(0, table.n_rows)
    assert rows[:, 0].tolist() == listed
    bits = [sum(1 << a for a in range(N) if key in per_acc[a]) for key in listed]
    assert rows[:, 1].tolist() == bits and 0 < sum(b != 7 for b in bits) < len(bits)
    partial = [i for i, b in enumerate(bits) if b != 7]
    pick = [partial[0], 0, len(listed) - 1, partial[-1], len(listed) // 2]
    file_rows, got = kg.filter_kmers(table, np.array([listed[i] for i in pick], U))
    assert file_rows.tolist() == sorted(set(pick)) and got[:, 1].tolist() == [bits[i] for i in sorted(set(pick))]
    table.close()


def test_default_hooks_twenty_million_windows(tmp_path):
    """2 Mb of genome at coverage 10 in reads of 150 with substitutions: 2 * 10^7 windows in one pass at the default sizes."""
    rng = np.random.default_rng(2024)
    k, G, n_reads, L = 31, 2_000_000, 166_000, 150
    genome = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=G)]
    starts = rng.integers(0, G - L, size=n_reads)
    m = genome[starts[:, None] + np.arange(L)[None, :]].copy()
    sub = rng.random(m.shape) < 0.005
    m[sub] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=int(sub.sum()))]
    m[::2] = np.frombuffer(bytes.maketrans(b"ACGT", b"TGCA"), np.uint8)[m[::2, ::-1]]
    stream = np.concatenate([m, np.full((n_reads, 1), 10, np.uint8)], axis=1).reshape(-1)
    want = ck.closed_stream(stream, k, 2, CX)
    assert want["counts"][7] == n_reads * (L - k + 1) and want["counts"][7] > 1.9e7
    out = str(tmp_path / "big.sorted")
    counts = kg.count_kmers(stream, k, 2, CX, out)
    assert counts == want["counts"]
    assert np.array_equal(np.fromfile(out, "<u8"), np.asarray(want["words"], U))
