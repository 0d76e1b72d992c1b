"""The SNP scorer (associate_snps: snp_kernels.hip, snps.cpp) beyond one chunk and one shape.

A NumPy statement of calculate_grammmar_approx_association (tests/snp_numpy.py) is pinned bit for bit to the oracle's C++
restatement on the CPU. On the GPU, SnpsDataBase.scores / .best and the associate_snps tool are compared with the oracle
at sample counts around every 32-sample lane and 128-sample block, at phenotype and MAC edges, at top-N sizes around the SNP
count, with up to 400 columns, and across chunk boundaries (KGWAS_SNP_CHUNK_SNPS, and the default chunk of 2^20 SNPs)."""
import os
import subprocess

import numpy as np
import pytest

from oracle import binding as ob
from helpers import phenotypes
import snp_numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "kmersgwas_amd", "bin")


def _random_dubits(n_snps, n_file, seed, p=(0.45, 0.05, 0.2, 0.3)):
    rng = np.random.default_rng(seed)
    dub = rng.choice(4, size=(n_snps, n_file), p=list(p)).astype(np.uint8)
    if n_snps >= 12:
        dub[:3] = 0              # monomorphic: fails every MAC above 0, 0/0 at mac 0
        dub[3:5] = 1             # all missing: N = 0
        dub[5, : n_file // 2] = 3
        dub[6] = dub[5]          # a duplicate pair: equal scores
        dub[7] = 2               # all heterozygous
    return dub


def _write_trio(base, dub, names=None):
    """PLINK .bed/.bim/.fam of dubits[n_snps][n_file]; returns (sample names, .bed body [n_snps][bytes per SNP])."""
    n_snps, n_file = dub.shape
    bps = (n_file + 3) // 4
    body = np.zeros((n_snps, bps), np.uint8)
    for s_ in range(n_file):
        body[:, s_ // 4] |= (dub[:, s_] << ((s_ % 4) * 2)).astype(np.uint8)
    names = names or ["smp%d" % i for i in range(n_file)]
    with open(base + ".bed", "wb") as f:
        f.write(bytes([0x6C, 0x1B, 0x01]) + body.tobytes())
    with open(base + ".bim", "w") as f:
        f.write("".join("1\tsnp%d\t0\t%d\tA\tG\n" % (i, 100 + i) for i in range(n_snps)))
    with open(base + ".fam", "w") as f:
        f.write("".join("%s %s 0 0 0 -9\n" % (n, n) for n in names))
    return names, body


def _phenotype(kind, S, P, seed):
    """P columns over S samples: the scan suite's float32 edges, a NaN value, a constant column, or plain Gaussians."""
    if kind in ("subnormal", "mixed_subnormal", "huge", "near_max", "neg_zero", "one_hot"):
        from test_gpu_parity import _edge_phenotypes
        return _edge_phenotypes(kind, S, P, np.random.default_rng(seed))
    Y = phenotypes(S, P - 1, seed=seed)
    if kind == "nan":
        Y[0, S // 2] = np.float32("nan")
        Y[P - 1, 0] = np.float32("nan")
    elif kind == "constant":
        Y[0] = np.float32(1.75)
    return np.ascontiguousarray(Y, np.float32)


def _oracle_scores(body, n_file, pick, Y, mac):
    return np.stack([ob.snps_scores(body.tobytes(), n_file, pick, Y[j], mac) for j in range(Y.shape[0])])


def _oracle_best(exp, topn):
    """get_most_associated_snps on a literal std::priority_queue: sorted SNP indices per column."""
    out = []
    for j in range(exp.shape[0]):
        h = ob.Heap(topn)
        h.add_many(np.zeros(exp.shape[1], np.uint64), exp[j], np.arange(exp.shape[1], dtype=np.uint64))
        out.append(np.sort(h.pop_all()[2]))
    return out


def _check_db(db, body, n_file, pick, Y, mac, topn):
    exp = _oracle_scores(body, n_file, pick, Y, mac)
    got = db.scores(Y, mac)
    assert got.tobytes() == exp.tobytes(), "scores differ at %s" % np.argwhere(got.view(np.uint64) != exp.view(np.uint64))[:5]
    best = db.best(Y, topn, mac)
    for j, rows in enumerate(_oracle_best(exp, topn)):
        assert best[j].dtype == np.uint64 and (best[j] == rows).all(), "column %d: top-%d differs" % (j, topn)
    return exp


# ---- CPU: the third statement against the oracle -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["normal", "subnormal", "mixed_subnormal", "huge", "near_max", "neg_zero", "one_hot", "nan",
                                  "constant"])
@pytest.mark.parametrize("n_file,n_use", [(9, 6), (130, 129), (300, 257)])
def test_snp_numpy_statement_equals_oracle(kind, n_file, n_use):
    """tests/snp_numpy.py and oracle.cpp state calculate_grammmar_approx_association independently; on random trios (every
    dubit value, shuffled subsets) and every phenotype edge the two give the same score bits, at mac 0 (0/0 = NaN) too."""
    dub = _random_dubits(200, n_file, seed=n_file + len(kind))
    bps = (n_file + 3) // 4
    body = np.zeros((dub.shape[0], bps), np.uint8)
    for s_ in range(n_file):
        body[:, s_ // 4] |= (dub[:, s_] << ((s_ % 4) * 2)).astype(np.uint8)
    pick = np.random.default_rng(n_use).permutation(n_file)[:n_use]
    Y = _phenotype(kind, n_use, 3 if n_use < 10 else 6, seed=n_use)
    for mac in (0.0, 1.5, float(max(np.ceil(0.05 * n_use), 1))):
        for j in range(Y.shape[0]):
            exp = ob.snps_scores(body.tobytes(), n_file, pick, Y[j], mac)
            got = snp_numpy.snps_scores(body, n_file, pick, Y[j], mac)
            assert got.tobytes() == exp.tobytes(), (kind, mac, j, np.argwhere(got.view(np.uint64) != exp.view(np.uint64))[:5])
    if kind == "huge":
        assert not np.isfinite(exp).all()


def test_snp_numpy_statement_lane_order():
    """The lane walk itself, spelt out: on values whose float32 sums depend on the order, the statement adds sample
    128 b + 32 l + 31 - s at step s of lane l and the lanes as ((l0 + l1) + l2) + l3 - neither in sample order nor pairwise."""
    S = 256
    rng = np.random.default_rng(1)  # (a seed on which the three orders give three different floats)
    y = (rng.standard_normal(S) * 10.0 ** rng.uniform(-3, 3, S)).astype(np.float32)
    plane = np.ones((1, S), bool)
    got = snp_numpy.lane_dot(plane, y)[0]
    acc = [np.float32(0)] * 4
    for b in range(2):
        for s in range(32):
            for l in range(4):
                acc[l] = np.float32(acc[l] + y[128 * b + 32 * l + 31 - s])
    assert got == np.float64(np.float32(np.float32(acc[0] + acc[1]) + acc[2]) + acc[3])
    seq = np.float32(0)
    for v in y:  # (sample order gives another float: the test would see a statement that ignored the lanes)
        seq = np.float32(seq + v)
    assert got != np.float64(seq) and got != np.float64(np.float32(acc[0] + acc[1]) + np.float32(acc[2] + acc[3]))


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n_use", [1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1135, 5121, 12000])
def test_snps_sample_counts(tmp_path, n_use):
    """Phenotyped sample counts around the 32-sample lanes and 128-sample blocks, up to 12 000. File sample counts alternate
    between a multiple of 4 (the last .fam sample, in the last dubit of the last byte, is phenotyped) and not; the subset is
    in shuffled order; counts divisible by 5 list one name twice."""
    import kmersgwas_amd as kg
    n_file = (n_use + 3) // 4 * 4 + 4 if n_use % 2 else n_use + (1 if (n_use + 2) % 4 == 0 else 2)
    n_snps = 900 if n_use < 5000 else 300
    dub = _random_dubits(n_snps, n_file, seed=n_use)
    base = str(tmp_path / "g")
    names, body = _write_trio(base, dub)
    rng = np.random.default_rng(n_use + 1)
    pick = rng.permutation(n_file)[:n_use]
    if n_use > 2 and n_use % 5 == 0:
        pick[1] = pick[0]
    if n_file % 4 == 0 and n_file - 1 not in pick:
        pick[-1] = n_file - 1
    assert n_file % 4 != 0 or n_file - 1 in pick
    use = [names[i] for i in pick]
    Y = phenotypes(n_use, 2, seed=n_use)
    mac = float(max(np.ceil(0.05 * n_use), 1))
    db = kg.SnpsDataBase(base, use)
    assert (db.n_snps, db.n_samples_file) == (n_snps, n_file)
    exp = _check_db(db, body, n_file, pick, Y, mac, 57)
    if n_use >= 5:
        assert (exp[:, 8:] > 0).any()
    _check_db(db, body, n_file, pick, Y[:1], 0.0, n_snps // 3)
    db.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["subnormal", "mixed_subnormal", "huge", "near_max", "neg_zero", "one_hot", "nan", "constant"])
def test_snps_phenotype_edges(tmp_path, kind):
    """Phenotype values at the float32 edges (the scan suite's kinds, a NaN value, a constant column): score bits, including
    inf and NaN scores, and the top-N lists equal the oracle's."""
    import kmersgwas_amd as kg
    n_file, n_use, n_snps = 300, 257, 1200
    base = str(tmp_path / "g")
    names, body = _write_trio(base, _random_dubits(n_snps, n_file, seed=len(kind)))
    pick = np.random.default_rng(3).permutation(n_file)[:n_use]
    Y = _phenotype(kind, n_use, 6, seed=11)
    db = kg.SnpsDataBase(base, [names[i] for i in pick])
    for mac in (13.0, 0.0):
        exp = _check_db(db, body, n_file, pick, Y, mac, 101)
    if kind in ("huge", "nan"):
        assert not np.isfinite(exp).all()
    db.close()


@pytest.mark.gpu
def test_snps_mac_edges(tmp_path):
    """The MAC predicate at its edges: mac 0 (0/0 = NaN scores go through best()); mac exactly S_gi and exactly N - S_gi at
    half-integer values from heterozygous calls (2.5 passes, 3.0 fails); mac above n / 2, where every score is 0 and the top-N
    is all ties."""
    import kmersgwas_amd as kg
    n_file = n_use = 40
    dub = _random_dubits(500, n_file, seed=9)
    # S_gi = 2.5: two homozygous major + one heterozygous, the rest homozygous minor
    dub[20] = 0; dub[20, [3, 17]] = 3; dub[20, 30] = 2
    # N - S_gi = 2.5: the mirror image, with some missing calls
    dub[21] = 3; dub[21, [4, 9]] = 0; dub[21, 11] = 2; dub[21, [0, 1]] = 1
    # S_gi = 3 (two heterozygous + two homozygous major), and N - S_gi = 3
    dub[22] = 0; dub[22, [1, 2]] = 2; dub[22, [5, 6]] = 3
    dub[23] = 3; dub[23, [7, 8, 9]] = 0
    base = str(tmp_path / "g")
    names, body = _write_trio(base, dub)
    pick = np.arange(n_file)
    Y = phenotypes(n_use, 3, seed=5)
    db = kg.SnpsDataBase(base, names)
    s = {}
    for mac in (0.0, 2.5, 3.0, 20.5, 21.0):
        for topn in (10, 499, 600):
            s[mac] = _check_db(db, body, n_file, pick, Y, mac, topn)
    assert np.isnan(s[0.0][:, :5]).all()
    assert (s[2.5][:, 20:22] != 0).all() and (s[3.0][:, 20:22] == 0).all()
    assert (s[3.0][:, 22:24] != 0).all() and (s[3.0][:, 22:24] == s[0.0][:, 22:24]).all()
    assert (s[21.0] == 0).all()
    db.close()


@pytest.mark.gpu
@pytest.mark.parametrize("P", [1, 101, 400])
def test_snps_topn_and_column_counts(tmp_path, P):
    """top-N of 1, n_snps - 1, n_snps and n_snps + 5, for 1, 101 and 400 columns (more columns than the heap threads)."""
    import kmersgwas_amd as kg
    n_file, n_use, n_snps = 150, 129, 700
    base = str(tmp_path / "g")
    names, body = _write_trio(base, _random_dubits(n_snps, n_file, seed=P))
    pick = np.random.default_rng(P).permutation(n_file)[:n_use]
    Y = phenotypes(n_use, P - 1, seed=P)
    db = kg.SnpsDataBase(base, [names[i] for i in pick])
    exp = _oracle_scores(body, n_file, pick, Y, 7.0)
    assert db.scores(Y, 7.0).tobytes() == exp.tobytes()
    for topn in (1, n_snps - 1, n_snps, n_snps + 5):
        best = db.best(Y, topn, 7.0)
        for j, rows in enumerate(_oracle_best(exp, topn)):
            assert len(rows) == min(topn, n_snps) and (best[j] == rows).all(), (topn, j)
    db.close()


def _tool_case(tmp_path, n_file, n_use, n_snps, P, seed):
    base = str(tmp_path / "g")
    names, body = _write_trio(base, _random_dubits(n_snps, n_file, seed=seed))
    pick = np.random.default_rng(seed).permutation(n_file)[:n_use]
    use = [names[i] for i in pick]
    Y = phenotypes(n_use, P - 1, seed=seed)
    pnames = ["trait%d" % j for j in range(P)]
    ph = tmp_path / "ph.tsv"
    with open(ph, "w") as f:
        f.write("accession_id\t" + "\t".join(pnames) + "\n")
        for i, a in enumerate(use):
            f.write(a + "\t" + "\t".join(repr(float(Y[j, i])) for j in range(P)) + "\n")
    return base, names, body, pick, use, Y, pnames, ph


def _expected_tool_files(outdir, base, body, lists, pnames):
    """output_plink_bed_file, restated as in test_gpu_cli.py::test_associate_snps: the selected .bim lines and .bed rows."""
    bim_lines = open(base + ".bim").read().split("\n")
    for j, pn in enumerate(pnames):
        with open(os.path.join(outdir, "o.%s.bed" % pn), "wb") as f:
            f.write(bytes([0x6C, 0x1B, 0x01]) + body[lists[j].astype(np.int64)].tobytes())
        with open(os.path.join(outdir, "o.%s.bim" % pn), "w") as f:
            f.write("".join(bim_lines[int(i)] + "\n" for i in lists[j]))


def _same_dirs(a, b):
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    assert fa == fb, (fa, fb)
    for f in fa:
        assert open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read(), f


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [1, 7, 1000, -1, 0])
def test_snps_chunk_boundaries(tmp_path, monkeypatch, chunk):
    """KGWAS_SNP_CHUNK_SNPS cuts the SNPs into chunks of 1, 7, 1000, n_snps - 1 and n_snps (0 and -1 below): scores (one copy
    per column from the second chunk on), top-N lists (heaps fed across chunks) and the tool's files equal the oracle's."""
    import kmersgwas_amd as kg
    n_file, n_use, n_snps, P, topn = 310, 301, 2345, 3, 150
    monkeypatch.setenv("KGWAS_SNP_CHUNK_SNPS", str(n_snps + chunk if chunk <= 0 else chunk))
    base, names, body, pick, use, Y, pnames, ph = _tool_case(tmp_path, n_file, n_use, n_snps, P, seed=23)
    mac = float(max(np.ceil(0.05 * n_use), 5.0))
    db = kg.SnpsDataBase(base, use)
    exp = _check_db(db, body, n_file, pick, Y, mac, topn)
    _check_db(db, body, n_file, pick, Y[1:], 0.0, n_snps - 2)
    db.close()
    out_p, out_o = tmp_path / "prod", tmp_path / "orc"
    out_p.mkdir(); out_o.mkdir()
    _expected_tool_files(str(out_o), base, body, _oracle_best(exp, topn), pnames)
    r = subprocess.run([os.path.join(BIN, "associate_snps"), str(ph), base, str(out_p / "o"), str(topn), "0.05", "5"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    _same_dirs(str(out_p), str(out_o))


@pytest.mark.gpu
def test_snps_default_chunk_over_a_million_snps(tmp_path, monkeypatch):
    """More than 2^20 SNPs at the default chunk size (no hook): two chunks, the second one ragged."""
    import kmersgwas_amd as kg
    monkeypatch.delenv("KGWAS_SNP_CHUNK_SNPS", raising=False)
    n_file, n_use, n_snps, P, topn = 14, 11, (1 << 20) + 3001, 3, 2000
    base = str(tmp_path / "g")
    names, body = _write_trio(base, _random_dubits(n_snps, n_file, seed=31))
    pick = np.random.default_rng(31).permutation(n_file)[:n_use]
    Y = phenotypes(n_use, P - 1, seed=31)
    db = kg.SnpsDataBase(base, [names[i] for i in pick])
    exp = _check_db(db, body, n_file, pick, Y, 2.0, topn)
    assert (exp[:, 1 << 20:] > 0).any()
    db.close()
