"""clump_kmers, the tool, against clump_np: the output's bytes must be the model's.

One table of 300 rows over 70 accessions, in families of noisy copies so that clumps exist, is shared by the cases: the assoc file
is lmm_lrt's own (--kmers_table --best 50, 9 columns; -bfile -lmm 4, 14 columns) or written by hand where the case needs chosen
p-values. The accessions of -p are a reordered subset of the table's, so the squeeze matters."""
import os
import subprocess

import numpy as np
import pytest

import kmersgwas_amd as kg
from kmersgwas_amd import capi

import clump_np as CN
import lmm_table_np as T
from test_gpu_lmm_lrt_table import write_case

pytestmark = pytest.mark.gpu
BINDIR = os.path.join(os.path.dirname(os.path.abspath(capi.__file__)), "bin")
S, S_F, N_ROWS = 67, 70, 300
TWIN_A, TWIN_B = 120, 45  # two rows with one pattern over ALL accessions of the table; the later row comes first in the hand-written file
HEAD9 = "chr\trs\tps\tn_miss\tallele1\tallele0\taf\tl_mle\tp_lrt\n"


def _run(cmd, rc=0):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == rc, (r.returncode, r.stderr[-2000:])
    return r


def _log(path):
    return dict(l.split("\t", 1) for l in open(path).read().split("\n") if "\t" in l)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("clump")
    rng = np.random.default_rng(2024)
    base_rows = rng.random((30, S)) < rng.uniform(0.2, 0.8, 30)[:, None]
    bits = np.repeat(base_rows, 10, axis=0)  # phenotype order of lmm_lrt's run
    bits ^= rng.random(bits.shape) < rng.choice([0.0, 0.01, 0.05], N_ROWS)[:, None]
    pick = np.random.default_rng(4).permutation(S_F)[:S]
    rows = T.table_from_bits(bits, S_F, pick, 41)
    rows[TWIN_B, 1:] = rows[TWIN_A, 1:]
    base, acc = write_case(d, rows, S_F, pick)
    K, y = T.kinship_and_phenotype(S)
    ph = d / "pheno.tsv"
    ph.write_text("accession_id\tv\n" + "".join("%s\t%r\n" % (a, float(v)) for a, v in zip(acc, y)))
    kin = d / "pheno.kinship"
    kin.write_text("\n".join("\t".join("%.17g" % v for v in r) for r in K) + "\n")
    out = str(d / "out")
    _run([os.path.join(BINDIR, "lmm_lrt"), "--kmers_table", base, "--kmers_len", str(T.K_LEN), "-p", str(ph), "-lmm", "2", "-k", str(kin),
          "-outdir", out, "-o", "best", "--mac", "5", "-maf", "0.05", "--best", "50"])
    # the accessions r2 is taken over: 40 of the table's 70, in another order than the table's and than lmm_lrt's
    cols = np.random.default_rng(9).permutation(S_F)[:40]
    sub = d / "subset.tsv"
    sub.write_text("accession_id\tv\n" + "".join("acc%d\t%d\n" % (c, i) for i, c in enumerate(cols)))
    return {"dir": d, "base": base, "rows": rows, "pheno": str(ph), "kin": str(kin), "acc": acc, "y": y, "out": out,
            "best": os.path.join(out, "best.assoc.txt"), "subset": str(sub), "cols": cols}


def read_assoc(path):
    lines = [l.split("\t") for l in open(path).read().split("\n") if l]
    i_rs, i_p = lines[0].index("rs"), lines[0].index("p_lrt")
    return [l[i_rs] for l in lines[1:]], [l[i_p] for l in lines[1:]]


def expected(case, assoc, cols, tm, p_max=float("inf")):
    """the model's bytes for an assoc file, over the table's columns `cols`; also (hits used, clumps)"""
    rs, p = read_assoc(assoc)
    rows = case["rows"]
    idx = np.searchsorted(rows[:, 0], T.kmer_words(rs))
    assert (rows[idx, 0] == T.kmer_words(rs)).all()
    bits = CN.unpack_rows(rows[idx, 1:], S_F)[:, np.asarray(cols)]
    text = CN.run(rs, p, bits, tm, p_max)
    body = [l.split("\t") for l in text.decode().split("\n")[1:-1]]
    return text, len(body), len({l[2] for l in body})


def clump_kmers(case, assoc, name, extra, rc=0):
    out = str(case["dir"] / name)
    r = _run([os.path.join(BINDIR, "clump_kmers"), "--kmers_table", case["base"], "--kmers_len", str(T.K_LEN), "--assoc", assoc, "-o", out] + extra, rc)
    return out, r


@pytest.mark.parametrize("r2,tile_rows", [("0.8", None), ("0.5", "64"), ("0.05", None), ("1", None)])
def test_with_a_reordered_subset_of_the_accessions(case, r2, tile_rows):
    exp, used, clumps = expected(case, case["best"], case["cols"], CN.millionths(r2))
    assert used == 50
    if r2 in ("0.8", "0.5"):
        assert 1 < clumps < 50, "the fixture has no clumps to find"
    out, r = clump_kmers(case, case["best"], "sub_%s.txt" % r2, ["-p", case["subset"], "--r2", r2] + (["--tile_rows", tile_rows] if tile_rows else []))
    assert open(out, "rb").read() == exp
    log = _log(out + ".log.txt")
    assert log["hits_read"] == "50" and log["hits_used"] == "50" and log["clumps"] == str(clumps) and log["accessions"] == "40"
    assert log["r2"] == "%.6f" % float(r2) and log["assoc"] == case["best"] and log["phenotypes"] == case["subset"]
    assert "[kgwas] clump_kmers: " in r.stderr and " clumps=%d " % clumps in r.stderr


def test_without_a_phenotype_file(case):
    exp, used, clumps = expected(case, case["best"], np.arange(S_F), 800000)
    out, _ = clump_kmers(case, case["best"], "all.txt", [])  # --r2 0.8 is the default
    assert open(out, "rb").read() == exp
    assert _log(out + ".log.txt")["accessions"] == str(S_F) and _log(out + ".log.txt")["clumps"] == str(clumps)
    # the squeeze matters: over the subset the same hits clump otherwise
    assert expected(case, case["best"], case["cols"], 800000)[0] != exp


def test_p_max_drops_hits(case):
    _, p = read_assoc(case["best"])
    cut = sorted(p, key=float)[19]  # the 20th smallest p, as the file spells it: hits that tie with it stay
    exp, used, clumps = expected(case, case["best"], case["cols"], 500000, float(cut))
    assert 20 <= used < 50
    out, _ = clump_kmers(case, case["best"], "cut.txt", ["-p", case["subset"], "--r2", "0.5", "--p_max", cut])
    assert open(out, "rb").read() == exp
    log = _log(out + ".log.txt")
    assert log["hits_read"] == "50" and log["hits_used"] == str(used) and log["clumps"] == str(clumps)


def hand_written(case, name, entries):
    path = case["dir"] / name
    path.write_text(HEAD9 + "".join("0\t%s\t0\t0\t0\t1\t0.300\t1.000000e+00\t%s\n" % (T.kmer_text(w), p) for w, p in entries))
    return str(path)


def test_equal_p_file_order_decides_the_lead(case):
    rows = case["rows"]
    entries = [(rows[7, 0], "2.5e-06"), (rows[TWIN_A, 0], "1.000000e-09"), (rows[200, 0], "0.01"), (rows[TWIN_B, 0], "1.000000e-09"),
               (rows[121, 0], "3e-4")]
    assoc = hand_written(case, "twins.assoc.txt", entries)
    for extra, cols in ((["-p", case["subset"]], case["cols"]), ([], np.arange(S_F))):
        exp, used, _ = expected(case, assoc, cols, 1000000)
        out, _ = clump_kmers(case, assoc, "twins.txt", ["--r2", "1"] + extra)
        got = open(out, "rb").read()
        assert got == exp and used == 5
        lines = [l.split("\t") for l in got.decode().split("\n")[1:-1]]
        a, b = lines[1], lines[3]
        assert a[0] == T.kmer_text(rows[TWIN_A, 0]) and b[0] == T.kmer_text(rows[TWIN_B, 0])
        assert a[2] == b[2] == "1" and a[3] == b[3] == a[0], "the earlier of two equal p does not lead"
        assert a[4] == b[4] == "1.000000" and a[5] == b[5] == a[6] == b[6]


def test_a_hit_the_table_lacks(case):
    rows = case["rows"]
    absent = int(rows[10, 0]) + 1
    assert absent not in set(rows[:, 0].tolist())
    assoc = hand_written(case, "absent.assoc.txt", [(rows[7, 0], "2.5e-06"), (absent, "1e-7"), (rows[200, 0], "0.01")])
    out, r = clump_kmers(case, assoc, "absent.txt", ["-p", case["subset"]], rc=1)
    assert "the k-mer %s of %s is not in the table" % (T.kmer_text(absent), assoc) in r.stderr, r.stderr
    assert not os.path.exists(out) and not os.path.exists(out + ".log.txt")


def test_the_14_column_file_of_the_bed_route(case):
    plink = str(case["dir"] / "plink")
    _run([os.path.join(BINDIR, "kmers_table_to_bed"), "-t", case["base"], "-k", str(T.K_LEN), "-p", case["pheno"], "--maf", "0.05", "--mac", "5",
          "-b", "100000", "-o", plink])
    _run([os.path.join(BINDIR, "lmm_lrt"), "-bfile", plink + ".0", "-lmm", "4", "-k", case["kin"], "-outdir", case["out"], "-o", "wald", "-maf", "0.05"])
    assoc = os.path.join(case["out"], "wald.assoc.txt")
    head = open(assoc).readline().rstrip("\n").split("\t")
    assert len(head) == 14 and head.index("p_lrt") == 12 and head.index("rs") == 1
    rs, p = read_assoc(assoc)
    assert len(rs) > 100
    cut = sorted(p, key=float)[79]
    exp, used, clumps = expected(case, assoc, case["cols"], 800000, float(cut))
    assert used >= 80 and 1 < clumps < used
    out, _ = clump_kmers(case, assoc, "wald.txt", ["-p", case["subset"], "--p_max", cut])
    assert open(out, "rb").read() == exp
    assert _log(out + ".log.txt")["hits_read"] == str(len(rs))


def test_python_mirror(case):
    words = np.ascontiguousarray(case["rows"][:, 1:])
    adj, n1 = kg.kmers_ld(words, S_F, 0.8, tile_rows=128)
    exp_adj, exp_n1 = CN.links(words, S_F, 800000)
    assert adj.dtype == np.uint32 and adj.shape == (N_ROWS, 10) and n1.dtype == np.uint32
    assert adj.tobytes() == exp_adj.tobytes() and n1.tobytes() == exp_n1.tobytes()
    assert exp_adj.any()
