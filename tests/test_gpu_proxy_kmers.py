"""proxy_kmers, the tool, against proxy_np: the output's bytes and the log's per-lead lines must be the model's.

Two written tables of 31-mers, 600 rows over 70 accessions (67 in use) and 300 rows over 1140 (1135 in use), in families of
noisy copies so that proxies exist, with a complement and two constant rows. The accessions of -p are a reordered subset of the
table's, so the squeeze matters. KGWAS_PROXY_PIECE_ROWS and KGWAS_PROXY_RECORDS are set so that the pass crosses pieces and a
piece is drained in rounds."""
import os
import subprocess

import numpy as np
import pytest

import kmersgwas_amd as kg
from kmersgwas_amd import capi

import clump_np as CN
import lmm_table_np as T
import proxy_np as PN
from test_gpu_lmm_lrt_table import write_case

pytestmark = pytest.mark.gpu
BINDIR = os.path.join(os.path.dirname(os.path.abspath(capi.__file__)), "bin")
SHAPES = {67: (70, 600, 40), 1135: (1140, 300, 500)}  # accessions in use: (in the table, rows, in the subset of -p)
COMPLEMENT, ALL0, ALL1 = 77, 78, 79  # row 77 is the complement of row 70 over the accessions in use
LEAD_ROWS = (70, 5, 299, 78, 140, 0)  # the leads of most cases, in the leads file's order: row 78 is constant
HEAD9 = "chr\trs\tps\tn_miss\tallele1\tallele0\taf\tl_mle\tp_lrt\n"


def _run(cmd, rc=0, env=None):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, **(env or {})))
    assert r.returncode == rc, (r.returncode, r.stderr[-2000:])
    return r


@pytest.fixture(scope="module", params=sorted(SHAPES))
def case(request, tmp_path_factory):
    S = request.param
    S_F, n_rows, n_sub = SHAPES[S]
    d = tmp_path_factory.mktemp("proxy%d" % S)
    rng = np.random.default_rng(S)
    fams = n_rows // 10
    bits = np.repeat(rng.random((fams, S)) < rng.uniform(0.2, 0.8, fams)[:, None], 10, axis=0)
    bits ^= rng.random(bits.shape) < rng.choice([0.0, 0.01, 0.05], n_rows)[:, None]
    bits[COMPLEMENT], bits[ALL0], bits[ALL1] = ~bits[70], False, True
    pick = np.random.default_rng(4).permutation(S_F)[:S]
    rows = T.table_from_bits(bits, S_F, pick, 43)
    base, acc = write_case(d, rows, S_F, pick)
    ph = d / "pheno.tsv"
    ph.write_text("accession_id\tv\n" + "".join("%s\t%d\n" % (a, i) for i, a in enumerate(acc)))
    cols = np.random.default_rng(9).permutation(pick)[:n_sub]  # of the accessions in use, in another order than the table's and pick's
    sub = d / "subset.tsv"
    sub.write_text("accession_id\tv\n" + "".join("acc%d\t%d\n" % (c, i) for i, c in enumerate(cols)))
    return {"S": S, "S_F": S_F, "dir": d, "base": base, "rows": rows, "pheno": str(ph), "pick": pick, "subset": str(sub), "cols": cols}


def table_bits(case, cols):
    return CN.unpack_rows(case["rows"][:, 1:], case["S_F"])[:, np.asarray(cols)]


def expected(case, lead_rows, cols, tm, max_per_lead=100000):
    bits = table_bits(case, cols)
    texts = [T.kmer_text(case["rows"][r, 0]) for r in lead_rows]
    return PN.run(texts, bits[list(lead_rows)], case["rows"][:, 0], bits, tm, T.K_LEN, max_per_lead)


def leads_list(case, lead_rows, name="leads.txt"):
    path = case["dir"] / name
    path.write_text("".join(T.kmer_text(case["rows"][r, 0]) + "\n" for r in lead_rows))
    return str(path)


def proxy_kmers(case, leads, name, extra, rc=0, env=None):
    out = str(case["dir"] / name)
    r = _run([os.path.join(BINDIR, "proxy_kmers"), "--kmers_table", case["base"], "--kmers_len", str(T.K_LEN), "--leads", leads, "-o", out] + extra, rc, env)
    return out, r


def log_of(path):
    text = open(path + ".log.txt").read()
    per_lead = "".join(l + "\n" for l in text.split("\n") if l.startswith("lead\t")).encode()
    return per_lead, dict(l.split("\t", 1) for l in text.split("\n") if "\t" in l and not l.startswith("lead\t"))


@pytest.mark.parametrize("r2,piece,records", [("0.8", None, None), ("0.5", "128", None), ("0.05", "256", "100"), ("1", "128", "1"), ("0.000001", "256", "1000")])
def test_with_a_reordered_subset_of_the_accessions(case, r2, piece, records):
    tm = CN.millionths(r2)
    exp_out, exp_log, counts = expected(case, LEAD_ROWS, case["cols"], tm)
    found = sum(f for _, f in counts)
    if r2 == "0.8":
        assert counts[0][1] > 2 and counts[3] == (0, 0), "the fixture has no proxies to find, or its constant lead finds"
    env = dict(([("KGWAS_PROXY_PIECE_ROWS", piece)] if piece else []) + ([("KGWAS_PROXY_RECORDS", records)] if records else []))
    out, r = proxy_kmers(case, leads_list(case, LEAD_ROWS), "sub_%s.txt" % r2, ["-p", case["subset"], "--r2", r2], env=env)
    assert open(out, "rb").read() == exp_out
    per_lead, log = log_of(out)
    n_rows = len(case["rows"])
    assert per_lead == exp_log
    assert log["accessions"] == str(len(case["cols"])) and log["leads"] == str(len(LEAD_ROWS)) and log["rows_read"] == str(n_rows)
    assert log["pairs_tested"] == str(n_rows * len(LEAD_ROWS)) and log["proxies_found"] == log["proxies_kept"] == str(found)
    assert log["r2"] == "%.6f" % float(r2) and log["phenotypes"] == case["subset"] and log["max_per_lead"] == "100000"
    if records:  # every piece's records in rounds of at most `records`: at least as many rounds as that takes
        assert int(log["drain_rounds"]) >= -(-found // int(records)) and (found <= int(records) or int(log["drain_rounds"]) > 1)
    assert "[kgwas] proxy_kmers: " in r.stderr and " proxies_found=%d " % found in r.stderr
    # (stated on their own) a non-constant lead finds its own row with r2 1.000000 and +; the complement comes with -
    body = [l.split("\t") for l in open(out).read().split("\n")[1:-1]]
    own = [l for l in body if l[0] == l[1]]
    assert sorted(int(l[6]) for l in own) == sorted(set(LEAD_ROWS) - {ALL0}) and all(l[2] == "1.000000" and l[3] == "+" for l in own)
    comp = [l for l in body if l[0] == T.kmer_text(case["rows"][70, 0]) and int(l[6]) == COMPLEMENT]
    assert len(comp) == 1 and comp[0][2] == "1.000000" and comp[0][3] == "-" and comp[0][5] == "0"


def test_without_a_phenotype_file(case):
    exp_out, exp_log, _ = expected(case, LEAD_ROWS, np.arange(case["S_F"]), 800000)
    out, _ = proxy_kmers(case, leads_list(case, LEAD_ROWS), "all.txt", [], env={"KGWAS_PROXY_PIECE_ROWS": "256"})  # --r2 0.8 is the default
    assert open(out, "rb").read() == exp_out
    per_lead, log = log_of(out)
    assert per_lead == exp_log and log["accessions"] == str(case["S_F"])
    # the squeeze matters: over the subset the same leads find otherwise
    assert expected(case, LEAD_ROWS, case["cols"], 800000)[0] != exp_out
    # the accessions of lmm_lrt's phenotype file, all in use: the table's columns in pick's order
    exp_out, exp_log, _ = expected(case, LEAD_ROWS, case["pick"], 800000)
    out, _ = proxy_kmers(case, leads_list(case, LEAD_ROWS), "pick.txt", ["-p", case["pheno"]])
    assert open(out, "rb").read() == exp_out and log_of(out)[0] == exp_log and log_of(out)[1]["accessions"] == str(case["S"])


def test_popcount_ablation_writes_the_same_file(case):
    exp_out, exp_log, _ = expected(case, LEAD_ROWS, case["cols"], 500000)
    out, _ = proxy_kmers(case, leads_list(case, LEAD_ROWS), "popc.txt", ["-p", case["subset"], "--r2", "0.5"],
                         env={"KGWAS_LD_POPCOUNT": "1", "KGWAS_PROXY_PIECE_ROWS": "128"})
    assert open(out, "rb").read() == exp_out and log_of(out)[0] == exp_log


def test_a_clump_kmers_output_as_leads(case):
    """a real one: clump_kmers over a hand-written assoc file of 40 hits; its distinct leads, in clump order, are the leads"""
    rows = case["rows"]
    hit_rows = np.random.default_rng(11).permutation(len(rows))[:40]
    assoc = case["dir"] / "hits.assoc.txt"
    assoc.write_text(HEAD9 + "".join("0\t%s\t0\t0\t0\t1\t0.300\t1.000000e+00\t%.6e\n" % (T.kmer_text(rows[r, 0]), 10.0 ** -(3 + (7 * i) % 11))
                                     for i, r in enumerate(hit_rows)))
    clumps = str(case["dir"] / "clumps.txt")
    _run([os.path.join(BINDIR, "clump_kmers"), "--kmers_table", case["base"], "--kmers_len", str(T.K_LEN), "--assoc", str(assoc), "-p", case["subset"],
          "--r2", "0.5", "-o", clumps])
    lines = [l.split("\t") for l in open(clumps).read().split("\n")[1:-1]]
    by_clump = {}
    for l in lines:
        by_clump.setdefault(int(l[2]), l[3])
    lead_texts = [by_clump[c] for c in sorted(by_clump)]
    in_file_order = list(dict.fromkeys(l[3] for l in lines))
    assert 1 < len(lead_texts) < 40 and in_file_order != lead_texts, "the file's order is the clump order: the case shows nothing"
    lead_rows = [int(np.searchsorted(rows[:, 0], w)) for w in T.kmer_words(lead_texts)]
    exp_out, exp_log, _ = expected(case, lead_rows, case["cols"], 800000)
    out, _ = proxy_kmers(case, clumps, "from_clumps.txt", ["-p", case["subset"]], env={"KGWAS_PROXY_PIECE_ROWS": "128"})
    assert open(out, "rb").read() == exp_out and log_of(out)[0] == exp_log


def test_max_per_lead(case):
    exp_out, exp_log, counts = expected(case, LEAD_ROWS, case["cols"], 500000, max_per_lead=3)
    assert any(kept == 3 and found > 3 for kept, found in counts), "the fixture has no lead whose kept and found counts differ"
    out, _ = proxy_kmers(case, leads_list(case, LEAD_ROWS), "max3.txt", ["-p", case["subset"], "--r2", "0.5", "--max_per_lead", "3"],
                         env={"KGWAS_PROXY_PIECE_ROWS": "128", "KGWAS_PROXY_RECORDS": "7"})
    assert open(out, "rb").read() == exp_out
    per_lead, log = log_of(out)
    assert per_lead == exp_log and log["max_per_lead"] == "3"
    assert log["proxies_kept"] == str(sum(k for k, _ in counts)) and log["proxies_found"] == str(sum(f for _, f in counts))


def test_a_lead_the_table_lacks(case):
    rows = case["rows"]
    absent = int(rows[10, 0]) + 1
    assert absent not in set(rows[:, 0].tolist())
    leads = case["dir"] / "absent.txt"
    leads.write_text(T.kmer_text(rows[7, 0]) + "\n" + T.kmer_text(absent) + "\n" + T.kmer_text(rows[200, 0]) + "\n")
    out, r = proxy_kmers(case, str(leads), "absent_out.txt", ["-p", case["subset"]], rc=1)
    assert "the k-mer %s of %s is not in the table" % (T.kmer_text(absent), leads) in r.stderr, r.stderr
    assert not os.path.exists(out) and not os.path.exists(out + ".log.txt")


def test_the_links_among_the_hits_are_kmers_ld_s(case):
    """every hit of an assoc file as leads: among the hits' rows the pairs proxy_kmers links are the bits kgwas_kmers_ld gives"""
    rows = case["rows"]
    hit_rows = np.sort(np.random.default_rng(12).permutation(len(rows))[:50])
    assoc = case["dir"] / "hits50.assoc.txt"
    assoc.write_text(HEAD9 + "".join("0\t%s\t0\t0\t0\t1\t0.300\t1.000000e+00\t1e-5\n" % T.kmer_text(rows[r, 0]) for r in hit_rows))
    rs = [l.split("\t")[1] for l in open(assoc).read().split("\n")[1:-1]]
    leads = case["dir"] / "hits50.txt"
    leads.write_text("".join(k + "\n" for k in rs))
    out, _ = proxy_kmers(case, str(leads), "hits50_out.txt", ["-p", case["subset"], "--r2", "0.5"], env={"KGWAS_PROXY_PIECE_ROWS": "256"})
    place = {int(r): i for i, r in enumerate(hit_rows)}
    lead_no = {k: i for i, k in enumerate(rs)}
    got = {(lead_no[l[0]], place[int(l[6])]) for l in (x.split("\t") for x in open(out).read().split("\n")[1:-1]) if int(l[6]) in place}
    bits = table_bits(case, case["cols"])[hit_rows]
    adj, n1 = kg.kmers_ld(CN.pack_rows(bits), bits.shape[1], "0.5")
    upper = {(a, b) for a in range(50) for b in range(a + 1, 50) if CN.adj_bit(adj, a, b)}
    want = upper | {(b, a) for a, b in upper} | {(a, a) for a in range(50) if 0 < n1[a] < bits.shape[1]}
    assert got == want and len(upper) > 10
