"""clump_kmers and proxy_kmers where the squeezed row gains a word: 127, 128 and 129 accessions in use, a reordered subset of a
table's 130. At 128 -> 129 the squeeze's padded column map and output row grow by a 128-bit unit (W_m 2 -> 4) while the r2
operands keep one chunk group of 512, so the squeeze's padding and the operands' padding meet here. The outputs' bytes must be
the models' (clump_np, proxy_np).

One table of 300 rows over 130 accessions, in families of noisy copies so that clumps and proxies exist, is shared by all cases."""
import os
import subprocess

import numpy as np
import pytest

from kmersgwas_amd import capi

import clump_np as CN
import lmm_table_np as T
import proxy_np as PN
from test_gpu_lmm_lrt_table import write_case

pytestmark = pytest.mark.gpu
BINDIR = os.path.join(os.path.dirname(os.path.abspath(capi.__file__)), "bin")
S_F, N_ROWS, N_HITS = 130, 300, 70
LEAD_ROWS = (70, 5, 299)
HEAD9 = "chr\trs\tps\tn_miss\tallele1\tallele0\taf\tl_mle\tp_lrt\n"


def _run(cmd, env=None):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    d = tmp_path_factory.mktemp("ld128")
    rng = np.random.default_rng(128)
    bits = np.repeat(rng.random((N_ROWS // 10, S_F)) < rng.uniform(0.2, 0.8, N_ROWS // 10)[:, None], 10, axis=0)
    bits ^= rng.random(bits.shape) < rng.choice([0.0, 0.01, 0.05], N_ROWS)[:, None]
    rows = T.table_from_bits(bits, S_F, np.arange(S_F), 47)
    base, _ = write_case(d, rows, S_F, np.arange(S_F))
    hit_rows = np.random.default_rng(13).permutation(N_ROWS)[:N_HITS]
    assoc = d / "hits.assoc.txt"
    assoc.write_text(HEAD9 + "".join("0\t%s\t0\t0\t0\t1\t0.300\t1.000000e+00\t%.6e\n" % (T.kmer_text(rows[r, 0]), 10.0 ** -(3 + (7 * i) % 11))
                                     for i, r in enumerate(hit_rows)))
    leads = d / "leads.txt"
    leads.write_text("".join(T.kmer_text(rows[r, 0]) + "\n" for r in LEAD_ROWS))
    return {"dir": d, "base": base, "rows": rows, "bits": bits, "hit_rows": hit_rows, "assoc": str(assoc), "leads": str(leads)}


@pytest.fixture(params=[127, 128, 129])
def subset(request, table):
    """S of the table's accessions, in another order than the table's"""
    S = request.param
    cols = np.random.default_rng(S).permutation(S_F)[:S]
    assert (np.sort(cols) != cols).any()
    ph = table["dir"] / ("subset%d.tsv" % S)
    ph.write_text("accession_id\tv\n" + "".join("acc%d\t%d\n" % (c, i) for i, c in enumerate(cols)))
    return S, cols, str(ph)


def test_clump_kmers(table, subset):
    S, cols, ph = subset
    lines = [l.split("\t") for l in open(table["assoc"]).read().split("\n")[1:] if l]
    exp = CN.run([l[1] for l in lines], [l[8] for l in lines], table["bits"][table["hit_rows"]][:, cols], 500000)
    clumps = {l.split("\t")[2] for l in exp.decode().split("\n")[1:-1]}
    assert 1 < len(clumps) < N_HITS, "the fixture has no clumps to find"
    out = str(table["dir"] / ("clumps%d.txt" % S))
    _run([os.path.join(BINDIR, "clump_kmers"), "--kmers_table", table["base"], "--kmers_len", str(T.K_LEN), "--assoc", table["assoc"], "-p", ph,
          "--r2", "0.5", "-o", out])
    assert open(out, "rb").read() == exp
    log = dict(l.split("\t", 1) for l in open(out + ".log.txt").read().split("\n") if "\t" in l)
    assert log["accessions"] == str(S) and log["hits_used"] == str(N_HITS) and log["clumps"] == str(len(clumps))


def test_proxy_kmers(table, subset):
    """pieces of 128 rows: 300 rows end in a partial piece of 44"""
    S, cols, ph = subset
    bits = table["bits"][:, cols]
    texts = [T.kmer_text(table["rows"][r, 0]) for r in LEAD_ROWS]
    exp_out, exp_log, counts = PN.run(texts, bits[list(LEAD_ROWS)], table["rows"][:, 0], bits, 500000, T.K_LEN)
    assert all(found > 1 for _, found in counts), "the fixture has a lead without proxies"
    out = str(table["dir"] / ("proxies%d.txt" % S))
    _run([os.path.join(BINDIR, "proxy_kmers"), "--kmers_table", table["base"], "--kmers_len", str(T.K_LEN), "--leads", table["leads"], "-p", ph,
          "--r2", "0.5", "-o", out], env={"KGWAS_PROXY_PIECE_ROWS": "128"})
    assert open(out, "rb").read() == exp_out
    text = open(out + ".log.txt").read()
    assert "".join(l + "\n" for l in text.split("\n") if l.startswith("lead\t")).encode() == exp_log
    log = dict(l.split("\t", 1) for l in text.split("\n") if "\t" in l and not l.startswith("lead\t"))
    assert log["accessions"] == str(S) and log["rows_read"] == str(N_ROWS) and log["proxies_found"] == str(sum(f for _, f in counts))
