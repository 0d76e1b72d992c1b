"""kmers_table_to_bed (bed_kernels.hip, table_to_bed.cpp) across pieces and panel widths, and the squeeze kernel's width limit.

Every case writes the oracle's files (oracle.cpp, orc_table_to_bed) and compares the library's and the tool's, byte for byte.
KGWAS_BED_PIECE_ROWS cuts the table into small pieces, so the second host buffer set, the reader / writer handshake and
batches that span pieces run; one case uses the default piece of 2^20 rows. Panel widths cover the three launch forms of
bed_rowinfo_kernel (static LDS up to 1920 phenotyped accessions, dynamic LDS from 1921, half blocks from 4737, quarter
blocks from 9473) up to 10 176, the squeeze kernel's limit."""
import os
import subprocess

import numpy as np
import pytest

import kmersgwas_amd as kg
from oracle import binding as ob
from oracle import oracle_np as onp
from helpers import random_table, phenotypes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "kmersgwas_amd", "bin")
K = 31


def _listing(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


def _run(tmp_path, rows, S_f, pick, batch, unique, maf="0.05", mac="5", cli=True):
    """Oracle, library and (cli) tool on the same table and phenotype file; returns (batches, written)."""
    names = ["acc%d" % i for i in range(S_f)]
    base = str(tmp_path / "tab")
    onp.write_table(base, names, K, rows[:, 0], rows[:, 1:])
    acc = [names[i] for i in pick]
    y = phenotypes(len(pick), 0, seed=len(pick))[0]
    ph = tmp_path / "ph.tsv"
    with open(ph, "w") as f:
        f.write("accession_id\tphenotype_value\n" + "".join("%s\t%r\n" % (a, float(v)) for a, v in zip(acc, y)))
    _, acc2, Y2 = onp.load_phenotypes(str(ph))
    col = onp.column_map(names, acc2)
    mc = max(int(np.ceil(len(pick) * float(maf))), int(mac))
    out_o, out_l, out_p = tmp_path / "orc", tmp_path / "lib", tmp_path / "cli"
    for d in (out_o, out_l, out_p):
        d.mkdir()
    nb, nw = ob.table_to_bed(str(out_o / "x"), rows, S_f, col, acc2, Y2[0], K, mc, batch, unique)
    exp = _listing(str(out_o))
    assert len(exp) == 3 * nb
    tbl = kg.KmersTable(base, K)
    assert kg.table_to_bed(str(out_l / "x"), tbl, col, acc2, Y2[0], mc, batch, unique) == (nb, nw)
    tbl.close()
    got = _listing(str(out_l))
    assert sorted(got) == sorted(exp)
    for f in exp:
        assert got[f] == exp[f], "library: %s differs" % f
    if cli:
        cmd = [os.path.join(BIN, "kmers_table_to_bed"), "-t", base, "-k", str(K), "-p", str(ph), "--maf", maf, "--mac", mac,
               "-b", str(batch), "-o", str(out_p / "x")] + (["-u"] if unique else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        got = _listing(str(out_p))
        assert sorted(got) == sorted(exp)
        for f in exp:
            assert got[f] == exp[f], "tool: %s differs" % f
    return nb, nw


# ---- pieces -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unique", [False, True])
def test_many_pieces_ragged_tail_and_an_empty_piece(tmp_path, monkeypatch, unique):
    """Pieces of 1000 rows over 10 007 (a ragged last piece), one piece in which no row passes the MAC filter, -u duplicates
    whose first occurrence sits pieces earlier, batches of 777 kept rows that span pieces."""
    monkeypatch.setenv("KGWAS_BED_PIECE_ROWS", "1000")
    S_f = 150
    rows = random_table(10_007, S_f, seed=41, dup_frac=0.3)
    rows[4000:5000, 1:] = 0                 # piece 4: nothing kept
    rows[[7500, 9999, 10_006], 1:] = rows[12, 1:]  # patterns first seen in piece 0
    pick = np.random.default_rng(2).permutation(S_f)[:131]
    nb, nw = _run(tmp_path, rows, S_f, pick, 777, unique)
    assert nb > 5


def test_batch_ends_on_a_piece_boundary(tmp_path, monkeypatch):
    """Every row passes the MAC filter and batches are as long as pieces: each batch closes on a piece's last row, and the
    next piece opens the next batch."""
    monkeypatch.setenv("KGWAS_BED_PIECE_ROWS", "1024")
    S_f = 100
    rows = random_table(5 * 1024, S_f, seed=42, freq_lo=0.3, freq_hi=0.7)
    nb, nw = _run(tmp_path, rows, S_f, np.arange(S_f)[::-1], 1024, False)
    assert (nb, nw) == (5, 5 * 1024)


def test_batch_size_one(tmp_path, monkeypatch):
    """One kept k-mer per batch (and -u), pieces of 64 rows."""
    monkeypatch.setenv("KGWAS_BED_PIECE_ROWS", "64")
    S_f = 70
    rows = random_table(301, S_f, seed=43, dup_frac=0.3)
    rows[100:140, 1:] = 0
    nb, nw = _run(tmp_path, rows, S_f, np.random.default_rng(4).permutation(S_f)[:65], 1, True)
    assert nb > 150


def test_default_piece_over_a_million_rows(tmp_path, monkeypatch):
    """More than 2^20 rows at the default piece size (no hook): the second piece uses the second host buffer set."""
    monkeypatch.delenv("KGWAS_BED_PIECE_ROWS", raising=False)
    S_f = 40
    rows = random_table((1 << 20) + 4321, S_f, seed=44, dup_frac=0.2)
    nb, nw = _run(tmp_path, rows, S_f, np.random.default_rng(5).permutation(S_f)[:37], 400_000, True)
    assert nb >= 1 and nw > 0


# ---- panel widths -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S_f", [1, 2, 3, 4, 5, 1920, 1921, 4736, 4737, 9472, 9473, 10176])
def test_panel_widths(tmp_path, monkeypatch, S_f):
    """All of the table phenotyped, in shuffled order, from 1 accession (MAC 0) to 10 176 (the squeeze kernel's limit)."""
    monkeypatch.setenv("KGWAS_BED_PIECE_ROWS", "500")
    n_rows = 1200 if S_f < 4000 else 700
    rows = random_table(n_rows, S_f, seed=S_f, dup_frac=0.2)
    tiny = S_f <= 5
    nb, nw = _run(tmp_path, rows, S_f, np.random.default_rng(S_f).permutation(S_f), 301, S_f % 2 == 1,
                  maf="0" if tiny else "0.05", mac="0" if tiny else "5", cli=S_f in (1, 4, 1921, 10176))
    assert nw > 0


# ---- the squeeze kernel's width limit -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("S_f,n_pick", [(10_177, 10_177), (20_289, 1)])
def test_squeeze_limit_refused_before_any_output(tmp_path, S_f, n_pick):
    """One accession past the limit (all phenotyped, or a single phenotyped accession of a wider table): a clean
    KGWAS_ERR_ARG naming the limit from the library and status 1 from the tool, and no output file."""
    names = ["acc%d" % i for i in range(S_f)]
    base = str(tmp_path / "tab")
    rows = random_table(50, S_f, seed=3)
    onp.write_table(base, names, K, rows[:, 0], rows[:, 1:])
    pick = np.random.default_rng(1).permutation(S_f)[:n_pick]
    acc = [names[i] for i in pick]
    y = phenotypes(n_pick, 0, seed=1)[0]
    out = tmp_path / "out"
    out.mkdir()
    tbl = kg.KmersTable(base, K)
    with pytest.raises(kg.KgwasError) as e:
        kg.table_to_bed(str(out / "x"), tbl, pick.astype(np.uint64), acc, y, 0, 100, False)
    tbl.close()
    assert e.value.code == kg.capi.KGWAS_ERR_ARG and "10176" in e.value.msg and "20288" in e.value.msg, e.value
    ph = tmp_path / "ph.tsv"
    with open(ph, "w") as f:
        f.write("accession_id\tphenotype_value\n" + "".join("%s\t%r\n" % (a, float(v)) for a, v in zip(acc, y)))
    r = subprocess.run([os.path.join(BIN, "kmers_table_to_bed"), "-t", base, "-k", str(K), "-p", str(ph), "--maf", "0",
                        "--mac", "0", "-b", "100", "-o", str(out / "y")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "squeeze" in r.stderr, r.stderr[-2000:]
    assert os.listdir(out) == []


def test_squeeze_limit_subset_of_the_widest_table(tmp_path, monkeypatch):
    """The widest table a subset may come from (20 288 accessions), one phenotyped accession per 64-bit word: exact files."""
    monkeypatch.setenv("KGWAS_BED_PIECE_ROWS", "300")
    S_f = 20_288
    rows = random_table(700, S_f, seed=7)
    pick = np.random.default_rng(7).permutation(S_f)[:100]
    _run(tmp_path, rows, S_f, pick, 250, True, cli=False)


@pytest.mark.parametrize("S_f", [10_176, 10_177])
def test_squeeze_limit_of_a_reordered_scan_session(S_f):
    """A scan session over a reordered panel squeezes its rows: the largest accepted panel gives the oracle's top-N, one
    accession more is refused by kgwas_scan_create, not by the first feed."""
    rng = np.random.default_rng(S_f)
    col = rng.permutation(S_f).astype(np.uint64)
    Y = phenotypes(S_f, 1, seed=S_f)
    mac = onp.min_count(S_f, 0.05, 5)
    if S_f > 10_176:
        with pytest.raises(kg.KgwasError) as e:
            kg.AssociationScan(S_f, col, Y, 50, mac)
        assert e.value.code == kg.capi.KGWAS_ERR_ARG and "kgwas_scan_create" in e.value.msg and "10176" in e.value.msg
        return
    rows = random_table(3000, S_f, seed=S_f)
    exp = ob.associate(rows, S_f, col, Y, 50, mac)
    scan = kg.AssociationScan(S_f, col, Y, 50, mac, chunk_rows=1024)
    scan.feed_host(rows)
    scan.finish()
    for j in range(2):
        k, s, r = scan.result(j)
        o = exp["per_pheno"][j]
        assert (k == o["kmer"]).all() and (r == o["file_row"]).all() and s.tobytes() == o["score"].tobytes()
    assert scan.stats()["rows_tested"] == exp["tested"]
    scan.close()
