"""lmm_lrt --kmers_table at the sizes its defaults run at (lmm_table.cpp, lmm_table_kernels.hip): pieces of more than 65 536
rows, so that lmm_table_scan_kernel carries its total over rounds of 256 blocks; more tested rows in a piece than a chunk of 10 240
and of 65 536 variants; select launches of more than 65 536 (column, row) pairs with open and with closed heaps; panels of 256 to
1135 accessions.

The yardsticks are those of test_gpu_lmm_lrt_table.py and test_gpu_lmm_lrt_table_multi.py: the .bed route (kgwas_table_to_bed in
one batch, then kgwas_lmm_test_bed), T.tested_rule for the row set, one test_table call per column for the multi route. Doubles are
compared by their raw bytes; there is no tolerance in this module. The geometry of its fixtures (blocks and rounds per piece and
per select launch) is asserted without a GPU in test_lmm_lrt_table_cli.py."""
import numpy as np
import pytest

import kmersgwas_amd as kg

import lmm_table_np as T
from test_gpu_lmm_lrt_table import FIELDS, assert_same, bed_route, edges_case, table_route, write_case
from test_gpu_lmm_lrt_table_multi import Case, columns, same_column, set_piece

pytestmark = pytest.mark.gpu
S, S_F, MC, MAF = T.SCALE_S, T.SCALE_S_F, T.SCALE_MIN_COUNT, T.SCALE_MAF


def rounds_of(flags, piece):
    """per piece (launch) the number of scan rounds and of blocks, for the printed record"""
    return ["%d rounds / %d blocks" % (len(p), sum(len(r) for r in p)) for p in T.scan_geometry(flags, piece)]


# ---- 2. the front end: pieces beyond 65 536 rows -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def block_table(tmp_path_factory):
    """The block-structured table on disk and its .bed route, computed once for every piece size."""
    d = tmp_path_factory.mktemp("blocks")
    bits, pick, rows, rule = T.scale_fixture()
    K, y = T.kinship_and_phenotype(S)
    base, acc = write_case(d, rows, S_F, pick)
    rows_exp, exp = bed_route(d, base, rows, pick, acc, K, y, MC, MAF)
    return base, K, y, rows_exp, exp


@pytest.mark.parametrize("piece", T.SCALE_PIECES)
def test_pieces_beyond_one_scan_round(block_table, monkeypatch, piece):
    base, K, y, rows_exp, exp = block_table
    bits, pick, rows, rule = T.scale_fixture()
    n_rows, want = T.SCALE_ROWS, np.flatnonzero(rule)
    assert rows_exp.tolist() == want.tolist(), "the .bed route tests other rows than the numpy rule"
    set_piece(monkeypatch, piece)
    res = table_route(base, pick, K, y, MC, MAF, n_rows, 10240)
    print("piece %s: %d of %d rows tested; front end %s" % (piece, len(want), n_rows, rounds_of(rule, T.piece_rows(n_rows, piece, rows.shape[1]))))
    got = res["row"].astype(np.int64)
    assert len(got) == len(want) and (np.diff(got) > 0).all(), "rows missing, repeated or out of order"
    assert res["row"].tolist() == want.tolist()
    assert res["kmer"].tobytes() == rows[want, 0].tobytes()
    assert res["af"].tobytes() == T.af_of(bits[want].sum(axis=1), S).tobytes()
    assert res["rows_read"] == n_rows and res["rows_tested"] == len(want)
    assert res["stats"]["variants_read"] == n_rows and res["stats"]["variants_tested"] == len(want)
    assert_same(res, rows_exp, exp, "piece %s" % piece)


# ---- 3. sub-chunks at real chunk sizes -----------------------------------------------------------------------------------------
def test_sub_chunks_at_real_chunk_sizes(tmp_path, monkeypatch):
    monkeypatch.delenv("KGWAS_LMM_PIECE_ROWS", raising=False)
    n_rows = T.CHUNK_ROWS
    bits = T.scale_bits(n_rows)
    K, y = T.kinship_and_phenotype(S)
    pick = np.random.default_rng(3).permutation(S_F)[:S]
    rows = T.table_from_bits(bits, S_F, pick, 3)
    base, acc = write_case(tmp_path, rows, S_F, pick)
    rule = T.scale_tested(bits)
    tested = int(rule.sum())
    assert tested >= T.CHUNK_MIN_TESTED and T.piece_rows(n_rows, None, rows.shape[1]) == n_rows, "not one piece of 25 000 tested rows"
    rows_exp, exp = bed_route(tmp_path, base, rows, pick, acc, K, y, MC, MAF, chunk=10240)
    assert rows_exp.tolist() == np.flatnonzero(rule).tolist()
    # a variant's numbers do not depend on its batch: the .bed route itself in batches of 10 240 and in one
    rows_one, one = bed_route(tmp_path, base, rows, pick, acc, K, y, MC, MAF, chunk=65536)
    assert rows_one.tolist() == rows_exp.tolist()
    for k in FIELDS:
        assert one[k].tobytes() == exp[k].tobytes(), "the .bed route: %s depends on chunk_variants" % k
    for chunk, chunks in ((10240, -(-tested // 10240)), (65536, 1), (100000, 1)):
        res = table_route(base, pick, K, y, MC, MAF, n_rows, chunk)
        print("chunk_variants %d: %d tested rows in %d sub-chunks" % (chunk, tested, res["stats"]["chunks"]))
        assert_same(res, rows_exp, exp, "chunk %d" % chunk)
        assert res["kmer"].tobytes() == rows[rule, 0].tobytes()
        assert res["stats"]["chunks"] == chunks and res["rows_tested"] == tested
    assert -(-tested // 10240) == 3 and tested % 10240, "the default chunk does not give three sub-chunks with a partial last one"


# ---- 4. the select stage: more than 65 536 pairs per launch --------------------------------------------------------------------
P = 33  # a block of 32 columns and a block of 1


def select_case(d, n_rows, ties=False):
    bits = T.scale_bits(n_rows, ties)
    K, y = T.kinship_and_phenotype(S)
    pick = np.random.default_rng(S_F).permutation(S_F)[:S]
    rows = T.table_from_bits(bits, S_F, pick, S)
    c = Case(d, rows, S_F, pick, K, columns(y, P), MC, MAF)
    c.rule = T.scale_tested(bits)
    c.tested = int(c.rule.sum())
    return c


def test_select_open_heaps_beyond_one_scan_round(tmp_path, monkeypatch):
    set_piece(monkeypatch, None)
    monkeypatch.delenv("KGWAS_LMM_TABLE_SELECT", raising=False)
    n_rows = T.SELECT_OPEN_ROWS
    c = select_case(tmp_path, n_rows)
    try:
        assert c.tested >= T.SELECT_OPEN_MIN_TESTED and 32 * c.tested > 65536 and c.tested <= 10240
        print("%d tested rows: select launch of %s" % (c.tested, rounds_of(np.ones(32 * c.tested, bool), 32 * c.tested)))
        res = c.multi(range(P), n_rows, 10240)
        assert res["rows_read"] == n_rows and res["rows_tested"] == c.tested
        assert res["pairs_shipped"] == c.tested * P, "a pair was dropped although no heap was full"
        for k in range(P):
            same_column(res["columns"][k], c.single(k, n_rows), "column %d" % k)
            assert res["columns"][k]["row"].tolist() == np.flatnonzero(c.rule).tolist()
    finally:
        c.close()


@pytest.fixture(scope="module")
def closed_case(tmp_path_factory):
    c = select_case(tmp_path_factory.mktemp("closed"), T.SELECT_ROWS)
    yield c
    c.close()


@pytest.mark.parametrize("best_n", [1, 7, 100])
def test_select_closed_heaps_beyond_one_scan_round(closed_case, monkeypatch, best_n):
    c = closed_case
    set_piece(monkeypatch, None)
    assert c.tested >= T.SELECT_MIN_TESTED and 32 * T.SELECT_CHUNK > 65536 and c.tested > 2 * T.SELECT_CHUNK
    monkeypatch.delenv("KGWAS_LMM_TABLE_SELECT", raising=False)
    before = c.handle(T.SELECT_CHUNK).stats()["chunks"]
    on = c.multi(range(P), best_n, T.SELECT_CHUNK)
    assert c.handle(T.SELECT_CHUNK).stats()["chunks"] - before == -(-c.tested // T.SELECT_CHUNK) >= 3
    monkeypatch.setenv("KGWAS_LMM_TABLE_SELECT", "0")
    off = c.multi(range(P), best_n, T.SELECT_CHUNK)
    print("N %d: %d tested rows x %d columns in sub-chunks of %d: %d pairs shipped with the selection, %d without"
          % (best_n, c.tested, P, T.SELECT_CHUNK, on["pairs_shipped"], off["pairs_shipped"]))
    assert on["rows_tested"] == off["rows_tested"] == c.tested
    assert best_n * P <= on["pairs_shipped"] < c.tested * P
    # the first launch of a column ships its whole sub-chunk (the heap is open); were the later ones not thinned, more would come
    assert on["pairs_shipped"] < 2 * T.SELECT_CHUNK * P, "the launches with closed heaps shipped every pair"
    assert off["pairs_shipped"] == c.tested * P
    for k in range(P):
        same_column(on["columns"][k], c.single(k, best_n), "N %d column %d" % (best_n, k))
        same_column(off["columns"][k], on["columns"][k], "N %d column %d with and without the selection" % (best_n, k))


def test_select_ties_across_sub_chunks(tmp_path, monkeypatch):
    set_piece(monkeypatch, None)
    monkeypatch.delenv("KGWAS_LMM_TABLE_SELECT", raising=False)
    n_rows, chunk, step = T.SELECT_ROWS, T.SELECT_CHUNK, T.TIE_TO - T.TIE_FROM
    c = select_case(tmp_path, n_rows, ties=True)
    try:
        assert c.tested >= T.SELECT_MIN_TESTED
        place = np.cumsum(c.rule) - 1  # a tested row's place among the piece's compacted rows
        # from the yardstick: a column whose N-th and (N+1)-th results are the two copies of one pattern, N within the first
        # sub-chunk's rows, so that the column's heap is closed when the second copy comes
        found = None
        for k in range(P):
            full = c.single(k, n_rows)
            order = np.lexsort((full["row"], -full["lrt"]))  # by lrt descending, then the table row
            ranked = full["row"][order].astype(np.int64)
            pairs = [i for i in range(min(len(ranked) - 1, chunk - 1)) if ranked[i + 1] == ranked[i] + step]
            if pairs:
                i = pairs[len(pairs) // 2]
                found = (k, i + 1, int(ranked[i]), int(ranked[i + 1]), full["lrt"][order[i]], full["lrt"][order[i + 1]])
                break
        assert found is not None, "no column ranks the two copies of a pattern next to each other"
        k, cut, first, second, lrt_a, lrt_b = found
        assert lrt_a.tobytes() == lrt_b.tobytes() and second == first + step, "no tie at the cut"
        assert place[first] // chunk == 0 and place[second] // chunk == 1 and cut <= chunk, "the tied rows do not lie in the first two sub-chunks"
        res = c.multi(range(P), cut, chunk)
        print("column %d, N %d: rows %d and %d tie; %d of %d pairs shipped" % (k, cut, first, second, res["pairs_shipped"], c.tested * P))
        assert res["pairs_shipped"] < c.tested * P
        for j in range(P):
            same_column(res["columns"][j], c.single(j, cut), "N %d column %d" % (cut, j))
        kept = res["columns"][k]["row"].tolist()
        assert first in kept and second not in kept, "the later of two tied rows was kept"
    finally:
        c.close()


# ---- 5. panel widths -----------------------------------------------------------------------------------------------------------
WIDTHS = [(256, 256), (257, 300), (511, 512), (512, 512), (513, 600), (1135, 1200)]


@pytest.mark.parametrize("S,S_f", WIDTHS)
def test_panel_widths(tmp_path, monkeypatch, S, S_f):
    n_rows = 600
    K, y = T.kinship_and_phenotype(S)
    pick = np.random.default_rng(S_f).permutation(S_f)[:S]
    bits = T.random_bits(n_rows, S, S_f)
    rows = T.table_from_bits(bits, S_f, pick, S)
    base, acc = write_case(tmp_path, rows, S_f, pick)
    mc, maf = kg.min_count(S, 0.05, 5), 0.05
    handles = {chunk: kg.LmmLrt(K, chunk_variants=chunk) for chunk in (64, 10240)}  # (the eigendecomposition of K: once per handle)
    try:
        rows_exp, exp = bed_route(tmp_path, base, rows, pick, acc, K, y, mc, maf, m=handles[10240])
        rule = T.tested_rule(bits.sum(axis=1), S, mc, maf)
        print("S=%d S_f=%d: %d of %d rows tested" % (S, S_f, len(rows_exp), n_rows))
        assert 256 < len(rows_exp) < n_rows and rows_exp.tolist() == np.flatnonzero(rule).tolist()
        for piece in (256, None):
            set_piece(monkeypatch, piece)
            for chunk in (64, 10240):
                res = table_route(base, pick, K, y, mc, maf, n_rows, chunk, m=handles[chunk])
                assert_same(res, rows_exp, exp, "piece %s chunk %d" % (piece, chunk))
                assert (res["kmer"] == rows[rows_exp.astype(np.int64), 0]).all()
                assert res["rows_read"] == n_rows and res["rows_tested"] == len(rows_exp)
                assert res["stats"]["variants_read"] == n_rows and res["stats"]["variants_tested"] == len(rows_exp)
    finally:
        for m in handles.values():
            m.close()


@pytest.mark.parametrize("S", [257, 1135])
def test_tested_set_edges_of_wide_panels(tmp_path, monkeypatch, S):
    monkeypatch.setenv("KGWAS_LMM_PIECE_ROWS", "64")
    counts, rule = edges_case(tmp_path, S, 0.05, 5)
    mc = kg.min_count(S, 0.05, 5)
    # of the ten edge counts mc, mc + 1, S - mc - 1 and S - mc are tested, and of 0 .. S the counts mc .. S - mc
    assert mc > 5 and rule.sum() == 3 * 4 + (S - 2 * mc + 1), "the edges are not where the fixture puts them"
