"""What kgwas_lmm_get_stats reports beside the counts the other lmm_lrt suites pin: `chunks` and the bucket a stage's time goes to
(rotate_ms, grid_ms, refine_ms), on all four routes (test, test_bed_multi, test_table, test_table_multi).

Every expected value is arithmetic from the inputs. A chunk is one pass of the back end: a .bed route makes ceil(M / c) of them
for M variants, c being chunk_variants rounded up to a multiple of 32, whatever the number of phenotype columns; a table route
makes ceil(t_k / c) per piece of table rows, t_k being the piece's tested rows by lmm_table_np.tested_rule. A table without a
tested row runs the front end alone, so only rotate_ms moves."""
import math

import numpy as np
import pytest

import kmersgwas_amd as kg

import lmm_table_np as T
from test_gpu_lmm_lrt_multi import panel, phenotypes
from test_gpu_lmm_lrt_table_multi import make_case

pytestmark = pytest.mark.gpu
TIMES = ("rotate_ms", "grid_ms", "refine_ms")


def delta(m, call):
    """the change of every field of m.stats() over call()"""
    before = m.stats()
    call()
    after = m.stats()
    return {k: after[k] - before[k] for k in before}


def all_stages_ran(d, what):
    for k in TIMES:
        print("%s: %s += %.6f" % (what, k, d[k]))
        assert math.isfinite(d[k]) and d[k] > 0, "%s: %s did not grow" % (what, k)


@pytest.mark.parametrize("chunk_variants,chunks", [(32, 5), (64, 3), (10240, 1)])
def test_bed_routes(chunk_variants, chunks):
    n, nv = 67, 130
    assert chunks == -(-nv // ((chunk_variants + 31) // 32 * 32))
    K, _ = T.kinship_and_phenotype(n)
    Y, bed = phenotypes(n), panel(n, nv)[1]
    m = kg.LmmLrt(K, chunk_variants=chunk_variants)
    try:
        for what, call in (("test", lambda: m.test(bed, Y[0])), ("test_bed_multi P 3", lambda: m.test_bed_multi(Y[:3], bed)),
                           ("test_bed_multi P 33", lambda: m.test_bed_multi(Y[:33], bed))):
            d = delta(m, call)
            assert d["chunks"] == chunks, what
            all_stages_ran(d, "chunk_variants %d %s" % (chunk_variants, what))
    finally:
        m.close()


def test_table_routes(tmp_path, monkeypatch):
    S, n_rows, piece, chunk = 67, 1200, 1000, 32
    monkeypatch.setenv("KGWAS_LMM_PIECE_ROWS", str(piece))
    monkeypatch.delenv("KGWAS_LMM_TABLE_SELECT", raising=False)
    bits = T.random_bits(n_rows, S, 70)
    c = make_case(tmp_path, S, 70, n_rows, 33, bits=bits)
    try:
        tested = T.tested_rule(bits.sum(axis=1), S, c.mc, c.maf)
        per_piece = [int(tested[k:k + piece].sum()) for k in range(0, n_rows, piece)]
        assert len(per_piece) == 2 and all(t > chunk for t in per_piece)
        chunks = sum(-(-t // chunk) for t in per_piece)
        m = c.handle(chunk)
        d = delta(m, lambda: m.test_table(c.tbl, c.pick, c.Y[0], c.mc, c.maf, 100))
        assert d["chunks"] == chunks and d["variants_tested"] == sum(per_piece)
        all_stages_ran(d, "test_table")
        for P in (1, 33):
            d = delta(m, lambda: c.multi(range(P), 100, chunk))
            assert d["chunks"] == chunks, "P %d" % P
            all_stages_ran(d, "test_table_multi P %d" % P)
        monkeypatch.setenv("KGWAS_LMM_TABLE_SELECT", "0")
        assert delta(m, lambda: c.multi(range(33), 100, chunk))["chunks"] == chunks, "without the selection"
    finally:
        c.close()


def test_table_without_a_tested_row(tmp_path):
    S = 67
    bits = T.bits_with_counts([0, 1, 2, 4, S, S - 4, S - 1] * 40, S, 1)  # (test_gpu_lmm_lrt_table_multi.test_no_row_tested's)
    c = make_case(tmp_path, S, S, len(bits), 3, bits=bits)
    try:
        m = c.handle(64)
        for what, call in (("test_table", lambda: m.test_table(c.tbl, c.pick, c.Y[0], c.mc, c.maf, 100)),
                           ("test_table_multi", lambda: c.multi(range(3), 100, 64))):
            d = delta(m, call)
            assert d["variants_read"] == len(bits) and d["variants_tested"] == 0, what
            assert d["chunks"] == 0, what
            assert d["grid_ms"] == 0.0 and d["refine_ms"] == 0.0, what + ": a back-end stage was timed"
            assert math.isfinite(d["rotate_ms"]) and d["rotate_ms"] > 0, what + ": the front end was not timed"
    finally:
        c.close()
