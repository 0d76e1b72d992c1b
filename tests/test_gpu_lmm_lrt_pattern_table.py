"""One pattern table behind lmm_lrt --pattern_cache and --pattern_skip (the lmm_pattern_* kernels of lmm_table_kernels.hip).

What a tested row is to the table - the owner of a new slot, a row whose code row equals its slot's, collided or rejected - is
decided from the piece's code rows alone: not from the phenotypes, and not from the route that asks. So on one table, at one piece
size, slot count and tag width, kgwas_lmm_test_table_unique and kgwas_lmm_test_table_multi_skip must count the same slots,
patterns_cached, rows_collided and rows_rejected, and the rows the cache serves (rows_from_cache) are the rows the skip finds equal
to their slot, dead or live: rows_tested - patterns_cached - rows_collided - rows_rejected of the skip run.

The table has 4096 slots, far more than the fixture's patterns: in a full table the tags that win a slot depend on the order of
the atomics, and those counters are not compared between runs anywhere."""
import numpy as np
import pytest

import kmersgwas_amd as kg
from oracle import oracle_np as onp

import lmm_table_np as T
import lmm_unique_np as Q

pytestmark = pytest.mark.gpu
SHARED = ("slots", "patterns_cached", "rows_collided", "rows_rejected")
SLOTS, P, BEST = 4096, 3, 7


@pytest.fixture(scope="module")
def repeated67(tmp_path_factory):
    S, S_f = 67, 70
    bits = Q.repeated_bits(S)
    pick = Q.pick_of(S, S_f)
    names = ["acc%d" % i for i in range(S_f)]
    base = str(tmp_path_factory.mktemp("pattern_table") / "tab")
    table = T.table_from_bits(bits, S_f, pick, S)
    onp.write_table(base, names, T.K_LEN, table[:, 0], table[:, 1:])
    K, y = T.kinship_and_phenotype(S)
    rng = np.random.default_rng(11)
    Y = np.stack([y] + [rng.permutation(y) for _ in range(P - 1)])
    return {"base": base, "pick": np.asarray(pick, np.uint64), "K": K, "y": y, "Y": Y, "mc": Q.min_count_of(S),
            "tested": int(Q.tested_of(bits, S).sum())}


@pytest.mark.parametrize("tag_bits", [None, 4])
@pytest.mark.parametrize("piece,chunk", Q.GEOMETRIES[:2])
def test_both_routes_look_up_alike(repeated67, monkeypatch, piece, chunk, tag_bits):
    f = repeated67
    monkeypatch.delenv("KGWAS_LMM_TABLE_SELECT", raising=False)
    monkeypatch.setenv("KGWAS_LMM_PIECE_ROWS", str(piece))
    if tag_bits is None:
        monkeypatch.delenv("KGWAS_LMM_PATTERN_TAG_BITS", raising=False)
    else:
        monkeypatch.setenv("KGWAS_LMM_PATTERN_TAG_BITS", str(tag_bits))
    tbl, m = kg.KmersTable(f["base"], T.K_LEN), kg.LmmLrt(f["K"], chunk_variants=chunk)
    try:
        one = m.test_table(tbl, f["pick"], f["y"], f["mc"], Q.MAF, BEST, max_patterns=SLOTS)
        many = m.test_table_multi(tbl, f["pick"], f["Y"], f["mc"], Q.MAF, BEST, max_patterns=SLOTS)
    finally:
        m.close()
        tbl.close()
    u, k = one["unique"], many["skip"]
    print("piece %d chunk %d tag bits %s: cache %s skip %s" % (piece, chunk, tag_bits, u, k))
    assert one["rows_tested"] == many["rows_tested"] == f["tested"]
    assert u["slots"] == SLOTS
    assert {c: u[c] for c in SHARED} == {c: k[c] for c in SHARED}
    assert u["rows_from_cache"] == many["rows_tested"] - k["patterns_cached"] - k["rows_collided"] - k["rows_rejected"]
    if tag_bits is None:
        assert u["rows_collided"] == 0 and u["rows_rejected"] == 0 and u["rows_from_cache"] > 0
    else:
        assert u["rows_collided"] > 0 and u["patterns_cached"] <= 15
