"""kgwas_kmers_ld (ld_kernels.hip) against clump_np.links: adj and n1 must have the model's bytes.

The grid: n_acc below, on and past a 64-bit word and a 128-wide MFMA step; n_kmers past a 16-row sub-tile, a 32-bit adj word and
the wave's 64 x 128 tile; tile_rows 0 and 64, so that 130 and 300 rows cross block boundaries; thresholds 1, 0.8, 0.25 and
0.000001. Every table holds random rows at several densities, copies of a row (one of them at the far end), a complement, a row
one bit apart, an all-0 and an all-1 row and, where the shape has them (n_acc 64 and 128), a pair exactly on r2 = 0.25 with its
one-bit neighbour."""
import functools

import numpy as np
import pytest

import kmersgwas_amd as kg

import clump_np as CN

pytestmark = pytest.mark.gpu
N_ACC = (5, 64, 67, 128, 129, 1135)
N_KMERS = (1, 2, 17, 33, 130, 300)
TILE_ROWS = (0, 64)
TM = (1000000, 800000, 250000, 1)
# places of the special rows in a table of at least 17 rows
COPY, COMPLEMENT, NEAR, ALL0, ALL1, ON_A, ON_B, ON_NEAR = 3, 5, 6, 7, 8, 9, 10, 11


@functools.lru_cache(maxsize=None)
def table(n, N):
    rng = np.random.default_rng([n, N])
    dens = np.array([0.5, 0.02, 0.2, 0.8, 0.97])[np.arange(N) % 5]
    bits = rng.random((N, n)) < dens[:, None]
    bits[0, :2] = [True, False]  # row 0 varies
    if N >= 2:
        bits[N - 1] = bits[0]  # a copy at the far end: in another tile and another block where there are any
    if N >= 17:
        bits[COPY] = bits[0]
        bits[COMPLEMENT] = ~bits[0]
        bits[NEAR] = bits[0]
        bits[NEAR, n - 1] ^= True
        bits[ALL0] = False
        bits[ALL1] = True
        if n in (64, 128):
            a, b = CN.pair_with(n, n // 2, n // 2, 3 * n // 8)
            bits[ON_A], bits[ON_B], bits[ON_NEAR] = a, b, CN.one_bit_moved(a, b)
            bits[N - 2] = b
    bits.setflags(write=False)
    return bits


@functools.lru_cache(maxsize=None)
def model(n, N, tm):
    adj, n1 = CN.links(CN.pack_rows(table(n, N)), n, tm)
    for a in (adj, n1):
        a.setflags(write=False)
    return adj, n1


def check_fixture(n, N):
    """the table holds what the docstring says, by the model"""
    bits = table(n, N)
    if N >= 2:
        assert CN.adj_bit(model(n, N, 1000000)[0], 0, N - 1), "identical rows are not linked at r2 = 1"
    if N >= 17:
        adj1, adj25 = model(n, N, 1000000)[0], model(n, N, 250000)[0]
        assert CN.adj_bit(adj1, 0, COPY) and CN.adj_bit(adj1, 0, COMPLEMENT) and CN.adj_bit(adj1, COPY, COMPLEMENT)
        assert not CN.adj_bit(adj1, 0, NEAR) and not bits[ALL0].any() and bits[ALL1].all()
        if n in (64, 128):
            assert CN.adj_bit(adj25, ON_A, ON_B) and CN.adj_bit(adj25, ON_A, N - 2) and not CN.adj_bit(adj25, ON_A, ON_NEAR)
            assert not CN.adj_bit(model(n, N, 250001)[0], ON_A, ON_B)


@pytest.mark.parametrize("n", N_ACC)
@pytest.mark.parametrize("N", N_KMERS)
def test_bytes_equal_the_model(n, N):
    check_fixture(n, N)
    words = CN.pack_rows(table(n, N))
    dirty = np.concatenate([words, np.full((N, 2), 0xDEADBEEFDEADBEEF, np.uint64)], axis=1)  # garbage at and past n_acc
    if n % 64:
        dirty[:, n // 64] |= np.uint64((1 << 64) - (1 << (n % 64)))
    lower = np.arange(N)[None, :] <= np.arange(N)[:, None]
    for tm in TM:
        exp_adj, exp_n1 = model(n, N, tm)
        text = "%d.%06d" % (tm // 1000000, tm % 1000000)
        for tile_rows in TILE_ROWS:
            for rows in ((words, dirty) if tile_rows == 64 else (words,)):
                adj, n1 = kg.kmers_ld(rows, n, text, tile_rows=tile_rows)
                what = "n_acc=%d n_kmers=%d tm=%d tile_rows=%d%s" % (n, N, tm, tile_rows, " (garbage past n_acc)" if rows is dirty else "")
                assert n1.tobytes() == exp_n1.tobytes(), what + ": n1 differs"
                if adj.tobytes() != exp_adj.tobytes():
                    diff = np.argwhere(adj != exp_adj)
                    raise AssertionError("%s: adj differs in %d words, first at row %d word %d: %08x, the model has %08x"
                                         % (what, len(diff), diff[0][0], diff[0][1], adj[tuple(diff[0])], exp_adj[tuple(diff[0])]))
                # (stated on their own, whatever the model says)
                full = np.unpackbits(adj.view(np.uint8), axis=1, bitorder="little")[:, :N].astype(bool)
                assert not full[lower].any(), what + ": the diagonal or the lower triangle is set"
                assert not np.unpackbits(adj.view(np.uint8), axis=1, bitorder="little")[:, N:].any(), what + ": bits past the last k-mer"
                const = np.flatnonzero((exp_n1 == 0) | (exp_n1 == n))
                assert not full[const].any() and not full[:, const].any(), what + ": a constant row is linked"


@pytest.mark.parametrize("n,N", [(67, 130), (128, 300), (1135, 33)])
def test_popcount_ablation_has_the_same_bytes(monkeypatch, n, N):
    monkeypatch.setenv("KGWAS_LD_POPCOUNT", "1")
    for tm in (800000, 250000):
        adj, n1 = kg.kmers_ld(CN.pack_rows(table(n, N)), n, "%.6f" % (tm / 1e6), tile_rows=64)
        assert adj.tobytes() == model(n, N, tm)[0].tobytes() and n1.tobytes() == model(n, N, tm)[1].tobytes()


def test_largest_accession_count():
    """n_acc = 8192, the most the predicate's integers are sized for: |n n11 - ca cb| reaches 2^24, num 2^48"""
    n, N = 8192, 40
    rng = np.random.default_rng(8192)
    bits = rng.random((N, n)) < 0.5
    bits[1], bits[2], bits[3] = bits[0], ~bits[0], bits[0]
    bits[3, 8191] ^= True
    a, b = CN.pair_with(n, n // 2, n // 2, 3 * n // 8)
    bits[4], bits[5], bits[6] = a, b, CN.one_bit_moved(a, b)
    bits[7], bits[8] = False, True
    words = CN.pack_rows(bits)
    for text in ("1", "0.25", "0.250001", "0.999"):
        tm = CN.millionths(text)
        exp_adj, exp_n1 = CN.links(words, n, tm)
        adj, n1 = kg.kmers_ld(words, n, text)
        assert adj.tobytes() == exp_adj.tobytes() and n1.tobytes() == exp_n1.tobytes(), text
    assert CN.adj_bit(exp_adj, 0, 1) and CN.adj_bit(exp_adj, 0, 2) and CN.adj_bit(exp_adj, 0, 3) and not CN.adj_bit(exp_adj, 4, 5)
    assert CN.adj_bit(CN.links(words, n, 250000)[0], 4, 5) and not CN.adj_bit(CN.links(words, n, 250000)[0], 4, 6)
