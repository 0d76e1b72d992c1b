"""Shared by test_gpu_lmm_lrt_table_unique.py and test_lmm_lrt_table_unique_cli.py (test infrastructure, not product): tables whose
rows repeat presence/absence patterns, and what the pattern cache of kgwas_lmm_test_table_unique must meet in them, restated in
numpy from the squeezed tested rows alone: the distinct patterns, each one's first row (its owner), the pieces of table_pass and the
sub-chunks of the rows to rotate."""
import functools

import numpy as np

import lmm_table_np as T

ROWS, PATTERNS = 3000, 300
PANELS = [(5, 5), (64, 64), (67, 70), (241, 241)]   # (S, S_f); S_f = 70 with a shuffled column map
WIDE = (1135, 1200)                                  # a code row of 71 dwords: more than a wave of lanes
GEOMETRIES = [(1024, 32), (1000, 64), (None, 10240)]  # (KGWAS_LMM_PIECE_ROWS, chunk_variants)
MAF = 0.05


def min_count_of(S):
    """min_count of the fixtures: kgwas_min_count(S, 0.05, 5), and 1 for the five accessions of the smallest panel"""
    return 1 if S == 5 else max(int(np.ceil(S * MAF)), 5)


def pick_of(S, S_f):
    return np.arange(S) if S == S_f else np.random.default_rng(S_f).permutation(S_f)[:S]


@functools.lru_cache(maxsize=None)
def repeated_bits(S, n_rows=ROWS, n_patterns=PATTERNS, seed=11):
    """bits (n_rows x S): every row one of n_patterns patterns with frequencies 0.01 .. 0.99, drawn at random, so that the copies
    of a pattern lie all over the table"""
    patterns = T.random_bits(n_patterns, S, seed)
    rng = np.random.default_rng([seed, S, n_rows, n_patterns])
    bits = patterns[rng.integers(0, n_patterns, n_rows)]
    bits.setflags(write=False)
    return bits


def tested_of(bits, S):
    return T.tested_rule(np.asarray(bits).sum(axis=1), S, min_count_of(S), MAF)


def geometry(bits, tested, n_rows, words_per_row, piece_forced, chunk):
    """What a cache that rejects nothing and meets no tag collision does with the tested rows, per tested row in row order:
    pattern (the number of its distinct pattern), owner (is it the first row of its pattern), piece, owner_piece (the piece of its
    pattern's first row), sub (for a row to rotate - an owner - its sub-chunk within its piece), owner_sub."""
    rows = np.flatnonzero(tested)
    tb = np.packbits(np.asarray(bits)[rows], axis=1)
    _, first, pattern = np.unique(tb, axis=0, return_index=True, return_inverse=True)
    pattern = pattern.reshape(-1)
    owner = np.zeros(len(rows), bool)
    owner[first] = True
    piece = rows // T.piece_rows(n_rows, piece_forced, words_per_row)
    sub = np.full(len(rows), -1)
    for k in np.unique(piece):
        own = np.flatnonzero((piece == k) & owner)
        sub[own] = np.arange(len(own)) // chunk
    return {"rows": rows, "pattern": pattern, "distinct": len(first), "owner": owner, "piece": piece, "owner_piece": piece[first][pattern],
            "sub": sub, "owner_sub": sub[first][pattern]}


def assert_fixture(bits, tested, words_per_row, sub_chunks=True):
    """The repeated-pattern fixture holds what it is for, at the pieces and chunks of GEOMETRIES: fewer distinct patterns than half
    the tested rows; copies of a pattern in their owner's piece and in later pieces; and, at chunk_variants 32 and 64, copies whose
    owner in the same piece is rotated in a sub-chunk behind the piece's first - a fan-out that ran before the piece's last
    sub-chunk would hand them a result nobody has written. sub_chunks=False leaves that part out: five accessions have 30 tested
    patterns, fewer than a sub-chunk. (The owner is the first row of its pattern, so it never lies behind a copy in row order; the
    sub-chunk that holds the last owner before a copy is the copy's owner's for some copies and a later one for others.)"""
    n_rows = len(bits)
    for piece_forced, chunk in GEOMETRIES:
        g = geometry(bits, tested, n_rows, words_per_row, piece_forced, chunk)
        n = len(g["rows"])
        assert 0 < g["distinct"] < n / 2, "%d distinct patterns among %d tested rows" % (g["distinct"], n)
        copy = ~g["owner"]
        same_piece = copy & (g["owner_piece"] == g["piece"])
        assert same_piece.any(), "no copy in its owner's piece"
        if piece_forced:
            assert g["piece"].max() >= 2 and (copy & (g["owner_piece"] < g["piece"])).any(), "no copy in a later piece than its owner"
        if chunk < 10240 and sub_chunks:
            assert g["sub"].max() >= 1, "one sub-chunk per piece"
            assert (same_piece & (g["owner_sub"] >= 1)).any(), "no copy whose owner is rotated behind the first sub-chunk of their piece"
            # the sub-chunk that holds the last owner before the copy: the owner's own, or a later one
            at = np.full(n, -1)
            for k in np.unique(g["piece"]):
                in_k = g["piece"] == k
                at[in_k] = np.maximum.accumulate(np.where(g["owner"][in_k], g["sub"][in_k], -1))
            here = same_piece & (at >= 0)
            assert (here & (at == g["owner_sub"])).any() and (here & (at > g["owner_sub"])).any(), "copies and owners share every sub-chunk"
    return geometry(bits, tested, n_rows, words_per_row, None, 10240)["distinct"]
