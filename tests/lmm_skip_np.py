"""Shared by test_lmm_skip_model.py and test_gpu_lmm_lrt_table_multi_skip.py (test infrastructure, not product): the dead-pattern
skip of kgwas_lmm_test_table_multi_skip restated in numpy.

simulate() takes what the device cannot change - every tested row's pattern, table row and per-column lrt - and walks the pieces of
table_pass, the sub-chunks of the tested rows (cut as without the skip, the dead rows then left out) and the blocks of 32 columns as
the host does: the thresholds are snapshotted
before each block, a pair ships iff its column's heap is open or its lrt is above the snapshot, the host heaps keep the best N by
(lrt, row), and a computed row that shipped no pair marks its pattern dead for the pieces that follow. It assumes a table that
rejects nothing and tags that do not collide: every pattern has a slot of its own."""
import heapq

import numpy as np

import lmm_table_np as T
import lmm_unique_np as Q

PBLOCK = 32                  # LMM_PBLOCK: phenotype columns per block
ROWS, PATTERNS, PANELS, WIDE, GEOMETRIES, MAF = Q.ROWS, Q.PATTERNS, Q.PANELS, Q.WIDE, Q.GEOMETRIES, Q.MAF
# (P, N) per geometry of GEOMETRIES: over the three geometries every P of 1, 3, 32, 33 meets every N of 1, 7, 100
CASES = {0: [(1, 100), (3, 7), (32, 1), (33, 100)], 1: [(1, 7), (3, 1), (32, 100), (33, 7)], 2: [(1, 1), (3, 100), (32, 7), (33, 1)]}
MAX_P = 33


def claims_skipping(geometry, S):
    """the parametrisations for which the tests demand rows_skipped > 0: pieces of 1024 or 1000 rows (the default piece holds the
    whole fixture, and a row is skipped only in a later piece than the one that marked its pattern); five accessions have 30
    tested patterns, which is too few for any claim"""
    return GEOMETRIES[geometry][0] is not None and S != 5


def patterns_of(bits, tested):
    """per tested row, in row order: the number of its distinct pattern"""
    tb = np.packbits(np.asarray(bits)[np.flatnonzero(tested)], axis=1)
    _, pattern = np.unique(tb, axis=0, return_inverse=True)
    return pattern.reshape(-1)


def synthetic_lrt(pattern, P, seed):
    """hand-made lrt (P x tested rows): one chi-square(1) draw per (column, pattern), so equal patterns have equal values"""
    rng = np.random.default_rng([seed, P, int(pattern.max()) + 1])
    return (rng.standard_normal((P, int(pattern.max()) + 1)) ** 2)[:, pattern]


def _key(x):
    return -np.inf if np.isnan(x) else x  # ranks_before: a NaN lrt ranks last


def simulate(pattern, rows, lrt, piece, chunk, N, select=True, trace=None, block_trace=None, flag_blocks=None):
    """pattern, rows [T]: the tested rows' pattern numbers and table rows, ascending; lrt [P][T]; piece: rows per piece of the
    table; chunk: chunk_variants. Returns the counters a run must show. trace, if a list, gets one (row, shipped, was_open) per
    computed row, block_trace one (row, per block of columns: did a pair ship) per computed row. flag_blocks=1 is a WRONG rule, for
    the tests' own checks: only the first block of columns counts for "any pair shipped"."""
    pattern, rows, lrt = np.asarray(pattern), np.asarray(rows, np.int64), np.asarray(lrt, np.float64)
    P, T_ = lrt.shape
    assert len(pattern) == len(rows) == T_ and (np.diff(rows) > 0).all()
    heaps = [[] for _ in range(P)]  # min-heaps of (lrt key, -row): the worst kept result on top
    cached, dead = set(), set()
    out = {"patterns_cached": 0, "patterns_dead": 0, "rows_skipped": 0, "rows_rotated": 0, "pairs_shipped": 0}
    piece_of = rows // piece
    for k in np.unique(piece_of):
        idx = np.flatnonzero(piece_of == k)
        dead_at_start = frozenset(dead)
        n_live = sum(pattern[i] not in dead_at_start for i in idx)
        out["rows_skipped"] += len(idx) - n_live
        out["rows_rotated"] += n_live
        for i in idx:
            if pattern[i] not in cached:
                cached.add(pattern[i])
                out["patterns_cached"] += 1
        for s0 in range(0, len(idx), chunk):  # the sub-chunks of all tested rows of the piece, less their dead rows
            sub = np.array([i for i in idx[s0:s0 + chunk] if pattern[i] not in dead_at_start], np.int64)
            if not len(sub):
                continue
            shipped = np.zeros(len(sub), bool)
            any_open = np.zeros(len(sub), bool)
            per_block = []
            for p0 in range(0, P, PBLOCK):
                cols = range(p0, min(p0 + PBLOCK, P))
                in_block = np.zeros(len(sub), bool)
                snap = [(not select or len(heaps[c]) < N, heaps[c][0][0] if len(heaps[c]) >= N else 0.0) for c in cols]
                for c, (is_open, thr) in zip(cols, snap):
                    v = lrt[c, sub]
                    ships = np.ones(len(sub), bool) if is_open else v > thr  # (false for a NaN)
                    in_block |= ships
                    any_open |= is_open
                    out["pairs_shipped"] += int(ships.sum())
                    for j in np.flatnonzero(ships):  # the (column, row) order of the records
                        item = (_key(v[j]), -int(rows[sub[j]]))
                        if len(heaps[c]) < N:
                            heapq.heappush(heaps[c], item)
                        elif item > heaps[c][0]:
                            heapq.heapreplace(heaps[c], item)
                per_block.append(in_block)
                if flag_blocks is None or len(per_block) <= flag_blocks:
                    shipped |= in_block
            for j in np.flatnonzero(~shipped):
                dead.add(pattern[sub[j]])
            if trace is not None:
                trace.extend(zip(rows[sub].tolist(), shipped.tolist(), any_open.tolist()))
            if block_trace is not None:
                block_trace.extend(zip(rows[sub].tolist(), any_open.tolist(), zip(*[b.tolist() for b in per_block])))
    out["patterns_dead"] = len(dead)
    out["kept"] = [sorted(-r for _, r in h) for h in heaps]
    return out


def skip_bound(pattern, rows, piece, N):
    """An upper bound of rows_skipped that holds for any table size and tags: a row can be skipped only if a row with its pattern
    lies in an earlier piece, in or behind a sub-chunk that began with every heap closed, that is with at least N tested rows
    before it - so behind the N-th tested row."""
    pattern, rows = np.asarray(pattern), np.asarray(rows, np.int64)
    piece_of = rows // piece
    bound = 0
    first_markable = {}  # pattern -> piece of its first row behind the N-th tested row
    for i in range(len(rows)):
        if i >= N and pattern[i] not in first_markable:
            first_markable[pattern[i]] = piece_of[i]
    for i in range(len(rows)):
        p = first_markable.get(pattern[i])
        if p is not None and p < piece_of[i]:
            bound += 1
    return bound


def fixture(S, S_f):
    """the base fixture of the GPU tests: 3000 rows drawn from 300 patterns (lmm_unique_np.repeated_bits)"""
    bits = Q.repeated_bits(S)
    tested = Q.tested_of(bits, S)
    pick = Q.pick_of(S, S_f)
    table = T.table_from_bits(bits, S_f, pick, S)
    return {"S": S, "S_f": S_f, "bits": bits, "tested": tested, "pick": pick, "table": table, "rows": np.flatnonzero(tested),
            "pattern": patterns_of(bits, tested), "mc": Q.min_count_of(S)}


def piece_of_geometry(f, geometry):
    return T.piece_rows(len(f["bits"]), GEOMETRIES[geometry][0], f["table"].shape[1])
