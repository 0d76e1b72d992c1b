"""The model of clump_kmers (test infrastructure, not product): the link predicate in Python integers, the clump pass and the
tool's output bytes. Shared by test_clump_model.py, test_gpu_kmers_ld.py and test_gpu_clump_kmers.py.

For rows a, b over n accessions with presence counts ca, cb and n11 accessions in common
    num = (n n11 - ca cb)^2,  den = ca (n - ca) cb (n - cb),  linked iff den > 0 and num * 10^6 >= tm * den
with tm the threshold in millionths. Nothing here rounds: the counts are exact int64 sums of 0/1 products, the predicate is
evaluated on Python integers (object arrays)."""
from fractions import Fraction

import numpy as np


def millionths(text):
    """the threshold's decimal text -> integer millionths, through Fraction (never a float)"""
    f = Fraction(text) * 1000000
    assert f.denominator == 1 and 0 < f <= 1000000, text
    return int(f)


def pack_rows(bits, words=None):
    """bool [N, n] -> uint64 [N, words] with bit i of a row = accession i"""
    bits = np.asarray(bits, bool)
    N, n = bits.shape
    W = words or max(1, (n + 63) // 64)
    pad = np.zeros((N, W * 64), bool)
    pad[:, :n] = bits
    return np.packbits(pad.reshape(N, W, 64), axis=2, bitorder="little").view(np.uint64).reshape(N, W)


def unpack_rows(words, n):
    """the inverse of pack_rows: uint64 [N, W] -> bool [N, n]; bits at or past n are dropped"""
    words = np.ascontiguousarray(words, np.uint64)
    N = words.shape[0]
    return np.unpackbits(words.view(np.uint8).reshape(N, -1), axis=1, bitorder="little")[:, :n].astype(bool)


def _obj(a):
    return np.asarray(a).astype(object)


def linked_matrix(bits, tm):
    """bool [N, n] -> (bool [N, N] linked, symmetric, diagonal included where den > 0; int64 [N] n1; int64 [N, N] n11)"""
    B = np.asarray(bits, bool).astype(np.int64)
    N, n = B.shape
    n1 = B.sum(axis=1)
    n11 = B @ B.T
    ca, cb = _obj(n1)[:, None], _obj(n1)[None, :]
    num = (int(n) * _obj(n11) - ca * cb) ** 2
    den = ca * (int(n) - ca) * cb * (int(n) - cb)
    linked = ((den > 0) & (num * 1000000 >= int(tm) * den)).astype(bool).reshape(N, N)
    return linked, n1, n11


def links(words, n, tm):
    """uint64 [N, W] rows -> (adj uint32 [N, ceil(N / 32)], n1 uint32 [N]): adj[a, b // 32] bit b % 32 = (b > a and linked)"""
    bits = unpack_rows(words, n)
    N = bits.shape[0]
    linked, n1, _ = linked_matrix(bits, tm)
    upper = linked & (np.arange(N)[None, :] > np.arange(N)[:, None])
    ndw = (N + 31) // 32
    pad = np.zeros((N, ndw * 32), bool)
    pad[:, :N] = upper
    adj = np.packbits(pad.reshape(N, ndw, 32), axis=2, bitorder="little").view(np.uint32).reshape(N, ndw)
    return adj, n1.astype(np.uint32)


def adj_bit(adj, a, b):
    return bool((int(adj[a, b // 32]) >> (b % 32)) & 1)


def clump(order, adj):
    """order: the hits' ids in p order (row i of adj is hit order[i]). Rows are walked in order; a row no lead has taken becomes
    a lead and takes every later row linked to it and not yet taken. -> (lead_of {hit: its lead}, leads [hit, ...] in lead order)"""
    N = len(order)
    lead_of, leads = {}, []
    for a in range(N):
        if order[a] in lead_of:
            continue
        lead_of[order[a]] = order[a]
        leads.append(order[a])
        for b in range(a + 1, N):
            if order[b] not in lead_of and adj_bit(adj, a, b):
                lead_of[order[b]] = order[a]
    return lead_of, leads


def p_order(p_texts, p_max=float("inf")):
    """the hits with p <= p_max by p ascending, ties by their line"""
    p = [float(t) for t in p_texts]
    return sorted((i for i in range(len(p)) if p[i] <= p_max), key=lambda i: (p[i], i))


HEADER = "rs\tp_lrt\tclump\tlead\tr2\tn1\tn11\n"


def format(rs, p_texts, bits, lead_of, leads):
    """The tool's output: one line per used hit (a key of lead_of) in file order. bits: bool [hits, n] over the accessions in use."""
    bits = np.asarray(bits, bool)
    n = bits.shape[1]
    number = {h: k + 1 for k, h in enumerate(leads)}
    out = [HEADER]
    for h in range(len(rs)):
        if h not in lead_of:
            continue
        l = lead_of[h]
        ca, cb, n11 = int(bits[h].sum()), int(bits[l].sum()), int((bits[h] & bits[l]).sum())
        num, den = (n * n11 - ca * cb) ** 2, ca * (n - ca) * cb * (n - cb)
        r2 = "nan" if den == 0 else "%.6f" % (1.0 if l == h else num / den)
        out.append("%s\t%s\t%d\t%s\t%s\t%d\t%d\n" % (rs[h], p_texts[h], number[l], rs[l], r2, ca, n11))
    return "".join(out).encode()


def run(rs, p_texts, bits, tm, p_max=float("inf")):
    """assoc lines (rs, p text) and their rows over the accessions in use -> the bytes clump_kmers writes"""
    bits = np.asarray(bits, bool)
    order = p_order(p_texts, p_max)
    adj, _ = links(pack_rows(bits[order]), bits.shape[1], tm) if order else (np.zeros((0, 0), np.uint32), None)
    lead_of, leads = clump(order, adj)
    return format(rs, p_texts, bits, lead_of, leads)


# ---- pairs exactly on a threshold, and their one-bit neighbours -------------------------------------------------------------------
def pair_with(n, ca, cb, n11):
    """two rows over n accessions with the given counts: a = the first ca, b = n11 of them and cb - n11 of the others"""
    a, b = np.zeros(n, bool), np.zeros(n, bool)
    a[:ca] = True
    b[:n11] = True
    b[ca:ca + cb - n11] = True
    return a, b


ON_THRESHOLD = [  # (n, ca, cb, n11, threshold text): r2 equals the threshold exactly
    (8, 4, 4, 3, "0.25"), (64, 32, 32, 24, "0.25"), (128, 64, 64, 48, "0.25"),
]


def one_bit_moved(a, b):
    """b with one shared accession moved to one neither row has: n11 falls by one, the counts stay"""
    both, neither = np.flatnonzero(a & b), np.flatnonzero(~a & ~b)
    c = b.copy()
    c[both[-1]] = False
    c[neither[-1]] = True
    return c
