"""The model of proxy_kmers (test infrastructure, not product), on clump_np: which rows are in LD with which leads, as the records
kgwas_kmers_ld_proxies returns, the tool's output bytes and its per-lead log lines. Shared by test_proxy_model.py,
test_gpu_kmers_ld_proxies.py and test_gpu_proxy_kmers.py.

The predicate is clump_np's, evaluated in Python integers (object arrays) on the L x R matrix of counts: for a lead a and a row b
over n accessions, num = (n n11 - ca cb)^2, den = ca (n - ca) cb (n - cb), linked iff den > 0 and num * 10^6 >= tm * den. There is
no diagonal rule: a lead's own row is a row like any other."""
import numpy as np

import clump_np as CN

RECORD = np.dtype([("row", np.uint64), ("kmer", np.uint64), ("lead", np.uint32), ("n1", np.uint32), ("n11", np.uint32), ("pad", np.uint32)])
HEADER = "lead\tkmer\tr2\tphase\tn1\tn11\trow\n"


def num_den(lead_bits, bits):
    """bool [L, n], bool [R, n] -> (num, den as object [L, R] of Python integers, int64 [L] and [R] the counts, int64 [L, R] n11):
    everything about the pairs that does not depend on the threshold"""
    A, B = np.asarray(lead_bits, bool).astype(np.int64), np.asarray(bits, bool).astype(np.int64)
    n = A.shape[1]
    assert B.shape[1] == n
    ca, cb = A.sum(axis=1), B.sum(axis=1)
    n11 = A @ B.T
    oa, ob = CN._obj(ca)[:, None], CN._obj(cb)[None, :]
    num = (int(n) * CN._obj(n11) - oa * ob) ** 2
    den = oa * (int(n) - oa) * ob * (int(n) - ob)
    return num, den, ca, cb, n11


def linked_rect(lead_bits, bits, tm, nd=None):
    """-> (bool [L, R] linked, int64 [L] n1 of the leads, int64 [R] n1 of the rows, int64 [L, R] n11); nd: num_den's, if at hand"""
    num, den, ca, cb, n11 = nd or num_den(lead_bits, bits)
    linked = ((den > 0) & (num * 1000000 >= int(tm) * den)).astype(bool).reshape(n11.shape)
    return linked, ca, cb, n11


def records(lead_bits, bits, tm, kmers=None, row0=0, nd=None):
    """the records in (row, lead) order: rows ascending, leads ascending within a row. kmers: uint64 [R] or None (0)."""
    linked, _, cb, n11 = linked_rect(lead_bits, bits, tm, nd)
    rows, leads = np.nonzero(linked.T)  # (row-major over [R, L]: the order asked for)
    rec = np.zeros(len(rows), RECORD)
    rec["row"] = rows + row0
    rec["kmer"] = 0 if kmers is None else np.asarray(kmers, np.uint64)[rows]
    rec["lead"], rec["n1"], rec["n11"] = leads, cb[rows], n11[leads, rows]
    return rec


def kmer_text(word, k):
    """bits2kmer31: the most significant base first"""
    return "".join("ACGT"[(int(word) >> (2 * (k - 1 - i))) & 3] for i in range(k))


def run(lead_texts, lead_bits, kmers, bits, tm, k, max_per_lead=100000):
    """The tool: lead texts (as their file spells them) with their rows' bits, and the table (k-mer words and bits, both over the
    accessions in use) -> (the output's bytes, the log's per-lead lines as bytes, [(kept, found)] per lead)"""
    lead_bits = np.asarray(lead_bits, bool)
    n = lead_bits.shape[1]
    rec = records(lead_bits, bits, tm, kmers)
    ca = lead_bits.sum(axis=1)
    out, log, counts = [HEADER], [], []
    for l, text in enumerate(lead_texts):
        mine = rec[rec["lead"] == l]  # (in table-row order already)
        kept = mine[:max_per_lead]
        for r in kept:
            a, b, n11 = int(ca[l]), int(r["n1"]), int(r["n11"])
            num, den, d = (n * n11 - a * b) ** 2, a * (n - a) * b * (n - b), n * n11 - a * b
            out.append("%s\t%s\t%.6f\t%s\t%d\t%d\t%d\n" % (text, kmer_text(r["kmer"], k), num / den, "-" if d < 0 else "+", b, n11, int(r["row"])))
        log.append("lead\t%s\t%d\t%d\n" % (text, len(kept), len(mine)))
        counts.append((len(kept), len(mine)))
    return "".join(out).encode(), "".join(log).encode(), counts
