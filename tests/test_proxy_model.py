"""proxy_np, the model behind the proxy_kmers tests, checked on cases whose answers are known without it."""
import numpy as np

import clump_np as CN
import proxy_np as PN


def base_row(n=40):
    rng = np.random.default_rng(n)
    a = rng.random(n) < 0.4
    a[:2] = [True, False]
    return a


def test_a_copy_is_found_with_plus_and_a_complement_with_minus():
    a = base_row()
    other = np.roll(a, 7) ^ (np.arange(40) % 3 == 0)
    rows = np.array([other, a, ~a])
    rec = PN.records(a[None], rows, 1000000)
    assert rec["row"].tolist() == [1, 2] and rec["lead"].tolist() == [0, 0]
    assert rec["n1"].tolist() == [int(a.sum()), int((~a).sum())] and rec["n11"].tolist() == [int(a.sum()), 0]
    assert (rec["kmer"] == 0).all() and (rec["pad"] == 0).all() and rec.dtype.itemsize == 32
    out, log, counts = PN.run(["ACGTACGTAC"], a[None], np.array([5, 6, 7], np.uint64), rows, 1000000, 10)
    lines = out.decode().split("\n")
    assert lines[0] + "\n" == PN.HEADER == "lead\tkmer\tr2\tphase\tn1\tn11\trow\n"
    assert lines[1] == "ACGTACGTAC\tAAAAAAAACG\t1.000000\t+\t%d\t%d\t1" % (a.sum(), a.sum())
    assert lines[2] == "ACGTACGTAC\tAAAAAAAACT\t1.000000\t-\t%d\t0\t2" % (~a).sum()
    assert log == b"lead\tACGTACGTAC\t2\t2\n" and counts == [(2, 2)]


def test_a_row_one_bit_off_is_not_found_at_r2_1():
    a = base_row()
    near = a.copy()
    near[-1] ^= True
    assert len(PN.records(a[None], near[None], 1000000)) == 0
    assert len(PN.records(a[None], near[None], 800000)) == 1


def test_constant_rows_are_found_by_nobody_and_find_nobody():
    a = base_row()
    zeros, ones = np.zeros(40, bool), np.ones(40, bool)
    rec = PN.records(np.array([a, zeros, ones]), np.array([zeros, ones, a, zeros]), 1)
    assert rec["row"].tolist() == [2] and rec["lead"].tolist() == [0]


def test_records_are_in_row_then_lead_order_and_max_per_lead_keeps_the_first():
    a = base_row()
    leads = np.array([a, ~a, np.roll(a, 1)])
    rows = np.array([a, np.roll(a, 1), ~a, a])
    rec = PN.records(leads, rows, 1000000, row0=100)
    assert list(zip(rec["row"].tolist(), rec["lead"].tolist())) == [(100, 0), (100, 1), (101, 2), (102, 0), (102, 1), (103, 0), (103, 1)]
    out, log, counts = PN.run(["A" * 10, "C" * 10, "G" * 10], leads, np.arange(4, dtype=np.uint64), rows, 1000000, 10, max_per_lead=2)
    assert counts == [(2, 3), (2, 3), (1, 1)]
    body = [l.split("\t") for l in out.decode().split("\n")[1:-1]]
    assert [(l[0][0], l[6]) for l in body] == [("A", "0"), ("A", "2"), ("C", "0"), ("C", "2"), ("G", "1")]
    assert log == b"lead\tAAAAAAAAAA\t2\t3\nlead\tCCCCCCCCCC\t2\t3\nlead\tGGGGGGGGGG\t1\t1\n"


def test_pairs_on_the_threshold():
    for n, ca, cb, n11, text in CN.ON_THRESHOLD:
        a, b = CN.pair_with(n, ca, cb, n11)
        tm = CN.millionths(text)
        assert len(PN.records(a[None], b[None], tm)) == 1 and len(PN.records(b[None], a[None], tm)) == 1
        assert len(PN.records(a[None], b[None], tm + 1)) == 0
        assert len(PN.records(a[None], CN.one_bit_moved(a, b)[None], tm)) == 0


def test_the_model_agrees_with_clump_np_on_a_square():
    rng = np.random.default_rng(3)
    bits = rng.random((40, 67)) < rng.uniform(0.05, 0.95, 40)[:, None]
    bits[5], bits[9] = bits[1], ~bits[1]
    for tm in (1000000, 250000, 1):
        linked, _, _ = CN.linked_matrix(bits, tm)
        rect = PN.linked_rect(bits, bits, tm)[0]
        assert (rect == linked).all() and rect[1, 5] and rect[1, 9]
