"""kgwas_kmers_ld_proxies (ld_kernels.hip: ld_rect_kernel and the compaction) against proxy_np.records: the records' bytes and
the count must be the model's.

The grid, the smallest shapes at each boundary: n_acc below, on and past a 64-bit word, a 128-wide MFMA step and a round of 512
accessions; leads below a 16-row sub-tile, on and past the wave's 64 leads and into a third tile row; rows below, on and past
the 128-row tile and the compaction's 256-row block; KGWAS_PROXY_PIECE_ROWS 128 and 256, so that 300 and 1000 rows cross pieces;
thresholds 1, 0.8, 0.25 and 0.000001, where nearly every pair links. Tables are built like test_gpu_kmers_ld.table: several
densities, copies of lead 0 (one in the last row), a complement, a row one bit off, an all-0 and an all-1 row among the leads and
among the rows and, at n_acc 64 and 128, the pair exactly on r2 = 0.25 with its one-bit neighbour. Every combination of the four
dimensions runs; a test case is one (n_acc, leads) with its rows, thresholds and pieces."""
import ctypes as C
import functools

import numpy as np
import pytest

import kmersgwas_amd as kg
from kmersgwas_amd import capi
from kmersgwas_amd.capi import lib

import clump_np as CN
import proxy_np as PN

pytestmark = pytest.mark.gpu
N_ACC = (5, 64, 67, 128, 129, 513, 1135)
N_LEADS = (1, 17, 64, 65, 130)
N_ROWS = (1, 127, 128, 129, 300, 1000)
TM = (1000000, 800000, 250000, 1)
PIECES = (128, 256)
# places of the special rows among the rows (R >= 17) and among the leads (L >= 17)
COPY, COMPLEMENT, NEAR, ALL0, ALL1, ON_B, ON_NEAR = 3, 5, 6, 7, 8, 10, 11
L_ALL0, L_ALL1, L_ON_A = 2, 4, 9


@functools.lru_cache(maxsize=None)
def tables(n, L, R):
    """(lead bits [L, n], row bits [R, n]); lead 0 varies and row R - 1 is a copy of it"""
    rng = np.random.default_rng([n, L, R])
    dens = np.array([0.5, 0.02, 0.2, 0.8, 0.97])
    leads = rng.random((L, n)) < dens[np.arange(L) % 5][:, None]
    rows = rng.random((R, n)) < dens[(np.arange(R) + 1) % 5][:, None]
    leads[0, :2] = rows[0, :2] = [True, False]  # lead 0 and row 0 vary
    rows[R - 1] = leads[0]
    if L >= 17:
        leads[L_ALL0], leads[L_ALL1] = False, True
        leads[L - 1] = rows[0]  # the last lead, in another tile where there is one, finds the first row
    if R >= 17:
        rows[COPY], rows[COMPLEMENT], rows[NEAR] = leads[0], ~leads[0], leads[0]
        rows[NEAR, n - 1] ^= True
        rows[ALL0], rows[ALL1] = False, True
    if L >= 17 and R >= 17 and n in (64, 128):
        a, b = CN.pair_with(n, n // 2, n // 2, 3 * n // 8)
        leads[L_ON_A], rows[ON_B], rows[ON_NEAR], rows[R - 2] = a, b, CN.one_bit_moved(a, b), b
    leads.setflags(write=False), rows.setflags(write=False)
    return leads, rows


@functools.lru_cache(maxsize=8)
def num_den(n, L, R):
    return PN.num_den(*tables(n, L, R))


@functools.lru_cache(maxsize=None)
def model(n, L, R, tm):
    rec = PN.records(*tables(n, L, R), tm, nd=num_den(n, L, R))
    rec.setflags(write=False)
    return rec


def pairs(rec):
    return set(zip(rec["row"].tolist(), rec["lead"].tolist()))


def check_fixture(n, L, R):
    """the tables hold what the docstring says, by the model"""
    one, quarter = pairs(model(n, L, R, 1000000)), pairs(model(n, L, R, 250000))
    assert (R - 1, 0) in one, "the copy in the last row is not found at r2 = 1"
    if R >= 17:
        assert {(COPY, 0), (COMPLEMENT, 0)} <= one and (NEAR, 0) not in one
        assert not [p for p in pairs(model(n, L, R, 1)) if p[0] in (ALL0, ALL1)], "a constant row is found"
    if L >= 17:
        assert (0, L - 1) in one and not [p for p in pairs(model(n, L, R, 1)) if p[1] in (L_ALL0, L_ALL1)], "a constant lead finds"
    if L >= 17 and R >= 17 and n in (64, 128):
        assert {(ON_B, L_ON_A), (R - 2, L_ON_A)} <= quarter and (ON_NEAR, L_ON_A) not in quarter
        assert (ON_B, L_ON_A) not in pairs(model(n, L, R, 250001))


def differ(got, exp, what):
    if got.tobytes() != exp.tobytes():
        k = next((i for i in range(min(len(got), len(exp))) if got[i] != exp[i]), min(len(got), len(exp)))
        raise AssertionError("%s: %d records, the model has %d; the first difference at %d: %s, the model has %s"
                             % (what, len(got), len(exp), k, got[k] if k < len(got) else None, exp[k] if k < len(exp) else None))


@pytest.mark.parametrize("n", N_ACC)
@pytest.mark.parametrize("L", N_LEADS)
def test_records_equal_the_model(monkeypatch, n, L):
    for R in N_ROWS:
        check_fixture(n, L, R)
        records_equal_the_model(monkeypatch, n, L, R)


def records_equal_the_model(monkeypatch, n, L, R):
    leads, rows = tables(n, L, R)
    lw, rw = CN.pack_rows(leads), CN.pack_rows(rows)
    # garbage at and past n_acc, and words past the ones in use
    dirty = [np.concatenate([w, np.full((len(w), 2), 0xDEADBEEFDEADBEEF, np.uint64)], axis=1) for w in (lw, rw)]
    if n % 64:
        for w in dirty:
            w[:, n // 64] |= np.uint64((1 << 64) - (1 << (n % 64)))
    for piece in PIECES if R > 128 else PIECES[:1]:
        monkeypatch.setenv("KGWAS_PROXY_PIECE_ROWS", str(piece))
        for tm in TM:
            exp = model(n, L, R, tm)
            text = "%d.%06d" % (tm // 1000000, tm % 1000000)
            for a, b in ((lw, rw), dirty) if piece == PIECES[0] else ((lw, rw),):
                got, count = kg.kmers_ld_proxies(a, b, n, text)
                what = "n_acc=%d leads=%d rows=%d tm=%d piece=%d%s" % (n, L, R, tm, piece, " (garbage past n_acc)" if a is not lw else "")
                assert count == len(exp), what + ": %d records, the model has %d" % (count, len(exp))
                differ(got, exp, what)
                # (stated on their own, whatever the model says)
                order = got["row"].astype(np.int64) * 4096 + got["lead"]
                assert (np.diff(order) > 0).all(), what + ": the records are not in (row, lead) order"
                assert (got["kmer"] == 0).all() and (got["pad"] == 0).all() and (got["row"] < R).all() and (got["lead"] < L).all(), what


@pytest.mark.parametrize("n,L,R,records", [(67, 130, 1000, 1000), (128, 130, 1000, 4097), (5, 65, 129, 1), (1135, 17, 1000, 333)])
def test_a_small_record_buffer_is_drained_in_rounds(monkeypatch, n, L, R, records):
    """130 x 1000 pairs of which nearly all link, through a device buffer of 1000 records: a piece of 256 rows holds about 30 000, a
    single block of the compaction more than the buffer, a single row up to 130"""
    monkeypatch.setenv("KGWAS_PROXY_RECORDS", str(records))
    monkeypatch.setenv("KGWAS_LD_TIMING", "1")
    leads, rows = tables(n, L, R)
    for piece in PIECES:
        monkeypatch.setenv("KGWAS_PROXY_PIECE_ROWS", str(piece))
        for tm in (1, 250000):
            exp = model(n, L, R, tm)
            got, count = kg.kmers_ld_proxies(CN.pack_rows(leads), CN.pack_rows(rows), n, "%.6f" % (tm / 1e6))
            assert count == len(exp)
            differ(got, exp, "n_acc=%d leads=%d rows=%d tm=%d piece=%d records=%d" % (n, L, R, tm, piece, records))
    assert len(model(n, L, R, 1)) > 3 * records, "the fixture does not need several rounds"


def test_a_cap_below_the_count(monkeypatch):
    n, L, R = 67, 65, 300
    monkeypatch.setenv("KGWAS_PROXY_PIECE_ROWS", "128")
    leads, rows = tables(n, L, R)
    exp = model(n, L, R, 250000)
    assert len(exp) > 40
    lw, rw = CN.pack_rows(leads), CN.pack_rows(rows)
    for cap in (0, 1, 40, len(exp) - 1, len(exp), len(exp) + 5):
        rec = np.zeros(cap + 3, kg.PROXY_RECORD)  # (three records of room behind cap: they must stay)
        rec[:] = (7, 7, 7, 7, 7, 7)
        n_out = C.c_uint64(0)
        rc = lib.kgwas_kmers_ld_proxies(capi.ptr(lw), L, capi.ptr(rw), R, lw.shape[1], n, 250000, 0, capi.ptr(rec) if cap else None, cap, C.byref(n_out))
        assert rc == capi.KGWAS_OK and n_out.value == len(exp), (cap, n_out.value)
        k = min(cap, len(exp))
        assert rec[:k].tobytes() == exp[:k].tobytes() and (rec[k:]["lead"] == 7).all(), cap
    got, count = kg.kmers_ld_proxies(lw, rw, n, "0.25", cap=40)
    assert count == len(exp) and got.tobytes() == exp[:40].tobytes()


@pytest.mark.parametrize("n,L,R", [(67, 130, 300), (128, 65, 1000), (1135, 17, 129)])
def test_popcount_ablation_has_the_same_bytes(monkeypatch, n, L, R):
    monkeypatch.setenv("KGWAS_LD_POPCOUNT", "1")
    monkeypatch.setenv("KGWAS_PROXY_PIECE_ROWS", "256")
    leads, rows = tables(n, L, R)
    for tm in (800000, 250000, 1):
        got, count = kg.kmers_ld_proxies(CN.pack_rows(leads), CN.pack_rows(rows), n, "%.6f" % (tm / 1e6))
        assert count == len(model(n, L, R, tm))
        differ(got, model(n, L, R, tm), "popcount n_acc=%d leads=%d rows=%d tm=%d" % (n, L, R, tm))


def test_largest_accession_count():
    """n_acc = 8192, the most the predicate's integers are sized for, with a handful of rows"""
    n = 8192
    rng = np.random.default_rng(8192)
    bits = rng.random((12, n)) < 0.5
    bits[1], bits[2], bits[3] = bits[0], ~bits[0], bits[0]
    bits[3, 8191] ^= True
    a, b = CN.pair_with(n, n // 2, n // 2, 3 * n // 8)
    bits[4], bits[5], bits[6] = a, b, CN.one_bit_moved(a, b)
    bits[7], bits[8] = False, True
    leads = bits[[0, 4, 7, 8, 9]]
    lw, rw = CN.pack_rows(leads), CN.pack_rows(bits)
    for text in ("1", "0.25", "0.250001", "0.999"):
        exp = PN.records(leads, bits, CN.millionths(text))
        got, count = kg.kmers_ld_proxies(lw, rw, n, text)
        assert count == len(exp)
        differ(got, exp, "n_acc=8192 r2=" + text)
    assert pairs(PN.records(leads, bits, 1000000)) == {(0, 0), (1, 0), (2, 0), (4, 1), (9, 4)}
    assert (5, 1) in pairs(PN.records(leads, bits, 250000)) and (6, 1) not in pairs(PN.records(leads, bits, 250000))
    assert (5, 1) not in pairs(PN.records(leads, bits, 250001))


def test_refusals():
    leads, bits, rec, n_out = np.zeros((4, 129), np.uint64), np.zeros((4, 129), np.uint64), np.zeros(8, kg.PROXY_RECORD), C.c_uint64(0)
    p = capi.ptr
    bad = [
        (p(leads), 4, p(bits), 4, 1, 0, p(rec), C.byref(n_out), "0 accessions"),
        (p(leads), 4, p(bits), 4, 129, 8193, p(rec), C.byref(n_out), "8193 accessions"),
        (p(leads), 4097, p(bits), 4, 1, 64, p(rec), C.byref(n_out), "4097 leads"),
        (None, 4, p(bits), 4, 1, 64, p(rec), C.byref(n_out), "null argument"),
        (p(leads), 4, None, 4, 1, 64, p(rec), C.byref(n_out), "null argument"),
        (p(leads), 4, p(bits), 4, 1, 64, None, C.byref(n_out), "null argument"),
        (p(leads), 4, p(bits), 4, 1, 64, p(rec), None, "null argument"),
        (p(leads), 4, p(bits), 4, 1, 65, p(rec), C.byref(n_out), "words_per_row is too small"),
    ]
    for a, L, b, R, words, n_acc, r, n_o, msg in bad:
        assert lib.kgwas_kmers_ld_proxies(a, L, b, R, words, n_acc, 500000, 0, r, 8, n_o) == capi.KGWAS_ERR_ARG, msg
        assert msg in lib.kgwas_last_error().decode(), lib.kgwas_last_error()
