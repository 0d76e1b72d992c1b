"""clump_np.py, the model the GPU tests of clump_kmers compare bytes with, checked on its own: the integer predicate against
numpy's correlation away from the threshold, exactly on the threshold and one bit beside it, and the clump pass's properties."""
import numpy as np
import pytest

import clump_np as CN


def random_rows(N, n, seed):
    rng = np.random.default_rng([seed, N, n])
    f = rng.choice([0.05, 0.3, 0.5, 0.9], N)
    bits = rng.random((N, n)) < f[:, None]
    # families: noisy copies of earlier rows, so that r2 covers (0, 1) and not only its low end
    for r in range(N // 2, N):
        src = bits[rng.integers(0, N // 2)]
        bits[r] = src ^ (rng.random(n) < rng.choice([0.0, 0.02, 0.1]))
    return bits


@pytest.mark.parametrize("N,n,text", [(60, 67, "0.8"), (60, 128, "0.25"), (40, 1135, "0.5"), (80, 5, "0.000001"), (50, 64, "1")])
def test_predicate_against_corrcoef(N, n, text):
    bits = random_rows(N, n, 1)
    tm = CN.millionths(text)
    linked, n1, _ = CN.linked_matrix(bits, tm)
    varies = (n1 > 0) & (n1 < n)
    with np.errstate(invalid="ignore", divide="ignore"):
        r2 = np.corrcoef(bits.astype(np.float64)) ** 2
    t = tm / 1e6
    checked = 0
    for a in range(N):
        for b in range(N):
            if not (varies[a] and varies[b]):
                assert not linked[a, b], "a constant row is linked"
            elif abs(r2[a, b] - t) > 1e-9:
                assert linked[a, b] == (r2[a, b] > t), (a, b, r2[a, b])
                checked += 1
    assert checked > N and linked.any() and not linked.all()
    assert (linked == linked.T).all()


@pytest.mark.parametrize("n,ca,cb,n11,text", CN.ON_THRESHOLD)
def test_on_the_threshold_is_linked(n, ca, cb, n11, text):
    a, b = CN.pair_with(n, ca, cb, n11)
    tm = CN.millionths(text)
    assert (n * n11 - ca * cb) ** 2 * 1000000 == tm * ca * (n - ca) * cb * (n - cb), "the fixture is not on its threshold"
    adj, n1 = CN.links(CN.pack_rows(np.stack([a, b])), n, tm)
    assert n1.tolist() == [ca, cb] and CN.adj_bit(adj, 0, 1)
    assert adj[1, 0] == 0 and not CN.adj_bit(adj, 0, 0), "the diagonal or the lower triangle is set"
    c = CN.one_bit_moved(a, b)
    assert c.sum() == cb and (a & c).sum() == n11 - 1
    adj, _ = CN.links(CN.pack_rows(np.stack([a, c])), n, tm)
    assert not CN.adj_bit(adj, 0, 1), "one bit beside the threshold is still linked"
    adj, _ = CN.links(CN.pack_rows(np.stack([a, b])), n, tm + 1)
    assert not CN.adj_bit(adj, 0, 1), "a millionth above the pair's r2 is still linked"


@pytest.mark.parametrize("n", [5, 64, 128, 1135, 8192])
def test_identical_and_complementary_rows_at_one(n):
    rng = np.random.default_rng(n)
    a = rng.random(n) < 0.4
    a[:2] = [True, False]
    near = a.copy()
    near[-1] = not near[-1]
    rows = np.stack([a, a.copy(), ~a, near, np.zeros(n, bool), np.ones(n, bool)])
    adj, n1 = CN.links(CN.pack_rows(rows), n, 1000000)
    assert CN.adj_bit(adj, 0, 1) and CN.adj_bit(adj, 0, 2) and CN.adj_bit(adj, 1, 2)
    assert not CN.adj_bit(adj, 0, 3) and not CN.adj_bit(adj, 2, 3), "one bit apart is linked at r2 = 1"
    for const in (4, 5):
        assert not any(CN.adj_bit(adj, r, const) for r in range(const)) and not adj[const].any(), "a constant row is linked"
    assert n1.tolist() == [int(r.sum()) for r in rows]


def test_garbage_past_n_is_dropped():
    bits = random_rows(20, 67, 2)
    words = CN.pack_rows(bits, 3)
    dirty = words.copy()
    dirty[:, 1] |= np.uint64(0xFFFFFFFFFFFFFFF8)  # bits 67 .. 127
    dirty[:, 2] = np.uint64(0xDEADBEEFDEADBEEF)
    for x, y in zip(CN.links(words, 67, 500000), CN.links(dirty, 67, 500000)):
        assert x.tobytes() == y.tobytes()


def test_millionths():
    assert [CN.millionths(t) for t in ("1", "0.8", "0.000001", "0.25", ".5")] == [1000000, 800000, 1, 250000, 500000]


@pytest.mark.parametrize("seed,text", [(0, "0.8"), (1, "0.3"), (2, "1"), (3, "0.000001")])
def test_clump_properties(seed, text):
    N, n = 90, 67
    bits = random_rows(N, n, 10 + seed)
    rng = np.random.default_rng(seed)
    p = rng.choice(["1e-9", "3.5e-08", "0.001", "2e-5", "1.000000e-03", "0.5"], N)  # many ties, two texts of one value
    tm = CN.millionths(text)
    order = CN.p_order(p)
    assert sorted(order) == list(range(N))
    adj, _ = CN.links(CN.pack_rows(bits[order]), n, tm)
    lead_of, leads = CN.clump(order, adj)
    linked, _, _ = CN.linked_matrix(bits, tm)
    key = lambda h: (float(p[h]), h)
    assert sorted(lead_of) == list(range(N)), "a hit is in no clump"
    assert all(lead_of[l] == l for l in leads) and len(set(leads)) == len(leads)
    assert set(lead_of.values()) == set(leads), "every hit is in exactly one clump, and every clump has its lead"
    for h, l in lead_of.items():
        assert h == l or linked[h, l], "a member is not linked to its lead"
        assert key(l) <= key(h), "a lead is not the first of its clump"
    for i, a in enumerate(leads):
        for b in leads[i + 1:]:
            assert not linked[a, b], "two leads are linked"
    assert [key(l) for l in leads] == sorted(key(l) for l in leads), "the leads are not in p order"
    if text != "1":
        assert len(leads) < N, "nothing was clumped"
    # the output: a line per hit in file order, leads with r2 1.000000 (nan for a constant row)
    rs = ["K%03d" % h for h in range(N)]
    lines = CN.format(rs, list(p), bits, lead_of, leads).decode().split("\n")
    assert lines[0] + "\n" == CN.HEADER and lines[-1] == "" and len(lines) == N + 2
    for h, line in enumerate(lines[1:-1]):
        f = line.split("\t")
        assert f[0] == rs[h] and f[1] == p[h] and f[3] == rs[lead_of[h]] and int(f[2]) == leads.index(lead_of[h]) + 1
        if lead_of[h] == h:
            assert f[4] in ("1.000000", "nan") and f[5] == f[6]
    assert CN.run(rs, list(p), bits, tm) == "\n".join(lines).encode()


def test_p_max_and_ties():
    bits = np.zeros((4, 8), bool)
    bits[:, :4] = True  # four copies of one pattern
    rs, p = ["A", "B", "C", "D"], ["0.5", "1e-3", "0.001", "0.9"]
    out = CN.run(rs, p, bits, 1000000, p_max=0.5).decode().split("\n")
    # B and C tie: the earlier line leads; D is cut
    assert out[1:-1] == ["A\t0.5\t1\tB\t1.000000\t4\t4", "B\t1e-3\t1\tB\t1.000000\t4\t4", "C\t0.001\t1\tB\t1.000000\t4\t4"]
