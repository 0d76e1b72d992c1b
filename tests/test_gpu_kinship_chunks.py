"""emma_kinship_kmers' session (kin_kernels.hip, kinship.cpp) across chunks of a device feed and at the widths its tiles and its
transpose's LDS decide, against the closed form K_ij = n - c_i - c_j + 2 c_ij (tests/exact_topn.py), computed blockwise in NumPy."""
import numpy as np
import pytest

import kmersgwas_amd as kg
import exact_topn as ex
from helpers import random_table, synth_rows_numpy

pytestmark = pytest.mark.gpu


class ClosedForm:
    """kinship_closed_form, summed block by block: (c = G^T G, n) over the rows that pass the MAF predicate."""

    def __init__(self, S_f, maf=0.05):
        self.S_f, self.mc = S_f, int(np.ceil(S_f * maf))
        self.c = np.zeros((S_f, S_f), np.int64)
        self.n = 0

    def add(self, rows, block=1 << 18):
        for r0 in range(0, len(rows), block):
            b = ex._bits(rows[r0: r0 + block], self.S_f)
            n1 = b.sum(axis=1, dtype=np.int64)
            g = b[(n1 >= self.mc) & (n1 <= self.S_f - self.mc)].astype(np.float64)  # 0/1, sums below 2^53: exact
            self.c += (g.T @ g).astype(np.int64)
            self.n += len(g)

    def check(self, kin):
        """The session's lower triangle (j < i) equals n - c_ii - c_jj + 2 c_ij, row block by row block."""
        Kg, ng = kin.matrix()
        assert ng == self.n
        ci = np.diag(self.c)
        for i0 in range(0, self.S_f, 512):
            i1 = min(self.S_f, i0 + 512)
            K = self.n - ci[i0:i1, None] - ci[None, :] + 2 * self.c[i0:i1]
            low = np.arange(self.S_f)[None, :] < np.arange(i0, i1)[:, None]
            got = np.asarray(Kg[i0:i1], np.int64)
            assert (got[low] == K[low]).all(), "rows %d..%d differ" % (i0, i1)
            assert (Kg[i0:i1][~low] == 0).all()


def test_feed_device_across_chunks_unsynchronised():
    """3 * 2^20 + 777 rows written by synth_rows_device on the caller's stream and fed at once, with no synchronisation (the
    session orders its chunks after the caller's stream): four chunks, the two plane buffers alternating. A second buffer is
    then fed into the same session."""
    import torch
    S_f, seed = 200, 61
    stride = 1 + (S_f + 63) // 64
    st_ = torch.cuda.current_stream().cuda_stream
    n1, n2 = 3 * (1 << 20) + 777, (1 << 20) + 5
    a = torch.empty(n1 * stride, dtype=torch.int64, device="cuda")
    b = torch.empty(n2 * stride, dtype=torch.int64, device="cuda")
    cf = ClosedForm(S_f)
    kin = kg.Kinship(S_f, cf.mc)
    kg.synth_rows_device(a.data_ptr(), 0, n1, S_f, seed, st_)
    kin.feed_device(a.data_ptr(), n1, st_)
    kg.synth_rows_device(b.data_ptr(), n1, n2, S_f, seed, st_)
    kin.feed_device(b.data_ptr(), n2, st_)
    assert kin.stats()["launches"] == 4 + 2
    torch.cuda.synchronize()
    rows_a = a.cpu().numpy().view(np.uint64).reshape(n1, stride)
    assert (rows_a[:5] == synth_rows_numpy(0, 5, S_f, seed)).all() and (rows_a[-3:] == synth_rows_numpy(n1 - 3, 3, S_f, seed)).all()
    cf.add(rows_a)
    cf.add(b.cpu().numpy().view(np.uint64).reshape(n2, stride))
    cf.check(kin)
    kin.close()


@pytest.mark.parametrize("S_f", [127, 128, 129, 255, 256, 257, 8000, 10_112])
def test_kinship_widths(S_f):
    """Tile edges (S_pad = 128 and 256 and one accession either side), 8000 accessions and 10 112, the widest session the
    transpose's LDS accepts."""
    n_rows = 3000 if S_f < 1000 else 1500
    rows = random_table(n_rows, S_f, seed=S_f + 5)
    cf = ClosedForm(S_f)
    cf.add(rows)
    kin = kg.Kinship(S_f, cf.mc)
    kin.feed_host(rows[: n_rows // 2])
    kin.feed_host(rows[n_rows // 2:])
    cf.check(kin)
    kin.close()


def test_kinship_width_limit():
    """One accession past 10 112: refused when the session is created, with the limit in the message."""
    with pytest.raises(kg.KgwasError) as e:
        kg.Kinship(10_113, 506)
    assert e.value.code == kg.capi.KGWAS_ERR_ARG and "at most 10112" in e.value.msg
