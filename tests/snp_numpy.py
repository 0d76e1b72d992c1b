"""A third statement of the SNP scorer, in NumPy (test infrastructure, not product).

MultipleSNPsDataBases (src/snps_multiple_databases.cpp) scores a SNP for one phenotype column as follows.
- Every phenotyped sample si (phenotype order) reads the dubit (bed[snp][byte(si)] >> shift(si)) & 3 of its .fam position:
  00 homozygous minor, 01 missing, 10 heterozygous, 11 homozygous major.
- Three bit planes over si, padded with zeros to 2 * ceil(S / 128) 64-bit words: presence (11), non-missing (not 01)
  and heterozygous (10). Per SNP: S_gi = #11 + #10 / 2, S_gi_2 = #11 + #10 / 4, N = #non-missing (all exact in double).
- dot_product_SSE4 of a plane: every 128-bit block of two words is four 32-bit lanes; lane l of block b covers samples
  128 b + 32 l .. + 31, and step s (0..31) takes the bit 31 - s of every lane first (blendv reads the sign bit, then the mask
  shifts left by one). Each lane adds the phenotype value of its selected sample (or +0.0) to its own float32 sum, so lane l
  sums, in order, samples 128 b + 32 l + 31 - s over b, then s. The four lane sums are added in float32 as
  ((l0 + l1) + l2) + l3 and widened to double.
- calculate_grammmar_approx_association: 0 if mac > S_gi or mac > N - S_gi; otherwise, in double without contraction,
  yigi = dot(presence) + dot(het) * 0.5, r = N * yigi - S_gi * dot(non-missing), score = (r * r) / (N * (N * S_gi_2 - S_gi * S_gi)).
"""
import numpy as np


def dubits(body, n_samples_file, sample_index):
    """dubits[snp][si] of a .bed body (bytes after the magic) for the .fam positions sample_index (phenotype order)."""
    bps = (n_samples_file + 3) // 4
    body = np.frombuffer(bytes(body), np.uint8).reshape(-1, bps) if not isinstance(body, np.ndarray) else body.reshape(-1, bps)
    idx = np.asarray(sample_index, np.int64)
    return (body[:, idx // 4] >> ((idx % 4) * 2).astype(np.uint8)) & np.uint8(3)


def lane_dot(plane, y):
    """dot_product_SSE4 of bool planes[n_snps][S] against float32 y[S], for every SNP: a float64 array."""
    n, S = plane.shape
    L = 128 * ((S + 127) // 128)
    bits = np.zeros((n, L), bool)
    bits[:, :S] = plane
    v = np.zeros(L, np.float32)
    v[:S] = y
    acc = np.zeros((n, 4), np.float32)
    zero = np.float32(0.0)
    with np.errstate(all="ignore"):
        for b in range(L // 128):
            for s in range(32):
                cols = 128 * b + 32 * np.arange(4) + 31 - s  # lane l's sample at this step
                acc = acc + np.where(bits[:, cols], v[cols][None, :], zero)
        f = acc[:, 0] + acc[:, 1]
        f = f + acc[:, 2]
        f = f + acc[:, 3]
    return f.astype(np.float64)


def snps_scores(body, n_samples_file, sample_index, y, mac):
    """calculate_grammmar_approx_association of every SNP (float64[n_snps]) for phenotype y (float32, phenotype order)."""
    d = dubits(body, n_samples_file, sample_index)
    pres, tot, het = d == 3, d != 1, d == 2
    S_gi = pres.sum(axis=1).astype(np.float64) + 0.5 * het.sum(axis=1)
    S_gi_2 = pres.sum(axis=1).astype(np.float64) + 0.25 * het.sum(axis=1)
    N = tot.sum(axis=1).astype(np.float64)
    y = np.asarray(y, np.float32)
    with np.errstate(all="ignore"):
        yigi = lane_dot(pres, y) + lane_dot(het, y) * 0.5
        score_sum = lane_dot(tot, y)
        p1 = N * yigi
        p2 = S_gi * score_sum
        r = p1 - p2
        r = r * r
        q1 = N * S_gi_2
        q2 = S_gi * S_gi
        den = N * (q1 - q2)
        out = r / den
    fail = (mac > S_gi) | (mac > (N - S_gi))
    out[fail] = 0.0
    return out
