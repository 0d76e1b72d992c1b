"""Shared by test_gpu_lmm_lrt_table.py and test_lmm_lrt_table_cli.py (test infrastructure, not product): small k-mers tables with
chosen presence counts, the tested-set rule of lmm_lrt --kmers_table restated in numpy, and the one fixture whose model gap the
CPU module asserts and whose statistics the GPU module checks against model E."""
import functools

import numpy as np

import lmm_lrt_np as M

K_LEN = 31
KIN_ROWS = {5: 400, 50: 400, 64: 400, 65: 400, 67: 400, 241: 600}  # rows of M.fixture's G, from which K comes


def kmer_text(word, k=K_LEN):
    """bits2kmer31: the most significant base first"""
    return "".join("ACGT"[(int(word) >> (2 * (k - 1 - i))) & 3] for i in range(k))


def table_from_bits(bits, S_f, pick, seed):
    """bits (rows x S, phenotype order) -> table rows [kmer, W_f words] with accession i of the phenotype order in column
    pick[i]; the other S_f - S columns get random bits; k-mer words ascending and unique."""
    bits = np.asarray(bits, bool)
    n_rows, S = bits.shape
    rng = np.random.default_rng([seed, S_f, n_rows])
    W = (S_f + 63) // 64
    pad = np.zeros((n_rows, W * 64), bool)
    pad[:, :S_f] = rng.random((n_rows, S_f)) < 0.5
    pad[:, np.asarray(pick)] = bits
    words = np.packbits(pad.reshape(n_rows, W, 64), axis=2, bitorder="little").view(np.uint64).reshape(n_rows, W)
    rows = np.empty((n_rows, 1 + W), np.uint64)
    rows[:, 0] = np.sort(rng.choice(1 << 40, size=n_rows, replace=False)).astype(np.uint64)
    rows[:, 1:] = words
    return rows


def random_bits(n_rows, S, seed, lo=0.01, hi=0.99):
    rng = np.random.default_rng([seed, S, n_rows, 3])
    f = rng.uniform(lo, hi, n_rows)
    return rng.random((n_rows, S)) < f[:, None]


def bits_with_counts(counts, S, seed):
    """one row per entry of counts, with exactly that many carriers, at random places"""
    rng = np.random.default_rng([seed, S, 5])
    bits = np.zeros((len(counts), S), bool)
    for r, c in enumerate(counts):
        bits[r, rng.permutation(S)[:c]] = True
    return bits


def tested_rule(n1, S, min_count, maf):
    """The rule in float64 numpy, operation for operation: kmers_table_to_bed's MAC filter and lmm_prep_kernel's af filter."""
    n1 = np.asarray(n1, np.int64)
    written = (S >= min_count) & (n1 >= min_count) & (n1 <= S - min_count)
    mean = (2 * (S - n1)).astype(np.float64) / np.float64(S)
    af = 0.5 * mean
    return written & (n1 != 0) & (n1 != S) & (np.minimum(af, 1.0 - af) >= maf)


def kinship_and_phenotype(S):
    _, K, y = M.fixture(S, KIN_ROWS[S], 3.0)
    return K, y


# ---- the fixture checked against model E: S = 67 of a table of 70 accessions, 40 rows that are all tested at MAC 5, MAF 0.05 ----
MODEL_S, MODEL_S_F, MODEL_ROWS, MODEL_MIN_COUNT, MODEL_MAF = 67, 70, 40, 5, 0.05


@functools.lru_cache(maxsize=None)
def model_fixture():
    """(K, y, bits, pick, rows): bits 40 x 67 in phenotype order, frequencies 0.2 .. 0.8"""
    K, y = kinship_and_phenotype(MODEL_S)
    bits = random_bits(MODEL_ROWS, MODEL_S, 77, 0.2, 0.8)
    pick = np.random.default_rng(77).permutation(MODEL_S_F)[:MODEL_S]
    return K, y, bits, pick, table_from_bits(bits, MODEL_S_F, pick, 77)


def model_dosages(bits):
    """the .bed's values: absence 2, presence 0"""
    return 2.0 * (1.0 - np.asarray(bits, np.float64))
