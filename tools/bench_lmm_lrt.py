#!/usr/bin/env python3
"""Synthetic benchmark of lmm_lrt at the size of one kmers_gwas.py run: 101 .bed files (1 phenotype + 100 permutations) x 10 001
k-mers x 1135 individuals against one kinship matrix. Self-contained: seeded data, no files.

Prints one JSON line: the host eigendecomposition and the rotation / grid / refinement kernels' milliseconds (summed over the
101 files), the wall time, and the rotation's fp64 rate (2 n^2 flop per variant) as a fraction of the MI355X's FP64 matrix peak.
The microarchitecture notes this project works from list no FP64 matrix figure; AMD's published 78.6 TFLOP/s is used.
There is no GEMMA timing to set beside these numbers: GEMMA is not installed where this was measured.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kmersgwas_amd as kg  # noqa: E402

FP64_MATRIX_PEAK_TFLOPS = 78.6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--beds", type=int, default=101)
    ap.add_argument("--variants", type=int, default=10001)
    ap.add_argument("--individuals", type=int, default=1135)
    ap.add_argument("--chunk_variants", type=int, default=10240)
    a = ap.parse_args()
    n, m = a.individuals, a.variants
    rng = np.random.default_rng(20240601)
    rows = 2 * n
    G = (rng.random((rows, n)) < rng.uniform(0.1, 0.9, rows)[:, None]).astype(np.float64)
    K = 1.0 - (G.T @ (1 - G) + (1 - G).T @ G) / rows
    d, U = np.linalg.eigh(K)
    y = rng.standard_normal(n) + 1.5 * ((U * np.sqrt(np.clip(d, 0, None))) @ rng.standard_normal(n)) + 1.2 * G[7]
    bps = (n + 3) // 4
    t0 = time.perf_counter()
    lmm = kg.LmmLrt(K, chunk_variants=a.chunk_variants)
    t_create = time.perf_counter() - t0
    t_test = 0.0
    tested = 0
    for b in range(a.beds):
        yy = y if b == 0 else rng.permutation(y)
        bits = rng.random((m, bps * 4)) < rng.uniform(0.06, 0.94, m)[:, None]  # presence: code 00, absence: code 11
        c = np.where(bits, 0, 3).astype(np.uint8).reshape(m, bps, 4)
        bed = c[:, :, 0] | (c[:, :, 1] << 2) | (c[:, :, 2] << 4) | (c[:, :, 3] << 6)
        t1 = time.perf_counter()
        r = lmm.test(bed, yy, maf=0.05, miss=0.5)
        t_test += time.perf_counter() - t1
        tested += int(r["tested"].sum())
    st = lmm.stats()
    lmm.close()
    flop = 2.0 * n * n * st["variants_read"]
    tf = flop / (st["rotate_ms"] * 1e-3) / 1e12 if st["rotate_ms"] else 0.0
    print(json.dumps({
        "beds": a.beds, "variants_per_bed": m, "individuals": n, "variants_tested": tested,
        "eigen_ms": round(st["eigen_ms"], 3), "rotate_ms": round(st["rotate_ms"], 3), "grid_ms": round(st["grid_ms"], 3),
        "refine_ms": round(st["refine_ms"], 3), "create_s": round(t_create, 3), "test_wall_s": round(t_test, 3),
        "rotate_tflops": round(tf, 3), "rotate_fraction_of_fp64_matrix_peak": round(tf / FP64_MATRIX_PEAK_TFLOPS, 4),
    }))


if __name__ == "__main__":
    main()
