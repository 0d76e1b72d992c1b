"""Kernel time of kgwas_kmers_ld: the LD kernels alone, by the events the library puts around them
(KGWAS_LD_TIMING=1), for the matrix-core kernel and for the popcount(AND) ablation (KGWAS_LD_POPCOUNT=1) on the same rows.

Rows are random at mixed densities with families of noisy copies, as a list of hits is. Each configuration runs in a process of
its own: one warm-up call, then --repeat timed calls. Prints one JSON line per configuration with the median kernel time, the
pairs per second and the fraction of the FP4 MFMA peak (2 * 128 * ceil(n_acc / 128) * N^2 / 2 operations counted).

  python tools/time_kmers_ld.py --kmers 10001,131072 --acc 1135 [--repeat 5] [--peak_pflops 10.0]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(N, n, repeat):
    import kmersgwas_amd as kg
    rng = np.random.default_rng(N)
    base = rng.random((max(N // 8, 1), n)) < rng.uniform(0.05, 0.95, max(N // 8, 1))[:, None]
    bits = base[rng.integers(0, len(base), N)] ^ (rng.random((N, n)) < 0.02)
    W = (n + 63) // 64
    pad = np.zeros((N, W * 64), bool)
    pad[:, :n] = bits
    words = np.packbits(pad.reshape(N, W, 64), axis=2, bitorder="little").view(np.uint64).reshape(N, W)
    del bits, pad
    for _ in range(1 + repeat):
        t0 = time.perf_counter()
        adj, _ = kg.kmers_ld(words, n, "0.8")
        print("wall_ms=%.3f linked=%d" % (1e3 * (time.perf_counter() - t0), int(np.unpackbits(adj.view(np.uint8)).sum()) if N <= 20000 else -1),
              file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kmers", default="10001,131072")
    ap.add_argument("--acc", type=int, default=1135)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--peak_pflops", type=float, default=10.0, help="dense FP4 MFMA peak of the device, PFLOP/s")
    ap.add_argument("--child", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.acc, a.repeat)
    for N in [int(x) for x in a.kmers.split(",")]:
        for popcount in (False, True):
            env = dict(os.environ, KGWAS_LD_TIMING="1")
            env.pop("KGWAS_LD_POPCOUNT", None)
            if popcount:
                env["KGWAS_LD_POPCOUNT"] = "1"
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(N), "--acc", str(a.acc), "--repeat", str(a.repeat)],
                               env=env, capture_output=True, text=True, timeout=1100)
            if r.returncode != 0:
                print(r.stderr[-3000:], file=sys.stderr)
                sys.exit(1)
            ms = [float(x) for x in re.findall(r"kernels_ms=([0-9.]+)", r.stderr)][1:]
            wall = [float(x) for x in re.findall(r"wall_ms=([0-9.]+)", r.stderr)][1:]
            med = float(np.median(ms))
            ops = 2.0 * 128 * ((a.acc + 127) // 128) * N * N / 2
            print(json.dumps({"kmers": N, "acc": a.acc, "n11": "popcount" if popcount else "mfma", "kernel_ms": ms, "kernel_ms_median": round(med, 3),
                              "wall_ms_median": round(float(np.median(wall)), 1), "pairs_per_s": round(N * (N - 1) / 2 / (med * 1e-3), 0),
                              "fp4_peak_fraction": round(ops / (med * 1e-3) / (a.peak_pflops * 1e15), 4),
                              "linked": re.findall(r"linked=(-?\d+)", r.stderr)[-1]}), flush=True)


if __name__ == "__main__":
    main()
