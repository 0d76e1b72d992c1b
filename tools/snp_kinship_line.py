"""Rate of emma_kinship on the GPU (kgwas_snpkin_*): one JSON line per sample count.

Writes a seeded synthetic PLINK .bed/.fam (5 % missing, 5 % het calls; a pool of distinct SNPs is cycled, the kernel's work
does not depend on the values) and times, with the device synchronised at the end of every feed:
  feed_file_s  open + feed_file + sums: the .bed streamed from the file (read, copy and kernels overlapped)
  resident_s   feed_bed of the whole body already in host memory (copy and kernels only)
  cli_s        wall time of bin/emma_kinship on the files, stdout to /dev/null
and reports pair.SNP updates/s = S(S-1)/2 x used SNPs / resident_s and its share of the fp64 VALU issue bound
CUs x 4 SIMDs x 16 lanes x clock / (VALU instructions per pair.SNP of the accumulate kernel's ISA, --ops).

  python tools/snp_kinship_line.py --samples 1135 --snps 2000000 --samples 241
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_synthetic(base, S, M, seed, pool=4096):
    rng = np.random.default_rng(seed)
    q = rng.uniform(0.05, 0.95, size=(pool, 1))
    c = np.where(rng.random((pool, S)) < q, 3, 0)
    c = np.where(rng.random((pool, S)) < 0.05, 2, c)
    c = np.where(rng.random((pool, S)) < 0.05, 1, c)
    bps = (S + 3) // 4
    body = np.zeros((pool, bps), np.uint8)
    for s in range(S):
        body[:, s >> 2] |= (c[:, s].astype(np.uint8) << (2 * (s & 3)))
    with open(base + ".bed", "wb") as f:
        f.write(bytes([0x6C, 0x1B, 0x01]))
        left = M
        while left:
            n = min(left, pool)
            f.write(body[:n].tobytes())
            left -= n
    with open(base + ".fam", "w") as f:
        f.write("".join("s%d s%d 0 0 0 -9\n" % (i, i) for i in range(S)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, action="append", help="S (repeatable; default 1135 and 241)")
    ap.add_argument("--snps", type=int, default=2_000_000)
    ap.add_argument("--seed", type=int, default=20261016)
    ap.add_argument("--ops", type=float, default=None,
                    help="VALU instructions per pair.SNP (default: by rows per wave, counted in the gfx950 ISA: 4 -> 15.3, 8 -> 11.9)")
    ap.add_argument("--clock-mhz", type=float, default=2400.0)
    ap.add_argument("--cus", type=int, default=256)
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--dir", default=None)
    a = ap.parse_args()
    import kmersgwas_amd as kg
    import torch

    for S in a.samples or [1135, 241]:
        with tempfile.TemporaryDirectory(dir=a.dir) as d:
            base = os.path.join(d, "synth")
            write_synthetic(base, S, a.snps, a.seed + S)
            t0 = time.perf_counter()
            h = kg.SnpKinship(base)
            h.feed_file()
            torch.cuda.synchronize()
            sums_f, n_used = h.sums()
            t_file = time.perf_counter() - t0
            h.close()
            with open(base + ".bed", "rb") as f:
                body = np.frombuffer(f.read()[3:], np.uint8)
            h = kg.SnpKinship(base)
            h.feed_bed(body[: h.bytes_per_snp * 64])  # (first launches and buffers out of the timed region)
            h.close()
            h = kg.SnpKinship(base)
            t0 = time.perf_counter()
            h.feed_bed(body)
            torch.cuda.synchronize()
            t_res = time.perf_counter() - t0
            sums_r, n_r = h.sums()
            h.close()
            assert n_r == n_used and sums_r.tobytes() == sums_f.tobytes(), "feed_bed and feed_file disagree"
            t_cli = None
            if not a.no_cli:
                t0 = time.perf_counter()
                with open(os.devnull, "wb") as null:
                    subprocess.run([os.path.join(ROOT, "kmersgwas_amd", "bin", "emma_kinship"), base], stdout=null, stderr=subprocess.DEVNULL,
                                   check=True, timeout=900)
                t_cli = time.perf_counter() - t0
        rw = 8 if sum(1 for r0 in range(0, S, 8) for _ in range(0, min(r0 + 8, S) - 1, 64)) >= 2048 else 4
        ops = a.ops or {4: 15.3, 8: 11.9}[rw]
        pairs = S * (S - 1) // 2
        rate = pairs * n_used / t_res
        bound = a.cus * 4 * 16 * a.clock_mhz * 1e6 / ops
        print(json.dumps(dict(samples=S, snps=a.snps, snps_used=n_used, rows_per_wave=rw, feed_file_s=round(t_file, 4),
                              resident_s=round(t_res, 4), cli_s=None if t_cli is None else round(t_cli, 4),
                              pair_snp_updates_per_s=float("%.4g" % rate), valu_ops_per_pair_snp=ops,
                              bound_updates_per_s=float("%.4g" % bound), bound_s=round(pairs * n_used / bound, 4),
                              share_of_bound=round(rate / bound, 3))), flush=True)


if __name__ == "__main__":
    main()
