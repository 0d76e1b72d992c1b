"""Kernel and copy time of kgwas_kmers_ld_proxies: the kernels alone (prep + link + compact) and the pieces'
host-to-device copies, by the events the library puts around them (KGWAS_LD_TIMING=1), for the matrix-core link kernel and for
the popcount(AND) ablation (KGWAS_LD_POPCOUNT=1) on the same rows.

Rows are synthetic table rows made on the device (kgwas_synth_rows_device) and brought to the host once; the leads are rows of
theirs, evenly spaced, so every lead finds at least itself. Each configuration runs in a process of its own: one warm-up call, then
--repeat timed calls. Appends one JSON line per configuration to --out and prints it: the median kernel and copy time, the pairs
per second and the fraction of the FP4 MFMA peak (2 * 128 * ceil(n_acc / 128) * leads_padded * rows operations counted).

  python tools/time_proxy_kmers.py --leads 256,4096 --rows 4194304 --acc 1135 [--popcount_rows 524288] [--repeat 3]
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


def child(L, R, n, repeat):
    import torch

    import kmersgwas_amd as kg
    W = (n + 63) // 64
    d = torch.empty((R, 1 + W), dtype=torch.int64, device="cuda")
    kg.synth_rows_device(d.data_ptr(), 0, R, n, 7)
    torch.cuda.synchronize()
    bits = np.ascontiguousarray(d.cpu().numpy().view(np.uint64)[:, 1:])
    del d
    torch.cuda.empty_cache()
    leads = np.ascontiguousarray(bits[np.arange(L) * (R // L)])
    # the tool's pieces come from pinned buffers (PieceReader): the rows are pinned here too, so that copy_ms is such a copy's
    try:
        pinned = int(torch.cuda.cudart().cudaHostRegister(bits.ctypes.data, bits.nbytes, 0)) == 0
    except RuntimeError:
        pinned = False
    print("pinned=%d" % pinned, file=sys.stderr, flush=True)
    for _ in range(1 + repeat):
        t0 = time.perf_counter()
        rec, count = kg.kmers_ld_proxies(leads, bits, n, "0.8", cap=1 << 16)
        print("wall_ms=%.3f found=%d" % (1e3 * (time.perf_counter() - t0), count), file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leads", default="256,4096")
    ap.add_argument("--rows", type=int, default=1 << 22)
    ap.add_argument("--popcount_rows", type=int, default=1 << 19, help="rows of the ablation's runs (it is slow; pairs per second are compared)")
    ap.add_argument("--acc", type=int, default=1135)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--peak_pflops", type=float, default=10.0, help="dense FP4 MFMA peak of the device, PFLOP/s")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "proxy_kmers_time.jsonl"))
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        L, R = [int(x) for x in a.child.split(",")]
        return child(L, R, a.acc, a.repeat)
    for L in [int(x) for x in a.leads.split(",")]:
        for popcount in (False, True):
            R = a.popcount_rows if popcount else a.rows
            env = dict(os.environ, KGWAS_LD_TIMING="1")
            env.pop("KGWAS_LD_POPCOUNT", None)
            if popcount:
                env["KGWAS_LD_POPCOUNT"] = "1"
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "%d,%d" % (L, R), "--acc", str(a.acc), "--repeat", str(a.repeat)],
                               env=env, capture_output=True, text=True, timeout=1100)
            if r.returncode != 0:
                print(r.stderr[-3000:], file=sys.stderr)
                sys.exit(1)
            ms = [float(x) for x in re.findall(r"kernels_ms=([0-9.]+)", r.stderr)][1:]
            copy = [float(x) for x in re.findall(r"copy_ms=([0-9.]+)", r.stderr)][1:]
            wall = [float(x) for x in re.findall(r"wall_ms=([0-9.]+)", r.stderr)][1:]
            med = float(np.median(ms))
            ops = 2.0 * 128 * ((a.acc + 127) // 128) * ((L + 63) // 64 * 64) * R
            line = json.dumps({"leads": L, "rows": R, "acc": a.acc, "n11": "popcount" if popcount else "mfma", "kernel_ms": ms,
                               "kernel_ms_median": round(med, 3), "copy_ms_median": round(float(np.median(copy)), 3),
                               "wall_ms_median": round(float(np.median(wall)), 1), "pairs_per_s": round(L * R / (med * 1e-3), 0),
                               "fp4_peak_fraction": round(ops / (med * 1e-3) / (a.peak_pflops * 1e15), 4),
                               "found": re.findall(r"found=(\d+)", r.stderr)[-1], "rows_pinned": "pinned=1" in r.stderr})
            print(line, flush=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
