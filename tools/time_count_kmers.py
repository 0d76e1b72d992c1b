"""Wall time of bin/count_kmers_with_strand on a synthetic accession in the page cache, and its kernels' time next to its copies'
(DESIGN.md §4.11).

Synthesises an accession: a random genome of --genome bases, reads of 150 bases at --coverage (half of them from the other strand),
0.5 % substitutions, written as FASTQ to --dir (a tmpfs or the page cache). The tool is timed end to end --repeat times (k = 31,
--ci 2); best and worst go to profiles/count_kmers_time.jsonl as one JSON line, with the tool's own trace line (passes, input and
count seconds) of the best run (--no-append: prints only). Two more timings bound the run from below: the tool with
KGWAS_COUNT_PARSE_ONLY=1 (the host parse and the upload, no counting), and what the input's bases take at 55 GB/s (the rate this
project measures for pinned pieces).

--profile DIR runs the tool once more under `rocprofv3 --kernel-trace --memory-copy-trace --stats` (no counters in that run) and
writes the summed time of the encode, sort, heads / reduce / compact kernels and of the copies, per pass, to
profiles/count_kmers_profile.jsonl, each with the bytes it moves over 8 TB/s beside it; the traces stay in DIR.

  python tools/time_count_kmers.py --genome 5000000 --coverage 30 [--dir /dev/shm/x] [--keep] [--profile /tmp/count_prof]
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_list_kmers import sum_traces  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "kmersgwas_amd", "bin", "count_kmers_with_strand")
K, L = 31, 150
HBM = 8e12


def write_fastq(path, genome_bases, coverage, seed=1):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    comp = np.frombuffer(bytes.maketrans(b"ACGT", b"TGCA"), np.uint8)
    genome = acgt[rng.integers(0, 4, size=genome_bases)]
    n_reads = genome_bases * coverage // L
    rec = 8 + 1 + L + 1 + 2 + L + 1  # "@" + 7 digits ... fixed-width records
    with open(path, "wb") as f:
        for r0 in range(0, n_reads, 1 << 18):
            n = min(1 << 18, n_reads - r0)
            m = genome[rng.integers(0, genome_bases - L, size=n)[:, None] + np.arange(L)[None, :]].copy()
            sub = rng.random(m.shape) < 0.005
            m[sub] = acgt[rng.integers(0, 4, size=int(sub.sum()))]
            m[::2] = comp[m[::2, ::-1]]
            out = np.full((n, rec), ord("I"), np.uint8)
            out[:, 0] = ord("@")
            ids = np.char.zfill((r0 + np.arange(n)).astype(str), 7).astype("S7")
            out[:, 1:8] = np.frombuffer(ids.tobytes(), np.uint8).reshape(n, 7)
            out[:, 8] = 10
            out[:, 9:9 + L] = m
            out[:, 9 + L] = 10
            out[:, 10 + L] = ord("+")
            out[:, 11 + L] = 10
            out[:, -1] = 10
            f.write(out.tobytes())
    return n_reads


def run_tool(cmd, env):
    t0 = time.perf_counter()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=3000, env=env)
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        print(r.stderr[-3000:], file=sys.stderr)
        sys.exit(1)
    return wall, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=5_000_000)
    ap.add_argument("--coverage", type=int, default=30)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--keep", action="store_true")
    ap.add_argument("--no-append", action="store_true")
    ap.add_argument("--profile", default=None)
    a = ap.parse_args()
    d = a.dir or tempfile.mkdtemp(prefix="ck_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    os.makedirs(d, exist_ok=True)
    fq = os.path.join(d, "reads_%d_%d.fq" % (a.genome, a.coverage))
    n_reads = a.genome * a.coverage // L
    if not os.path.exists(fq):
        need = n_reads * (2 * L + 13)
        if shutil.disk_usage(d).free < 1.3 * need:
            sys.exit("time_count_kmers: %s has too little room for %.1f GB of reads" % (d, need / 1e9))
        write_fastq(fq, a.genome, a.coverage)
    in_bytes = os.path.getsize(fq)
    with open(fq, "rb") as f:  # into the page cache
        while f.read(64 << 20):
            pass
    out = os.path.join(d, "out.sorted")
    cmd = [BIN, "-i", fq, "-k", str(K), "--ci", "2", "-o", out]
    env = dict(os.environ, KGWAS_TRACE="1")
    shape = {"genome": a.genome, "coverage": a.coverage, "reads": n_reads, "windows": n_reads * (L - K + 1), "input_bytes": in_bytes,
             "bases_bytes": n_reads * (L + 1)}
    runs = []
    for rep in range(a.repeat):
        wall, r = run_tool(cmd, env)
        trace = [l for l in r.stderr.splitlines() if l.startswith("[kgwas] count:")][0]
        runs.append((wall, trace, r.stdout.splitlines()[0]))
    parse = []
    for rep in range(min(a.repeat, 3)):
        wall, r = run_tool(cmd, dict(env, KGWAS_COUNT_PARSE_ONLY="1"))
        parse.append(wall)
    runs.sort()
    line = json.dumps(dict(shape, best_s=round(runs[0][0], 3), worst_s=round(runs[-1][0], 3), repeats=a.repeat, trace_of_best=runs[0][1],
                           kept=runs[0][2], output_bytes=os.path.getsize(out), parse_and_upload_only_best_s=round(min(parse), 3),
                           upload_at_55GBps_s=round(shape["bases_bytes"] / 55e9, 4)))
    print(line, flush=True)
    if not a.no_append:
        with open(os.path.join(ROOT, "profiles", "count_kmers_time.jsonl"), "a") as f:
            f.write(line + "\n")
    if a.profile:
        os.makedirs(a.profile, exist_ok=True)
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--memory-copy-trace", "--stats", "-f", "csv", "-d", a.profile, "--"] + cmd,
                           capture_output=True, text=True, timeout=3000, env=dict(env, KGWAS_CLI_FULL_TEARDOWN="1"))  # (the tool's
        # _exit would leave before the profiler writes its traces)
        if r.returncode != 0:
            print(r.stderr[-3000:], file=sys.stderr)
            sys.exit(1)
        trace = [l for l in r.stderr.splitlines() if l.startswith("[kgwas] count:")][0]
        passes = max(1, int(trace.split("passes=")[1].split()[0]))
        kern, copy_ns = sum_traces(a.profile)
        group = {"encode": 0, "sort": 0, "heads_reduce_compact": 0, "other": 0}
        for name, ns in kern.items():
            g = ("encode" if "ck_encode" in name else "heads_reduce_compact" if "ck_heads" in name or "ck_reduce" in name or "ck_compact" in name
                 else "sort" if "sort" in name.lower() or "onesweep" in name.lower() or "histogram" in name.lower() else "other")
            group[g] += ns
        w, kept_b = shape["windows"], os.path.getsize(out)
        enc_bytes = passes * shape["bases_bytes"] + 8 * w       # every pass reads the bases; every word is written once
        red_bytes = 2 * 8 * w + 4 * w + 3 * 8 * kept_b // 8     # heads twice over the words; at most: positions, results, kept words
        line = json.dumps(dict(shape, passes=passes, trace=trace,
                               kernel_ms_by_name={k: round(v / 1e6, 3) for k, v in sorted(kern.items(), key=lambda kv: -kv[1])},
                               kernel_ms_by_group={k: round(v / 1e6, 3) for k, v in group.items()},
                               kernel_ms_per_pass={k: round(v / 1e6 / passes, 3) for k, v in group.items()},
                               copy_ms_by_direction={k: round(v / 1e6, 3) for k, v in copy_ns.items()},
                               encode_hbm_floor_ms=round(enc_bytes / HBM * 1e3, 3), reduce_hbm_floor_ms=round(red_bytes / HBM * 1e3, 3),
                               encode_fraction_of_hbm=round(enc_bytes / HBM / max(group["encode"] / 1e9, 1e-12), 3),
                               reduce_fraction_of_hbm=round(red_bytes / HBM / max(group["heads_reduce_compact"] / 1e9, 1e-12), 3)))
        print(line, flush=True)
        if not a.no_append:
            with open(os.path.join(ROOT, "profiles", "count_kmers_profile.jsonl"), "a") as f:
                f.write(line + "\n")
    if os.path.exists(out):
        os.remove(out)
    if not (a.dir or a.keep):
        shutil.rmtree(d)


if __name__ == "__main__":
    main()
