"""Wall time of bin/list_kmers_found_in_multiple_samples on sorted k-mer files in the page cache, and its kernels' time next to its
copies' (DESIGN.md §4.10).

Writes --acc sorted k-mer files at k = 31 whose keys come from --keys distinct values spread over the 62-bit key space (so that the
reference's 5001 key windows are even). A key's multiplicity is drawn from a distribution with many singletons and a long tail (60 % of
the keys in one file, 20 % in 2-5, 10 % in 10-50, 7 % in 100-300, 3 % in 1000 of 1135 files: about 48 words per key), its files are
spread over the list and its strand flags are random. The files are read once so that they are in the page cache; then the tool is
timed --repeat times and one JSON line per run is appended to profiles/list_kmers_time.jsonl (--no-append: prints only). Inputs
already in --dir, of this shape, are used as they are; --keep leaves them there.

--profile DIR runs the tool once more under `rocprofv3 --kernel-trace --memory-copy-trace --stats` (no counters in that run), sums
the kernels' and the copies' durations from the traces and prints them per device piece, with the piece's host-to-device bytes and
what 55 GB/s (the feed rate this project has measured) would take for them; the traces stay in DIR.

  python tools/time_list_kmers.py --keys 1000000 --acc 1135 [--dir /tmp/x] [--keep] [--profile /tmp/list_prof]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "kmersgwas_amd", "bin", "list_kmers_found_in_multiple_samples")
K = 31
U = np.uint64
_KEYS = {}


def multiplicity(keys, n_acc):
    """Files per key, from bits of the key (a random 62-bit number)."""
    u = ((keys >> U(8)) & U(0xFFFF)).astype(np.float64) / 65536.0
    v = ((keys >> U(24)) & U(0xFFFF)).astype(np.float64) / 65536.0
    m = np.ones(len(keys), np.int64)
    for lo, hi, a, b in ((0.60, 0.80, 2, 5), (0.80, 0.90, 10, 50), (0.90, 0.97, 100, 300), (0.97, 1.01, 1000, 1000)):
        sel = (u >= lo) & (u < hi)
        m[sel] = (a + v[sel] * (b - a + 1)).astype(np.int64).clip(a, b)
    return np.minimum(m, n_acc)


def write_accession(args):
    d, c, n_acc = args
    if d not in _KEYS:  # (once per worker process)
        keys = np.fromfile(os.path.join(d, "keys.u64"), "<u8")
        _KEYS[d] = keys, multiplicity(keys, n_acc), ((keys >> U(40)) % U(n_acc)).astype(np.int64)
    keys, m, off = _KEYS[d]
    mult = next(x for x in range(389, 2 * n_acc + 389) if np.gcd(x, n_acc) == 1)  # c -> (c + off) * mult mod n_acc is a bijection
    w = keys[((c + off) * mult) % n_acc < m]
    if len(w) == 0:
        w = keys[:1]
    flags = (((w ^ U(c * 0x9E3779B1)) * U(0x2545F4914F6CDD1D)) >> U(33)) % U(3) + U(1)
    (w | (flags << U(62))).tofile(os.path.join(d, "a%d.sorted" % c))
    return len(w)


def sum_traces(prof_dir):
    """(kernel ns by name, copy ns by direction) from rocprofv3's csv traces under prof_dir."""
    kern, copy_ns = {}, {}
    for path in glob.glob(os.path.join(prof_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            name = r["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0].split("<")[0]
            kern[name] = kern.get(name, 0) + int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    for path in glob.glob(os.path.join(prof_dir, "**", "*memory_copy_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            d = r["Direction"]
            copy_ns[d] = copy_ns.get(d, 0) + int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    return kern, copy_ns


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=1_000_000)
    ap.add_argument("--acc", type=int, default=1135)
    ap.add_argument("--mac", type=int, default=5)
    ap.add_argument("--percent", type=float, default=0.2)
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--workers", type=int, default=12)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--keep", action="store_true")
    ap.add_argument("--no-append", action="store_true")
    ap.add_argument("--profile", default=None)
    a = ap.parse_args()
    d = a.dir or tempfile.mkdtemp(prefix="lk_")
    os.makedirs(d, exist_ok=True)
    need = 8 * a.keys * 50
    free = shutil.disk_usage(d).free
    if free < 1.2 * need:
        sys.exit("time_list_kmers: %s has %.1f GB free, the inputs need about %.1f GB" % (d, free / 1e9, need / 1e9))
    shape = os.path.join(d, "shape.json")
    want = {"keys": a.keys, "acc": a.acc}
    if not (os.path.exists(shape) and json.load(open(shape)) == want):
        rng = np.random.default_rng(1)
        keys = np.unique(rng.integers(0, 1 << 62, size=a.keys, dtype=U))
        keys.tofile(os.path.join(d, "keys.u64"))
        del keys
        with ProcessPoolExecutor(a.workers) as ex:
            list(ex.map(write_accession, [(d, c, a.acc) for c in range(a.acc)], chunksize=8))
        with open(os.path.join(d, "list.txt"), "w") as f:
            for c in range(a.acc):
                f.write("%s\tacc%d\n" % (os.path.join(d, "a%d.sorted" % c), c))
        json.dump(want, open(shape, "w"))
    in_bytes = 0
    for c in range(a.acc):  # into the page cache
        with open(os.path.join(d, "a%d.sorted" % c), "rb") as f:
            while True:
                b = f.read(64 << 20)
                if not b:
                    break
                in_bytes += len(b)
    out = os.path.join(d, "out")
    cmd = [BIN, "-l", os.path.join(d, "list.txt"), "-k", str(K), "--mac", str(a.mac), "-p", str(a.percent), "-o", out]
    env = dict(os.environ, KGWAS_TRACE="1")
    for rep in range(a.repeat):
        t0 = time.perf_counter()
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=3000, env=env)
        wall = time.perf_counter() - t0
        if r.returncode != 0:
            print(r.stderr[-3000:], file=sys.stderr)
            sys.exit(1)
        err = r.stderr.strip().splitlines()
        line = json.dumps({"keys": a.keys, "acc": a.acc, "words": in_bytes // 8, "rep": rep, "wall_s": round(wall, 3),
                           "input_GBps": round(in_bytes / wall / 1e9, 2), "input_bytes": in_bytes, "passed_bytes": os.path.getsize(out),
                           "pieces": err[0], "summary": err[1:4], "tool_seconds": err[-1]})
        print(line, flush=True)
        if not a.no_append:
            with open(os.path.join(ROOT, "profiles", "list_kmers_time.jsonl"), "a") as f:
                f.write(line + "\n")
    if a.profile:
        os.makedirs(a.profile, exist_ok=True)
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--memory-copy-trace", "--stats", "-f", "csv", "-d", a.profile, "--"] + cmd,
                           capture_output=True, text=True, timeout=3000, env=dict(env, KGWAS_CLI_FULL_TEARDOWN="1"))  # (the tool's
        # _exit would leave before the profiler writes its traces)
        if r.returncode != 0:
            print(r.stderr[-3000:], file=sys.stderr)
            sys.exit(1)
        trace = [l for l in r.stderr.splitlines() if l.startswith("[kgwas] list:")][0]
        pieces = int(trace.split("device_pieces=")[1].split()[0])
        kern, copy_ns = sum_traces(a.profile)
        h2d = sum(v for k, v in copy_ns.items() if "HOST_TO_DEVICE" in k.upper() or "H2D" in k.upper())
        line = json.dumps({"keys": a.keys, "acc": a.acc, "words": in_bytes // 8, "device_pieces": pieces, "trace": trace,
                           "kernel_ms_by_name": {k: round(v / 1e6, 3) for k, v in sorted(kern.items(), key=lambda kv: -kv[1])},
                           "copy_ms_by_direction": {k: round(v / 1e6, 3) for k, v in copy_ns.items()},
                           "kernels_ms_per_piece": round(sum(kern.values()) / 1e6 / max(pieces, 1), 3),
                           "h2d_ms_per_piece": round(h2d / 1e6 / max(pieces, 1), 3),
                           "h2d_ms_per_piece_at_55GBps": round(in_bytes / 55e9 * 1e3 / max(pieces, 1), 3)})
        print(line, flush=True)
        if not a.no_append:
            with open(os.path.join(ROOT, "profiles", "list_kmers_profile.jsonl"), "a") as f:
                f.write(line + "\n")
    for e in ("", ".no_pass_kmers", ".shareness", ".stats.only_canonical", ".stats.only_non_canonical", ".stats.both"):
        if os.path.exists(out + e):
            os.remove(out + e)
    if not (a.dir or a.keep):
        shutil.rmtree(d)


if __name__ == "__main__":
    main()
