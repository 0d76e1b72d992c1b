"""Wall time of bin/build_kmers_table on sorted k-mer files in the page cache.

Writes an all-k-mers file of --rows ascending keys spread over the 62-bit key space of k = 31 (so that the reference's 5001 key
windows are even) and --acc accession files, each holding a random --density of those keys; reads them once so that they are in the
page cache; then times the tool --repeat times and appends one JSON line per run to profiles/build_kmers_table_time.jsonl
(--no-append: prints only). Inputs already in --dir, of this shape, are used as they are; --keep leaves them there.

  python tools/time_build_kmers_table.py --rows 4000000 --acc 1135 [--density 0.25] [--dir /tmp/x] [--keep]
"""
import argparse
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
BIN = os.path.join(ROOT, "kmersgwas_amd", "bin", "build_kmers_table")
K = 31


_ALL = {}


def write_accession(args):
    d, c, rows, density = args
    if d not in _ALL:  # (once per worker process)
        _ALL[d] = np.fromfile(os.path.join(d, "all.kmers"), "<u8")
    a = _ALL[d]
    rng = np.random.default_rng(1000 + c)
    w = a[rng.random(rows) < density]
    if len(w) == 0:
        w = a[:1]
    w.tofile(os.path.join(d, "a%d.sorted" % c))
    return len(w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--acc", type=int, default=1135)
    ap.add_argument("--density", type=float, default=0.25)
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--workers", type=int, default=12)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--keep", action="store_true")
    ap.add_argument("--no-append", action="store_true")
    a = ap.parse_args()
    d = a.dir or tempfile.mkdtemp(prefix="bt_")
    os.makedirs(d, exist_ok=True)
    need = 8 * a.rows * (1 + a.acc * a.density) + 8 * a.rows * (1 + (a.acc + 63) // 64)
    free = shutil.disk_usage(d).free
    if free < 1.1 * need:
        sys.exit("time_build_kmers_table: %s has %.1f GB free, inputs and table need about %.1f GB" % (d, free / 1e9, need / 1e9))
    shape = os.path.join(d, "shape.json")
    want = {"rows": a.rows, "acc": a.acc, "density": a.density}
    if not (os.path.exists(shape) and json.load(open(shape)) == want):
        rng = np.random.default_rng(1)
        keys = np.unique(rng.integers(0, 1 << 62, size=a.rows, dtype=np.uint64))
        while len(keys) < a.rows:
            keys = np.unique(np.concatenate([keys, rng.integers(0, 1 << 62, size=a.rows - len(keys), dtype=np.uint64)]))
        keys.tofile(os.path.join(d, "all.kmers"))
        del keys
        with ProcessPoolExecutor(a.workers) as ex:
            list(ex.map(write_accession, [(d, c, a.rows, a.density) for c in range(a.acc)], chunksize=8))
        with open(os.path.join(d, "list.txt"), "w") as f:
            for c in range(a.acc):
                f.write("%s\tacc%d\n" % (os.path.join(d, "a%d.sorted" % c), c))
        json.dump(want, open(shape, "w"))
    paths = [os.path.join(d, "all.kmers")] + [os.path.join(d, "a%d.sorted" % c) for c in range(a.acc)]
    in_bytes = 0
    for p in paths:  # into the page cache
        with open(p, "rb") as f:
            while True:
                b = f.read(64 << 20)
                if not b:
                    break
                in_bytes += len(b)
    out = os.path.join(d, "out")
    for rep in range(a.repeat):
        t0 = time.perf_counter()
        r = subprocess.run([BIN, "-l", os.path.join(d, "list.txt"), "-k", str(K), "-a", paths[0], "-o", out], capture_output=True,
                           text=True, timeout=3000)
        wall = time.perf_counter() - t0
        if r.returncode != 0:
            print(r.stderr[-3000:], file=sys.stderr)
            sys.exit(1)
        line = json.dumps({"rows": a.rows, "acc": a.acc, "density": a.density, "rep": rep, "wall_s": round(wall, 3),
                           "input_GBps": round(in_bytes / wall / 1e9, 2), "input_bytes": in_bytes,
                           "table_bytes": os.path.getsize(out + ".table"), "tool_seconds": r.stderr.strip().splitlines()[-1]})
        print(line, flush=True)
        if not a.no_append:
            with open(os.path.join(ROOT, "profiles", "build_kmers_table_time.jsonl"), "a") as f:
                f.write(line + "\n")
        os.remove(out + ".table")
    if not (a.dir or a.keep):
        shutil.rmtree(d)


if __name__ == "__main__":
    main()
