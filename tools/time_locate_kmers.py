"""Kernel, copy and parse time of locate_kmers on a synthetic reference: the tool itself, timed by the events and
clocks it writes into its log (kernels and copies by HIP events, parsing by the reader thread's clock without its waits).

The reference is random bases in contigs of 60 Mb with lines of 60 letters, written once per size under --dir; the queries are
windows of it, a third as they stand, a third with one base changed, a third reverse-complemented, as a plain list. Each
configuration (reference size, queries, mismatches) runs the tool 1 + --repeat times as a process of its own; the first run warms
the page cache. Appends one JSON line per configuration to --out and prints it: the medians, the bases per second of the kernels
alone and of the whole pass, and which of parsing, copies and kernels is the largest.

  python tools/time_locate_kmers.py [--mb 120,3000] [--queries 1000,100000] [--mismatches 0,1] [--repeat 3] [--dir /tmp]
"""
import argparse
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "kmersgwas_amd", "bin", "locate_kmers")
K = 31
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def write_reference(path, mb, rng):
    """mb * 10^6 bases in contigs of 60 Mb, 60 letters a line; returns a sample of its windows"""
    sample = []
    with open(path, "wb") as f:
        left, no = mb * 1000000, 0
        while left > 0:
            n = min(left, 60000000)
            no += 1
            f.write(b">contig%d synthetic\n" % no)
            for at in range(0, n, 6000000):
                m = min(6000000, n - at) // 60 * 60  # whole lines
                if not m:
                    continue
                s = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, m, dtype=np.uint8)]
                for p in rng.integers(0, m - K, 20000):
                    sample.append(s[p:p + K].tobytes())
                lines = np.full((m // 60, 61), ord("\n"), np.uint8)
                lines[:, :60] = s.reshape(-1, 60)
                f.write(lines.tobytes())
            left -= n
    return sample


def write_queries(path, sample, n, rng):
    seen, out = set(), []
    for i, w in enumerate(sample):
        if len(out) == n:
            break
        if i % 3 == 1:
            j = int(rng.integers(0, K))
            w = w[:j] + bytes([b"ACGT"[(b"ACGT".index(w[j]) + 1 + int(rng.integers(0, 3))) % 4]]) + w[j + 1:]
        elif i % 3 == 2:
            w = w.translate(COMP)[::-1]
        c = min(w, w.translate(COMP)[::-1])
        if c not in seen:
            seen.add(c)
            out.append(w)
    if len(out) < n:
        raise SystemExit("the sample holds only %d distinct k-mers" % len(out))
    with open(path, "wb") as f:
        f.write(b"".join(w + b"\n" for w in out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", default="120,3000", help="reference sizes, 10^6 bases")
    ap.add_argument("--queries", default="1000,100000")
    ap.add_argument("--mismatches", default="0,1")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--dir", default="/tmp")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "locate_kmers_time.jsonl"))
    a = ap.parse_args()
    rng = np.random.default_rng(15)
    for mb in [int(x) for x in a.mb.split(",")]:
        ref = os.path.join(a.dir, "locate_ref_%d.fa" % mb)
        sample = write_reference(ref, mb, rng)
        for nq in [int(x) for x in a.queries.split(",")]:
            kmers = os.path.join(a.dir, "locate_kmers_%d_%d.txt" % (mb, nq))
            write_queries(kmers, sample, nq, rng)
            for d in [int(x) for x in a.mismatches.split(",")]:
                out = os.path.join(a.dir, "locate_out_%d_%d_%d.txt" % (mb, nq, d))
                runs = []
                for _ in range(1 + a.repeat):
                    r = subprocess.run([BIN, "--reference", ref, "--kmers", kmers, "--kmers_len", str(K), "--mismatches", str(d), "-o", out],
                                       capture_output=True, text=True, timeout=1100)
                    if r.returncode != 0:
                        print(r.stderr[-3000:], file=sys.stderr)
                        sys.exit(1)
                    log = open(out + ".log.txt").read()
                    ms = re.search(r"ms: parse=([0-9.]+) copy=([0-9.]+) kernels=([0-9.]+) total=([0-9.]+)", log)
                    runs.append([float(x) for x in ms.groups()])
                med = np.median(np.asarray(runs[1:]), axis=0)
                parts = dict(zip(("parse", "copy", "kernels"), med[:3]))
                found = int(re.search(r"hits_found\t(\d+)", log).group(1))
                bases = int(re.search(r"bases\t(\d+)", log).group(1))
                line = json.dumps({"bases": bases, "queries": nq, "mismatches": d, "parse_ms": round(float(med[0]), 1), "copy_ms": round(float(med[1]), 1),
                                   "kernel_ms": round(float(med[2]), 1), "total_ms": round(float(med[3]), 1),
                                   "kernel_gbases_per_s": round(bases / (med[2] * 1e-3) / 1e9, 2), "pass_gbases_per_s": round(bases / (med[3] * 1e-3) / 1e9, 3),
                                   "largest": max(parts, key=parts.get), "hits_found": found})
                print(line, flush=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")
                for p in (out, out + ".log.txt"):
                    os.remove(p)
            os.remove(kmers)
        os.remove(ref)


if __name__ == "__main__":
    main()
