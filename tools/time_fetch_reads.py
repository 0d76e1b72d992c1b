"""Parse, copy and kernel time of fetch_reads on a synthetic read set: the tool itself, timed by the events and
clocks it writes into its log (kernels and copies by HIP events, parsing by the reader thread's clock without its waits).

The reads are random 150-base FASTQ records generated from a seed, --gb * 10^9 bases of them (at least 1), written once under
--dir. The queries are a plain list: 1 000 windows of the reads, half of them reverse-complemented, and - for a larger list - random
31-mers on top, which occur in no read; so the same few reads are kept whatever the list's size, and the kernels' time shows what
the list's size and the prefilter cost. Each configuration (queries, prefilter on / off through KGWAS_FETCH_PREFILTER) runs the
tool 1 + --repeat times as a process of its own; the first run warms the page cache. Appends one JSON line per configuration to
--out and prints it: the medians, the bases per second of the kernels alone and of the whole pass, and which of parsing, copies
and kernels is the largest.

  python tools/time_fetch_reads.py [--gb 1] [--queries 1000,1048576] [--prefilter 1,0] [--repeat 3] [--dir /tmp]
"""
import argparse
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "kmersgwas_amd", "bin", "fetch_reads")
K = 31
READ = 150
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def write_reads(path, n_reads, rng):
    """n_reads FASTQ records "@r<9 digits>", 150 bases, "+", 150 quality letters; returns a sample of the reads' windows"""
    sample = []
    with open(path, "wb") as f:
        for first in range(0, n_reads, 200000):
            n = min(200000, n_reads - first)
            rec = np.empty((n, 12 + READ + 1 + 2 + READ + 1), np.uint8)
            ids = np.arange(first, first + n, dtype=np.int64)
            rec[:, 0], rec[:, 1] = ord("@"), ord("r")
            for d in range(9):
                rec[:, 10 - d] = ord("0") + (ids // 10 ** d) % 10
            seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (n, READ), dtype=np.uint8)]
            rec[:, 11], rec[:, 12:12 + READ], rec[:, 12 + READ] = 10, seq, 10
            rec[:, 13 + READ], rec[:, 14 + READ], rec[:, 15 + READ:15 + 2 * READ], rec[:, 15 + 2 * READ] = ord("+"), 10, ord("I"), 10
            f.write(rec.tobytes())
            for r, p in zip(rng.integers(0, n, 40), rng.integers(0, READ - K + 1, 40)):
                sample.append(seq[r, p:p + K].tobytes())
    return sample


def write_queries(path, sample, n, rng):
    seen, out = set(), []

    def add(w):
        c = min(w, w.translate(COMP)[::-1])
        if c not in seen:
            seen.add(c)
            out.append(w)

    for i, w in enumerate(sample):
        if len(out) == min(n, 1000):
            break
        add(w.translate(COMP)[::-1] if i % 2 else w)
    while len(out) < n:  # random 31-mers: in none of the reads
        block = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (min(n - len(out), 1 << 18), K), dtype=np.uint8)]
        for row in block:
            add(row.tobytes())
    with open(path, "wb") as f:
        f.write(b"".join(w + b"\n" for w in out[:n]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=1.0, help="10^9 bases of reads")
    ap.add_argument("--queries", default="1000,1048576")
    ap.add_argument("--prefilter", default="1,0")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--dir", default="/tmp")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fetch_reads_time.jsonl"))
    a = ap.parse_args()
    rng = np.random.default_rng(16)
    n_reads = int(a.gb * 1e9 + READ - 1) // READ
    reads = os.path.join(a.dir, "fetch_reads_%d.fq" % n_reads)
    sample = write_reads(reads, n_reads, rng)
    for nq in [int(x) for x in a.queries.split(",")]:
        kmers = os.path.join(a.dir, "fetch_kmers_%d.txt" % nq)
        write_queries(kmers, sample, nq, rng)
        for pre in [int(x) for x in a.prefilter.split(",")]:
            prefix = os.path.join(a.dir, "fetch_out_%d_%d" % (nq, pre))
            runs = []
            for _ in range(1 + a.repeat):
                r = subprocess.run([BIN, "--reads", reads, "--kmers", kmers, "--kmers_len", str(K), "-o", prefix], capture_output=True, text=True, timeout=1100,
                                   env=dict(os.environ, KGWAS_FETCH_PREFILTER=str(pre)))
                if r.returncode != 0:
                    print(r.stderr[-3000:], file=sys.stderr)
                    sys.exit(1)
                log = open(prefix + ".log.txt").read()
                ms = re.search(r"ms: parse=([0-9.]+) copy=([0-9.]+) kernels=([0-9.]+) total=([0-9.]+)", log)
                runs.append([float(x) for x in ms.groups()])
            med = np.median(np.asarray(runs[1:]), axis=0)
            parts = dict(zip(("parse", "copy", "kernels"), med[:3]))
            count = lambda key: int(re.search(r"^%s\t(\d+)$" % key, log, re.M).group(1))
            bases = count("bases")
            line = json.dumps({"reads": count("reads"), "bases": bases, "queries": nq, "prefilter": pre, "parse_ms": round(float(med[0]), 1),
                               "copy_ms": round(float(med[1]), 1), "kernel_ms": round(float(med[2]), 1), "total_ms": round(float(med[3]), 1),
                               "kernel_gbases_per_s": round(bases / (med[2] * 1e-3) / 1e9, 2), "pass_gbases_per_s": round(bases / (med[3] * 1e-3) / 1e9, 3),
                               "largest": max(parts, key=parts.get), "windows_hit": count("windows_hit"), "reads_kept": count("reads_kept")})
            print(line, flush=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
            for e in (".fastq", ".reads.tsv", ".log.txt"):
                os.remove(prefix + e)
        os.remove(kmers)
    os.remove(reads)


if __name__ == "__main__":
    main()
