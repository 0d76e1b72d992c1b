"""Wall time of bin/filter_kmers on a file-backed table in the page cache.

Writes a synthetic table (keys = row + 1, ascending; kgwas_synth_rows_host bits) of --rows x --acc, reads it once so that it
is in the page cache, then times the tool for each list size: `present` of the list are table keys, the rest absent. With
--descend the first two rows are swapped, so the host's merge-join runs over the whole table. Prints one JSON line per run.

  python tools/time_filter_kmers.py --rows 10000000 --acc 1135 --lists 1000,10000000 [--descend] [--dir /tmp/x]
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import kmersgwas_amd as kg  # noqa: E402

K = 31


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--acc", type=int, default=1135)
    ap.add_argument("--lists", default="1000,10000000")
    ap.add_argument("--present", type=float, default=0.01, help="fraction of each list that are table keys")
    ap.add_argument("--descend", action="store_true")
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--dir", default=None)
    a = ap.parse_args()
    d = a.dir or tempfile.mkdtemp(prefix="fk_")
    os.makedirs(d, exist_ok=True)
    base = os.path.join(d, "tab")
    W = (a.acc + 63) // 64
    with open(base + ".names", "w") as f:
        f.write("".join("acc%d\n" % i for i in range(a.acc)))
    want = 16 + 8 * (1 + W) * a.rows
    fresh = not (a.dir and os.path.exists(base + ".table") and os.path.getsize(base + ".table") == want and not a.descend)
    if fresh:  # (a table already in --dir, of this shape and ascending, is used as it is)
        with open(base + ".table", "wb") as f:
            f.write(np.uint32(0xDDCCBBAA).tobytes() + np.uint64(a.acc).tobytes() + np.uint32(K).tobytes())
            step = max(1, (256 << 20) // (8 * (1 + W)))
            for r0 in range(0, a.rows, step):
                rows = kg.synth_rows_host(r0, min(step, a.rows - r0), a.acc, 99)
                if a.descend and r0 == 0:
                    rows[[0, 1], 0] = rows[[1, 0], 0]
                f.write(rows.tobytes())
    table_bytes = os.path.getsize(base + ".table")
    with open(base + ".table", "rb") as f:  # into the page cache
        while f.read(64 << 20):
            pass
    rng = np.random.default_rng(1)
    for n in [int(x) for x in a.lists.split(",")]:
        n_in = int(n * a.present) if n > 1000 else n // 2
        keys = rng.integers(1, a.rows + 1, size=n_in, dtype=np.uint64)
        absent = rng.integers(a.rows + 2, 1 << 40, size=n - n_in, dtype=np.uint64)
        codes = np.concatenate([keys, absent])
        # words whose canonical code is the key itself (keys < 4^31 / 2 are their own canonical form when the rc is larger)
        lst = os.path.join(d, "list_%d.txt" % n)
        acgt = np.frombuffer(b"ACGT", np.uint8)
        buf = np.empty((n, K + 1), np.uint8)
        for j in range(K):
            buf[:, j] = acgt[((codes >> np.uint64(2 * (K - 1 - j))) & np.uint64(3)).astype(np.int64)]
        buf[:, K] = ord("\n")
        with open(lst, "wb") as f:
            f.write(buf.tobytes())
        for rep in range(a.repeat):
            out = os.path.join(d, "out.tsv")
            t0 = time.perf_counter()
            r = subprocess.run([os.path.join(ROOT, "kmersgwas_amd", "bin", "filter_kmers"), "-t", base, "-k", lst, "-o", out],
                               capture_output=True, text=True, timeout=1800)
            wall = time.perf_counter() - t0
            if r.returncode != 0:
                print(r.stderr[-3000:], file=sys.stderr)
                sys.exit(1)
            out_bytes = os.path.getsize(out)
            print(json.dumps({"rows": a.rows, "acc": a.acc, "list": n, "descend": a.descend, "rep": rep, "wall_s": round(wall, 3),
                              "table_GBps": round(table_bytes / wall / 1e9, 2), "table_bytes": table_bytes, "out_bytes": out_bytes,
                              "tool_seconds": r.stderr.strip().splitlines()[-1]}), flush=True)
            os.remove(out)
    if not a.dir:
        shutil.rmtree(d)


if __name__ == "__main__":
    main()
