#!/usr/bin/env python3
"""Synthetic benchmark of lmm_lrt at the size of one kmers_gwas.py run: 101 .bed files (1 phenotype + 100 permutations) x 10 001
k-mers x 1135 individuals against one kinship matrix. Self-contained: seeded data, no files.

Prints one JSON line: the host eigendecomposition and the rotation / grid / refinement kernels' milliseconds (summed over the
101 files), the wall time, and the rotation's fp64 rate (2 n^2 flop per variant) as a fraction of the MI355X's FP64 matrix peak.
The microarchitecture notes this project works from list no FP64 matrix figure; AMD's published 78.6 TFLOP/s is used.
There is no GEMMA timing to set beside these numbers: GEMMA is not installed where this was measured.

--columns [P] (default 101) is the SNP branch's shape instead (kmers_gwas.py:193-223): ONE synthetic .bed of 200 000 variants x 1135
individuals and P phenotype columns (one phenotype and its permutations). It times one test_bed_multi call against P test calls
on the same handle: a warm-up of each, then --reps timed repetitions (median, minimum and maximum are printed), checks that the two
give the same bits, and prints the rotation / grid / refinement split of each. grid_ms of the multi pass holds both the shared
sums and lmm_grid_xy_kernel; its rate counts the useful flop of both (2 n 202 per sum: 2 shared ones per variant, one per
variant and column).

--table [ROWS] (default 4 000 000) times lmm_lrt --kmers_table: a synthetic k-mers table of ROWS rows x 1135 accessions (the seeded
generator of the other benchmarks, written to a temporary directory), one phenotype, --mac 5 -maf 0.05 --best 10001. A warm-up and
--reps timed runs of the tool (median, minimum, maximum of the wall time; the kernels' split and the counts come from its log),
and beside them, on the same files, the wall time of the route that needs the PLINK files: kmers_table_to_bed, then lmm_lrt
-bfile (files in the page cache, the output of the first removed before every run). Both routes eigendecompose K once per run;
eigen_ms is printed so that it can be taken off.

--table [ROWS] --distinct F and / or --pattern_cache MIB time the pattern cache of lmm_lrt --kmers_table on that table (the PLINK
route is left out). With --distinct F the presence words of the rows are drawn from max(1, round(F x ROWS)) distinct synthetic
patterns: every pattern is there at least once, the other rows take one at random, and all are placed at random (the k-mer words
stay ascending); F = 1.0 gives a table without a repeated pattern. A warm-up and --reps timed runs of the tool without
--pattern_cache - the path without the cache - and, with --pattern_cache MIB, as many with it: median, minimum and maximum of the
wall time and of the kernels' split, the cache's counters from the log, the ratio of the medians, and whether the two outputs have
the same bytes.

--table [ROWS] --pheno_columns [P] (default 101) times the phenotype and its P - 1 permutations over the same synthetic table,
--mac 5 -maf 0.05 --best 10001, a warm-up and --reps timed runs of each (median, minimum, maximum of the wall time):
(a) ONE lmm_lrt --kmers_table --pheno_columns run of the P columns; (b) the way without it, one --kmers_table -n i run per column,
measured on --subset columns (default 3: the first, the middle and the last one) and scaled to P, the subset is printed; (c) run (a)
with KGWAS_LMM_TABLE_SELECT=0, the device's selection switched off. It prints the ratios (b)/(a) and (c)/(a), the kernels' split
of (a) and (c), and the share of (column, row) pairs the selection handed to the host (from the library, on the same files). The
outputs of (a) and of the measured columns of (b) are compared byte for byte.

--table [ROWS] --pheno_columns [P] --pattern_skip MIB [--distinct F] [--best N] times the dead-pattern skip of the multi-phenotype
pass on the table of --distinct (above): a warm-up and --reps timed runs of lmm_lrt --kmers_table --pheno_columns with
--pattern_skip MIB, and as many without it on the same build - the path without the option. It compares every column's output
byte for byte (cmp) and prints median, minimum and maximum of the wall time and of the kernels' split, the ratios of the medians
(kernel time and wall, without over with) and the skip's counters from the log.
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

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kmersgwas_amd as kg  # noqa: E402

FP64_MATRIX_PEAK_TFLOPS = 78.6


BINDIR = os.path.join(os.path.dirname(os.path.abspath(kg.__file__)), "bin")
SEED = 20240601


def synth_model(n, rng):
    """K, y: the kinship matrix of 2 n synthetic markers and a phenotype with a polygenic part and one strong marker"""
    rows = 2 * n
    G = (rng.random((rows, n)) < rng.uniform(0.1, 0.9, rows)[:, None]).astype(np.float64)
    K = 1.0 - (G.T @ (1 - G) + (1 - G).T @ G) / rows
    d, U = np.linalg.eigh(K)
    y = rng.standard_normal(n) + 1.5 * ((U * np.sqrt(np.clip(d, 0, None))) @ rng.standard_normal(n)) + 1.2 * G[7]
    return K, y


def write_inputs(tmp, n, rows, K, Y, rng, fraction=None):
    """The files of a --table mode in tmp: the synthetic k-mers table t.table of `rows` rows with t.names, the phenotype file (one
    column v for a vector Y, columns P0 .. for a matrix, then with the column list cols.txt) and the kinship file. With `fraction`
    the rows' presence words are drawn from max(1, round(fraction x rows)) distinct patterns, the presence words of the first
    synthetic rows: every pattern is there at least once, the other rows take one at random, all placed at random. Returns the
    paths and the number of distinct patterns."""
    base = os.path.join(tmp, "t")
    distinct = rows if fraction is None else max(1, min(rows, int(round(fraction * rows))))
    pool = which = None
    if fraction is not None:
        pool = np.concatenate([kg.synth_rows_host(r0, min(1_000_000, distinct - r0), n, SEED)[:, 1:] for r0 in range(0, distinct, 1_000_000)])
        which = rng.permutation(np.concatenate([np.arange(distinct), rng.integers(0, distinct, rows - distinct)]))
    with open(base + ".table", "wb") as f:
        f.write(np.uint32(0xDDCCBBAA).tobytes() + np.uint64(n).tobytes() + np.uint32(31).tobytes())
        for r0 in range(0, rows, 1_000_000):
            part = kg.synth_rows_host(r0, min(1_000_000, rows - r0), n, SEED)
            if pool is not None:
                part[:, 1:] = pool[which[r0:r0 + len(part)]]
            part.tofile(f)
    del pool, which
    names = ["s%d" % i for i in range(n)]
    open(base + ".names", "w").write("".join(x + "\n" for x in names))
    ph, kin, lst = os.path.join(tmp, "ph.tsv"), os.path.join(tmp, "ph.kinship"), None
    if Y.ndim == 1:
        open(ph, "w").write("accession_id\tv\n" + "".join("%s\t%.6f\n" % (x, v) for x, v in zip(names, Y)))
    else:
        P = len(Y)
        open(ph, "w").write("accession_id\t" + "\t".join("P%d" % k for k in range(P)) + "\n"
                            + "".join(names[i] + "".join("\t%.6f" % Y[k, i] for k in range(P)) + "\n" for i in range(n)))
        lst = os.path.join(tmp, "cols.txt")
        open(lst, "w").write("".join("%d\tP%d\n" % (k + 1, k) for k in range(P)))
    open(kin, "w").write("\n".join("\t".join("%.17g" % v for v in r) for r in K) + "\n")
    return {"base": base, "ph": ph, "kin": kin, "lst": lst, "distinct": distinct}


def table_cmd(inp, best, chunk_variants):
    """lmm_lrt --kmers_table on the files of write_inputs; the mode adds the outputs and its options"""
    return [os.path.join(BINDIR, "lmm_lrt"), "--kmers_table", inp["base"], "--kmers_len", "31", "-p", inp["ph"], "-lmm", "2", "-k", inp["kin"],
            "--mac", "5", "-maf", "0.05", "--best", str(best), "--chunk_variants", str(chunk_variants)]


def run_tool(cmd, env=None):
    """the wall time of one run of a tool"""
    t = time.perf_counter()
    r = subprocess.run(cmd, capture_output=True, text=True, env=env)
    if r.returncode != 0:
        sys.exit("%s failed: %s" % (os.path.basename(cmd[0]), r.stderr[-2000:]))
    return time.perf_counter() - t


def read_log(outdir, name):
    """a .log.txt as a dict: its key<TAB>value lines, and the kernels' split of its "ms: " line as floats"""
    log = {}
    for l in open(os.path.join(outdir, name + ".log.txt")).read().split("\n"):
        if "\t" in l:
            k, v = l.split("\t", 1)
            log[k] = v
        elif l.startswith("ms: "):
            log.update((kv.split("=")[0], float(kv.split("=")[1])) for kv in l[4:].split())
    return log


def timed_runs(name, fn, reps, keys):
    """A warm-up of fn and `reps` timed runs; fn returns a dict. Returns the runs and, per key, the record NAME_KEY (a key that names
    no unit is a log's milliseconds): median, minimum, maximum."""
    fn()
    runs = [fn() for _ in range(reps)]
    rec = {}
    for k in keys:
        v = sorted(float(r[k]) for r in runs)
        rec["%s_%s" % (name, k if k.endswith(("_s", "_ms")) else k + "_ms")] = {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3),
                                                                              "max": round(v[-1], 3)}
    return runs, rec


LOG_KEYS = ("wall_s", "eigen", "rotate", "grid", "refine")


def kernel_ms(line, name):
    return sum(line["%s_%s_ms" % (name, k)]["median"] for k in ("rotate", "grid", "refine"))


def bench_columns(a):
    n, m, P = a.individuals, a.variants if a.variants != 10001 else 200000, a.columns
    rng = np.random.default_rng(SEED)
    K, y = synth_model(n, rng)
    Y = np.stack([y] + [rng.permutation(y) for _ in range(P - 1)])
    bps = (n + 3) // 4
    bed = np.zeros((m, bps), np.uint8)
    for v0 in range(0, m, 20000):  # presence: code 00, absence: code 11
        v1 = min(m, v0 + 20000)
        bits = rng.random((v1 - v0, bps * 4)) < rng.uniform(0.06, 0.94, v1 - v0)[:, None]
        c = np.where(bits, 0, 3).astype(np.uint8).reshape(v1 - v0, bps, 4)
        bed[v0:v1] = c[:, :, 0] | (c[:, :, 1] << 2) | (c[:, :, 2] << 4) | (c[:, :, 3] << 6)
    lmm = kg.LmmLrt(K, chunk_variants=a.chunk_variants)
    out = {}

    def timed(name, fn):
        def run():
            before = lmm.stats()
            t = time.perf_counter()
            out[name] = fn()
            wall = time.perf_counter() - t
            after = lmm.stats()
            return dict(wall_s=wall, **{k: after[k] - before[k] for k in ("rotate_ms", "grid_ms", "refine_ms")})
        return timed_runs(name, run, a.reps, ("wall_s", "rotate_ms", "grid_ms", "refine_ms"))[1]

    recs = [timed("multi", lambda: lmm.test_bed_multi(Y, bed, maf=0.05, miss=0.5)),
            timed("single", lambda: [lmm.test(bed, Y[k], maf=0.05, miss=0.5) for k in range(P)])]
    lmm.close()
    mo, so = out["multi"], out["single"]
    same = all(mo[k][j].tobytes() == so[j][k].tobytes() for k in ("lrt", "lambda", "p") for j in range(P))
    same = same and all(mo[k].tobytes() == so[0][k].tobytes() for k in ("af", "n_miss", "tested"))
    line = {"columns": P, "variants": m, "individuals": n, "variants_tested": int(mo["tested"].sum()), "reps": a.reps, "same_bits": bool(same)}
    for rec in recs:
        line.update(rec)
    med = lambda name, k: line["%s_%s" % (name, k)]["median"]  # noqa: E731
    line["wall_ratio"] = round(med("single", "wall_s") / med("multi", "wall_s"), 3)
    line["kernel_ms_ratio"] = round(kernel_ms(line, "single") / kernel_ms(line, "multi"), 3)
    tf = 2.0 * n * 202 * m * (P + 2) / (med("multi", "grid_ms") * 1e-3) / 1e12
    line["multi_grid_tflops"] = round(tf, 3)
    line["multi_grid_fraction_of_fp64_matrix_peak"] = round(tf / FP64_MATRIX_PEAK_TFLOPS, 4)
    tf = 2.0 * n * 202 * m * 3 * P / (med("single", "grid_ms") * 1e-3) / 1e12
    line["single_grid_tflops"] = round(tf, 3)
    print(json.dumps(line))
    return 0 if same else 1


def bench_table(a):
    n, rows = a.individuals, a.table
    rng = np.random.default_rng(SEED)
    K, y = synth_model(n, rng)
    tmp = tempfile.mkdtemp(prefix="bench_lmm_table_")
    try:
        inp = write_inputs(tmp, n, rows, K, y, rng)
        out = os.path.join(tmp, "out")

        def table_route():
            wall = run_tool(table_cmd(inp, 10001, a.chunk_variants) + ["-outdir", out, "-o", "table"])
            return dict(wall_s=wall, **read_log(out, "table"))

        def bed_route():
            for f in os.listdir(tmp):
                if f.startswith("plink."):
                    os.remove(os.path.join(tmp, f))
            t1 = run_tool([os.path.join(BINDIR, "kmers_table_to_bed"), "-t", inp["base"], "-k", "31", "-p", inp["ph"], "--maf", "0.05",
                           "--mac", "5", "-b", str(rows + 1), "-o", os.path.join(tmp, "plink")])
            t2 = run_tool([os.path.join(BINDIR, "lmm_lrt"), "-bfile", os.path.join(tmp, "plink.0"), "-lmm", "2", "-k", inp["kin"], "-maf", "0.05",
                           "-outdir", out, "-o", "bed", "--chunk_variants", str(a.chunk_variants)])
            return dict(wall_s=t1 + t2, table_to_bed_s=t1, lmm_lrt_s=t2, **read_log(out, "bed"))

        line = {"table_rows": rows, "individuals": n, "best": 10001, "reps": a.reps}
        runs, rec = timed_runs("table", table_route, a.reps, LOG_KEYS)
        line.update(rec)
        line["rows_tested"], line["rows_kept"] = int(runs[0]["rows_tested"]), int(runs[0]["rows_kept"])
        runs, rec = timed_runs("bed", bed_route, a.reps, LOG_KEYS + ("table_to_bed_s", "lmm_lrt_s"))
        line.update(rec)
        line["bed_variants_tested"] = int(runs[0]["variants_tested"])
        wall = line["table_wall_s"]["median"]
        line["rows_per_s"] = round(rows / wall)
        line["tested_rows_per_s"] = round(line["rows_tested"] / wall)
        line["kernel_ms_per_million_tested"] = round(kernel_ms(line, "table") / max(line["rows_tested"], 1) * 1e6, 3)
        line["wall_ratio_bed_over_table"] = round(line["bed_wall_s"]["median"] / wall, 3)
        print(json.dumps(line))
        return 0 if line["rows_tested"] == line["bed_variants_tested"] else 1
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def bench_table_cache(a):
    n, rows = a.individuals, a.table
    rng = np.random.default_rng(SEED)
    K, y = synth_model(n, rng)
    tmp = tempfile.mkdtemp(prefix="bench_lmm_cache_")
    try:
        inp = write_inputs(tmp, n, rows, K, y, rng, a.distinct)
        out = os.path.join(tmp, "out")

        def route(name, extra):
            wall = run_tool(table_cmd(inp, 10001, a.chunk_variants) + ["-outdir", out, "-o", name] + extra)
            return dict(wall_s=wall, **read_log(out, name))

        line = {"table_rows": rows, "individuals": n, "distinct_patterns": inp["distinct"], "best": 10001, "reps": a.reps}
        runs, rec = timed_runs("table", lambda: route("table", []), a.reps, LOG_KEYS)
        line.update(rec)
        line["rows_tested"], line["rows_kept"] = int(runs[0]["rows_tested"]), int(runs[0]["rows_kept"])
        same = True
        if a.pattern_cache:
            runs, rec = timed_runs("cache", lambda: route("cache", ["--pattern_cache", str(a.pattern_cache)]), a.reps, LOG_KEYS)
            line.update(rec)
            line["pattern_cache_mib"] = a.pattern_cache
            for k in ("pattern_cache_slots", "patterns_cached", "rows_from_cache", "rows_collided", "rows_rejected", "rows_rotated"):
                line[k] = int(runs[0][k])
            same = open(os.path.join(out, "table.assoc.txt"), "rb").read() == open(os.path.join(out, "cache.assoc.txt"), "rb").read()
            line["same_bytes"] = bool(same)
            line["wall_ratio_table_over_cache"] = round(line["table_wall_s"]["median"] / line["cache_wall_s"]["median"], 3)
            line["kernel_ms_ratio_table_over_cache"] = round(kernel_ms(line, "table") / max(kernel_ms(line, "cache"), 1e-9), 3)
        print(json.dumps(line))
        return 0 if same else 1
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def bench_table_multi(a):
    n, rows, P = a.individuals, a.table, a.pheno_columns
    rng = np.random.default_rng(SEED)
    K, y = synth_model(n, rng)
    Y = np.stack([y] + [rng.permutation(y) for _ in range(P - 1)])
    tmp = tempfile.mkdtemp(prefix="bench_lmm_table_multi_")
    try:
        inp = write_inputs(tmp, n, rows, K, Y, rng)
        common = table_cmd(inp, 10001, a.chunk_variants)
        subset = sorted(set(np.linspace(0, P - 1, max(1, min(a.subset, P))).astype(int).tolist()))
        out_a, out_b, out_c = (os.path.join(tmp, d) for d in ("multi", "single", "noselect"))
        off = dict(os.environ, KGWAS_LMM_TABLE_SELECT="0")

        def run_a():
            return dict(wall_s=run_tool(common + ["-outdir", out_a, "--pheno_columns", inp["lst"]]), **read_log(out_a, "P0"))

        def run_c():
            return dict(wall_s=run_tool(common + ["-outdir", out_c, "--pheno_columns", inp["lst"]], env=off), **read_log(out_c, "P0"))

        def run_b():
            walls = [run_tool(common + ["-outdir", out_b, "-n", str(k + 1), "-o", "P%d" % k]) for k in subset]
            return dict(wall_s=sum(walls) * P / len(subset), measured_s=sum(walls), **read_log(out_b, "P%d" % subset[0]))

        line = {"table_rows": rows, "individuals": n, "columns": P, "best": 10001, "reps": a.reps, "single_subset": [k + 1 for k in subset]}
        for name, fn in (("multi", run_a), ("single_scaled", run_b), ("multi_noselect", run_c)):
            runs, rec = timed_runs(name, fn, a.reps, LOG_KEYS)
            line.update(rec)
            if name == "multi":
                line["rows_tested"] = int(runs[0]["rows_tested"])
        same = all(open(os.path.join(d, "P%d.assoc.txt" % k), "rb").read() == open(os.path.join(out_a, "P%d.assoc.txt" % k), "rb").read()
                   for d, ks in ((out_b, subset), (out_c, range(P))) for k in ks)
        line["same_bytes"] = bool(same)
        med = lambda name: line[name + "_wall_s"]["median"]  # noqa: E731
        line["wall_ratio_single_over_multi"] = round(med("single_scaled") / med("multi"), 3)
        line["wall_ratio_noselect_over_multi"] = round(med("multi_noselect") / med("multi"), 3)
        # the selection's share, from the library on the same files (one more pass, not timed)
        tbl = kg.KmersTable(inp["base"], 31)
        lmm = kg.LmmLrt(K, chunk_variants=a.chunk_variants)
        # the values the tool tests: the file's "%.6f" text as the loader's float32, printed with six significant digits, parsed again
        Yt = np.array([[float("%g" % np.float32(float("%.6f" % v))) for v in row] for row in Y])
        res = lmm.test_table_multi(tbl, np.arange(n, dtype=np.uint64), Yt, kg.min_count(n, 0.05, 5), 0.05, 10001)
        lmm.close()
        tbl.close()
        line["pairs_shipped"], line["pairs"] = int(res["pairs_shipped"]), int(res["rows_tested"]) * P
        line["pairs_shipped_share"] = round(res["pairs_shipped"] / max(res["rows_tested"] * P, 1), 6)
        print(json.dumps(line))
        return 0 if same else 1
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def bench_table_multi_skip(a):
    n, rows, P, best = a.individuals, a.table, a.pheno_columns, a.best
    rng = np.random.default_rng(SEED)
    K, y = synth_model(n, rng)
    Y = np.stack([y] + [rng.permutation(y) for _ in range(P - 1)])
    tmp = tempfile.mkdtemp(prefix="bench_lmm_skip_")
    try:
        inp = write_inputs(tmp, n, rows, K, Y, rng, a.distinct)
        common = table_cmd(inp, best, a.chunk_variants) + ["--pheno_columns", inp["lst"]]

        def route(name, extra):
            outdir = os.path.join(tmp, name)
            wall = run_tool(common + ["-outdir", outdir] + extra)
            print("%s: %.1f s" % (name, wall), file=sys.stderr, flush=True)
            return dict(wall_s=wall, **read_log(outdir, "P0"))

        line = {"table_rows": rows, "individuals": n, "columns": P, "distinct_patterns": inp["distinct"], "best": best, "reps": a.reps,
                "pattern_skip_mib": a.pattern_skip}
        runs, rec = timed_runs("skip", lambda: route("skip", ["--pattern_skip", str(a.pattern_skip)]), a.reps, LOG_KEYS)
        line.update(rec)
        line["rows_tested"] = int(runs[0]["rows_tested"])
        for k in ("pattern_skip_slots", "patterns_cached", "patterns_dead", "rows_skipped", "rows_collided", "rows_rejected", "rows_rotated"):
            line[k] = int(runs[0][k])
        line.update(timed_runs("plain", lambda: route("plain", []), a.reps, LOG_KEYS)[1])
        same = all(subprocess.run(["cmp", "-s", os.path.join(tmp, "skip", "P%d.assoc.txt" % k), os.path.join(tmp, "plain", "P%d.assoc.txt" % k)]).returncode == 0
                   for k in range(P))
        line["same_bytes"] = bool(same)
        line["kernel_ms_ratio_plain_over_skip"] = round(kernel_ms(line, "plain") / max(kernel_ms(line, "skip"), 1e-9), 3)
        line["wall_ratio_plain_over_skip"] = round(line["plain_wall_s"]["median"] / line["skip_wall_s"]["median"], 3)
        print(json.dumps(line))
        return 0 if same else 1
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--beds", type=int, default=101)
    ap.add_argument("--variants", type=int, default=10001)
    ap.add_argument("--individuals", type=int, default=1135)
    ap.add_argument("--chunk_variants", type=int, default=10240)
    ap.add_argument("--columns", type=int, nargs="?", const=101, default=None,
                    help="time one test_bed_multi call of P columns (default 101) over one .bed of 200 000 variants against P test calls")
    ap.add_argument("--reps", type=int, default=3, help="timed repetitions of the --columns and --table modes")
    ap.add_argument("--table", type=int, nargs="?", const=4_000_000, default=None,
                    help="time lmm_lrt --kmers_table over a synthetic table of ROWS rows (default 4 000 000) against kmers_table_to_bed + lmm_lrt -bfile")
    ap.add_argument("--pheno_columns", type=int, nargs="?", const=101, default=None,
                    help="with --table: time one --pheno_columns run of P columns (default 101) against P runs of --kmers_table -n i "
                         "(measured on --subset columns and scaled) and against the same run without the device's selection")
    ap.add_argument("--distinct", type=float, default=None,
                    help="with --table: the rows' patterns are drawn from F x ROWS distinct ones, placed at random (0 < F <= 1)")
    ap.add_argument("--pattern_cache", type=int, default=None,
                    help="with --table: time lmm_lrt --kmers_table with --pattern_cache MIB against the run without it")
    ap.add_argument("--pattern_skip", type=int, default=None,
                    help="with --table --pheno_columns: time the run with --pattern_skip MIB against the run without it (--distinct and --best apply)")
    ap.add_argument("--best", type=int, default=10001, help="--best of the --pattern_skip mode's runs (default 10001)")
    ap.add_argument("--subset", type=int, default=3, help="columns of the --pheno_columns mode's one-run-per-column route that are measured")
    a = ap.parse_args()
    if a.pattern_skip is not None:
        if a.table is None or a.pheno_columns is None or a.pattern_cache is not None:
            sys.exit("--pattern_skip needs --table and --pheno_columns, without --pattern_cache")
        if a.distinct is not None and not 0 < a.distinct <= 1:
            sys.exit("--distinct takes a fraction within (0, 1]")
        sys.exit(bench_table_multi_skip(a))
    if a.distinct is not None or a.pattern_cache is not None:
        if a.table is None or a.pheno_columns is not None:
            sys.exit("--distinct and --pattern_cache need --table, without --pheno_columns")
        if a.distinct is not None and not 0 < a.distinct <= 1:
            sys.exit("--distinct takes a fraction within (0, 1]")
        sys.exit(bench_table_cache(a))
    if a.pheno_columns is not None:
        if a.table is None:
            sys.exit("--pheno_columns needs --table")
        sys.exit(bench_table_multi(a))
    if a.table is not None:
        sys.exit(bench_table(a))
    if a.columns is not None:
        sys.exit(bench_columns(a))
    n, m = a.individuals, a.variants
    rng = np.random.default_rng(20240601)
    K, y = synth_model(n, rng)
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
