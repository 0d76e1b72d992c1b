"""lmm_lrt --kmers_table without a GPU: the refusals of the tool (each a non-zero exit, its message, and no output file), the
device error of a well-formed command line on a machine without a GPU, the new entry points, and the model gap of the fixture
that test_gpu_lmm_lrt_table.py checks against model E."""
import os
import subprocess

import numpy as np
import pytest

from kmersgwas_amd import capi
from kmersgwas_amd.capi import lib
from oracle import oracle_np as onp

import lmm_lrt_np as M
import lmm_table_np as T

BIN = os.path.join(os.path.dirname(os.path.abspath(capi.__file__)), "bin", "lmm_lrt")
S, S_F = 12, 14


@pytest.fixture
def files(tmp_path):
    """A table of 14 accessions, a phenotype file of 12 of them (two columns) and their 12 x 12 kinship matrix."""
    rng = np.random.default_rng(1)
    pick = rng.permutation(S_F)[:S]
    rows = T.table_from_bits(T.random_bits(60, S, 1, 0.2, 0.8), S_F, pick, 1)
    names = ["acc%d" % i for i in range(S_F)]
    base = str(tmp_path / "tab")
    onp.write_table(base, names, T.K_LEN, rows[:, 0], rows[:, 1:])
    ph = tmp_path / "ph.tsv"
    ph.write_text("accession_id\ta\tb\n" + "".join("%s\t%.4f\t%.4f\n" % (names[c], rng.normal(60, 9), rng.normal()) for c in pick))
    G = (rng.random((200, S)) < 0.4).astype(np.float64)
    K = 1.0 - (G.T @ (1 - G) + (1 - G).T @ G) / 200
    kin = tmp_path / "ph.kinship"
    kin.write_text("\n".join("\t".join("%.17g" % v for v in r) for r in K) + "\n")
    return {"T": base, "P": str(ph), "K": str(kin), "out": str(tmp_path / "out"), "tmp": tmp_path, "Kmat": K}


def run(files, args):
    sub = {"T": files["T"], "P": files["P"], "K": files["K"]}
    cmd = [BIN, "-lmm", "2", "-outdir", files["out"], "-o", "res"] + [sub.get(a, a) for a in args]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    return r


def no_output(files):
    return not os.path.exists(os.path.join(files["out"], "res.assoc.txt")) and not os.path.exists(os.path.join(files["out"], "res.log.txt"))


GOOD = ["--kmers_table", "T", "--kmers_len", "31", "-p", "P", "-k", "K", "--mac", "2", "-maf", "0.05"]


@pytest.mark.parametrize("extra", [["-bfile", "B"], ["--bfiles", "LIST"], ["--columns", "LIST"], ["-bfile", "B", "--columns", "LIST"]])
def test_excludes_the_plink_inputs(files, extra):
    r = run(files, GOOD + extra)
    assert r.returncode == 1 and "--kmers_table excludes -bfile, --bfiles and --columns" in r.stderr, r.stderr
    assert no_output(files)


@pytest.mark.parametrize("drop", ["--kmers_len", "-p", "-k"])
def test_missing_required_option(files, drop):
    args = list(GOOD)
    i = args.index(drop)
    del args[i:i + 2]
    r = run(files, args)
    assert r.returncode == 1 and "--kmers_table needs --kmers_len, -p and -k" in r.stderr, r.stderr
    assert no_output(files)


def test_table_options_need_the_table(files):
    for opt, val in (("--kmers_len", "31"), ("-p", "P"), ("--mac", "5"), ("--best", "10"), ("--device", "0")):
        r = run(files, ["-bfile", "B", "-k", "K", opt, val])
        assert r.returncode == 1 and "needs --kmers_table" in r.stderr, r.stderr


@pytest.mark.parametrize("args,msg", [
    (["--best", "0"], "--best 0"),
    (["--best", "x"], "is not a whole number"),
    (["--best", "-3"], "is not a whole number"),
    (["--mac", "1.5"], "is not a whole number"),
    (["-n", "0"], "is not a whole number within 1"),
    (["--kmers_len", "32"], "kmer length has to be between 10-31"),
    (["-maf", "abc"], "failed to parse"),
])
def test_bad_values(files, args, msg):
    base = list(GOOD)
    if args[0] in base:
        i = base.index(args[0])
        del base[i:i + 2]
    r = run(files, base + args)
    assert r.returncode == 1 and msg in r.stderr, r.stderr
    assert no_output(files)


def test_lmm_1_stays_refused(files):
    cmd = [BIN, "-lmm", "1", "-outdir", files["out"], "-o", "res", "--kmers_table", files["T"], "--kmers_len", "31", "-p", files["P"], "-k", files["K"]]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "only -lmm 2" in r.stderr and no_output(files)


def test_missing_files(files):
    for key, gone in (("--kmers_table", str(files["tmp"] / "absent")), ("-p", str(files["tmp"] / "absent.tsv")), ("-k", str(files["tmp"] / "absent.kin"))):
        args = list(GOOD)
        args[args.index(key) + 1] = gone
        r = run(files, args)
        assert r.returncode == 1 and "Couldn't find file: " + gone in r.stderr, r.stderr
        assert no_output(files)


def test_kinship_of_another_size(files):
    K = files["Kmat"]
    small = files["tmp"] / "small.kin"
    small.write_text("\n".join("\t".join("%.17g" % v for v in r[:S - 1]) for r in K[:S - 1]) + "\n")
    args = list(GOOD)
    args[args.index("-k") + 1] = str(small)
    r = run(files, args)
    assert r.returncode == 1 and "has 11 rows, the phenotype file has 12 individuals" in r.stderr, r.stderr
    assert no_output(files)


def test_unknown_accession_and_missing_column(files):
    ph = files["tmp"] / "other.tsv"
    ph.write_text(open(files["P"]).read().replace("acc", "ACC", 1).replace("acc", "nobody", 1))
    args = list(GOOD)
    args[args.index("-p") + 1] = str(ph)
    r = run(files, args)
    assert r.returncode != 0 and "nobody" in r.stderr and no_output(files), r.stderr
    r = run(files, GOOD + ["-n", "3"])
    assert r.returncode == 1 and "has no phenotype column 3" in r.stderr and no_output(files), r.stderr


def test_a_value_that_a_fam_reads_as_missing_is_refused(files):
    lines = open(files["P"]).read().split("\n")
    f = lines[3].split("\t")
    lines[3] = "\t".join([f[0], "-9.0", f[2]])
    ph = files["tmp"] / "minus9.tsv"
    ph.write_text("\n".join(lines))
    args = list(GOOD)
    args[args.index("-p") + 1] = str(ph)
    r = run(files, args)
    assert r.returncode == 1 and "a .fam reads as missing" in r.stderr and f[0] in r.stderr and no_output(files), r.stderr


def test_well_formed_command_line(files, have_gpu):
    """Without a GPU: the device error and exit code 3 of every tool here, after every file was read, and no output. With one
    the same line runs."""
    r = run(files, GOOD)
    if have_gpu:
        assert r.returncode == 0, r.stderr
        lines = open(os.path.join(files["out"], "res.assoc.txt")).read().split("\n")
        assert lines[0].startswith("chr\trs\t") and len(lines) > 10 and all(len(l.split("\t")[1]) == 31 for l in lines[1:-1])
    else:
        assert r.returncode == 3 and "no HIP device available: libkgwas has no CPU fallback" in r.stderr, r.stderr
        assert no_output(files)


def test_help_names_the_table_mode():
    r = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--kmers_table" in r.stderr and "--best" in r.stderr and "--mac" in r.stderr


def test_entry_points():
    assert capi.ABI_VERSION == 15 and lib.kgwas_abi_version() == 15
    for s in ("kgwas_lmm_test_table", "kgwas_lmm_run_table"):
        assert s in capi.SYMBOLS and hasattr(lib, s)
    y = np.zeros(4)
    assert lib.kgwas_lmm_test_table(None, capi.ptr(y), None, None, 4, 1, 0.0, 10, *([None] * 9)) == capi.KGWAS_ERR_ARG
    assert lib.kgwas_lmm_run_table(b"k", b"t", 31, b"p", 1, 5, 0.05, 0, 1e-5, 1e5, 0, 0, b"o", None) == capi.KGWAS_ERR_ARG
    assert lib.kgwas_lmm_run_table(b"k", b"t", 31, b"p", 0, 5, 0.05, 10, 1e-5, 1e5, 0, 0, b"o", None) == capi.KGWAS_ERR_ARG
    assert lib.kgwas_lmm_run_table(None, b"t", 31, b"p", 1, 5, 0.05, 10, 1e-5, 1e5, 0, 0, b"o", None) == capi.KGWAS_ERR_ARG


def test_model_fixture():
    """The fixture of test_gpu_lmm_lrt_table.py::test_against_model_E: every row is tested, and the two numpy models agree on
    its dosage columns within 1e-10 (a hundredth of the GPU tolerance's cap, as for the other lmm fixtures)."""
    K, y, bits, pick, rows = T.model_fixture()
    assert T.tested_rule(bits.sum(axis=1), T.MODEL_S, T.MODEL_MIN_COUNT, T.MODEL_MAF).all()
    assert len(set(pick.tolist())) == T.MODEL_S and rows.shape == (T.MODEL_ROWS, 1 + 2)
    # the table holds the bits at the picked columns
    got = np.array([[(int(r[1 + int(c) // 64]) >> (int(c) % 64)) & 1 for c in pick] for r in rows], bool)
    assert (got == bits).all()
    xs = T.model_dosages(bits)
    a, l0a = M.lrt_R(K, y, xs)
    b, l0b = M.lrt_E(K, y, xs)
    gap = max(float(np.abs(a - b).max()), abs(l0a - l0b))
    print("table fixture S=67: max |LRT_R - LRT_E| = %.3e, |l0_R - l0_E| = %.3e, LRT range %.3g..%.3g" % (np.abs(a - b).max(), abs(l0a - l0b), a.min(), a.max()))
    assert gap <= 1e-10


def test_tested_rule_edges():
    """The numpy statement of the rule at the counts where its two halves part: S = 50, maf = 0.1 keeps 45 carriers and drops 5."""
    t = T.tested_rule(np.arange(51), 50, 5, 0.1)
    assert not t[5] and t[6] and t[45] and not t[46] and not t[0] and not t[50]
    t = T.tested_rule(np.arange(68), 67, 5, 0.05)
    assert list(np.flatnonzero(t)) == list(range(5, 63))
