"""lmm_lrt --kmers_table without a GPU: the refusals of the tool (each a non-zero exit, its message, and no output file), the
device error of a well-formed command line on a machine without a GPU, the new entry points, the model gap of the fixture
that test_gpu_lmm_lrt_table.py checks against model E, and the geometry of the fixtures of test_gpu_lmm_lrt_table_scale.py: which
blocks and scan rounds (lmm_table_scan_kernel) their pieces and select launches reach."""
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


# ---- the fixtures of test_gpu_lmm_lrt_table_scale.py: numpy only ----------------------------------------------------------------
def test_kmer_words_inverts_kmer_text():
    words = np.array([0, 1, (1 << 62) - 1, 0x2AAAAAAAAAAAAAAA, 123456789012345], np.uint64)
    assert T.kmer_words([T.kmer_text(w) for w in words]).tolist() == words.tolist()
    assert T.kmer_words([]).shape == (0,)


def test_block_fixture_kinds():
    """The block-structured table holds every kind of block, the rows that must not be tested come from both sides of the rule
    and are mostly not empty, and the table's words hold the bits."""
    bits, pick, rows, rule = T.scale_fixture()
    n_rows, S, mc = T.SCALE_ROWS, T.SCALE_S, T.SCALE_MIN_COUNT
    assert bits.shape == (n_rows, S) and rows.shape == (n_rows, 3) and n_rows == (1 << 18) + (1 << 16) + 77
    assert (np.diff(rows[:, 0].astype(np.int64)) > 0).all()
    sample = np.r_[0:300, 65500:65600, n_rows - 100:n_rows]
    got = np.array([[(int(rows[r, 1 + int(c) // 64]) >> (int(c) % 64)) & 1 for c in pick] for r in sample], bool)
    assert (got == bits[sample]).all()
    n1 = bits.sum(axis=1)
    for count in (0, S, mc - 1, S - mc + 1):
        assert ((n1 == count) & ~rule).sum() > n_rows // 8, "few untested rows with %d carriers" % count
    kinds = T.scale_kinds()
    (blocks,) = [r for p in T.scan_geometry(rule, n_rows) for r in [np.concatenate(p)]]
    assert len(blocks) == len(kinds) == 1281
    assert (blocks[kinds == T.FULL][:-1] == 256).all() and blocks[-1] == 77 and (blocks[kinds == T.EMPTY] == 0).all()
    for kind, at in ((T.FIRST, 0), (T.LAST, 255)):
        b = np.flatnonzero(kinds == kind)
        assert len(b) > 100 and (blocks[b] == 1).all() and rule[b * 256 + at].all()
    rnd = blocks[kinds == T.RANDOM]
    assert len(rnd) > 400 and 2 < rnd.mean() < 40 and rnd.max() < 256


@pytest.mark.parametrize("forced", T.SCALE_PIECES)
def test_block_fixture_geometry(forced):
    """What lmm_table_scan_kernel meets in test_pieces_beyond_one_scan_round at this KGWAS_LMM_PIECE_ROWS."""
    bits, pick, rows, rule = T.scale_fixture()
    n_rows = T.SCALE_ROWS
    piece = T.piece_rows(n_rows, forced, rows.shape[1])
    geo = T.scan_geometry(rule, piece)
    sizes = [min(piece, n_rows - pos) for pos in range(0, n_rows, piece)]
    print("KGWAS_LMM_PIECE_ROWS %s: pieces of %s rows, rounds x blocks %s" % (forced, sizes, [[len(r) for r in p] for p in geo]))
    # a lost carry shows in the very next round: no round without a tested row
    assert all(r.sum() > 0 for p in geo for r in p)
    later = [r for p in geo for r in p[1:]]
    if forced is None:
        assert sizes == [1 << 18, 65613] and [[len(r) for r in p] for p in geo] == [[256] * 4, [256, 1]]
    elif forced == T.MAX_PIECE:
        assert sizes == [n_rows] and [len(r) for r in geo[0]] == [256] * 5 + [1]
    elif forced == 65536:
        assert sizes == [65536] * 5 + [77] and [[len(r) for r in p] for p in geo] == [[256]] * 5 + [[1]]
    else:
        assert sizes == [65537] * 5 + [72] and [[len(r) for r in p] for p in geo] == [[256, 1]] * 5 + [[1]]
        assert all(p[1].tolist() == [1] for p in geo[:5]), "the second round's one row is not tested"
    if forced in (None, T.MAX_PIECE):
        # a full, an empty and a single-row block (the row first and last in its block) in a round other than the first
        assert any((r == 256).any() for r in later) and any((r == 0).any() for r in later) and any((r == 1).any() for r in later)
        flags = np.concatenate([np.r_[rule[pos:pos + piece], np.zeros(-len(rule[pos:pos + piece]) % 256, bool)].reshape(-1, 256)[256:]
                                for pos in range(0, n_rows, piece)])
        alone = flags[flags.sum(axis=1) == 1]
        assert alone[:, 0].any() and alone[:, 255].any()
        # a partial last round and a partial last block
        assert any(len(p[-1]) < 256 for p in geo) and any(s % 256 for s in sizes)


def test_sub_chunk_and_select_fixture_geometry():
    """The tables of the sub-chunk and select tests: one piece each, the tested rows they need, and the scan rounds of their
    select launches (256 pairs per block, 256 blocks per round)."""
    for n_rows, least, ties in ((T.CHUNK_ROWS, T.CHUNK_MIN_TESTED, False), (T.SELECT_OPEN_ROWS, T.SELECT_OPEN_MIN_TESTED, False),
                                (T.SELECT_ROWS, T.SELECT_MIN_TESTED, False), (T.SELECT_ROWS, T.SELECT_MIN_TESTED, True)):
        tested = int(T.scale_tested(T.scale_bits(n_rows, ties)).sum())
        assert least <= tested < n_rows and T.piece_rows(n_rows, None, 3) == n_rows
        assert len(T.scan_geometry(np.ones(n_rows, bool), n_rows)[0]) == 1, "the front end of these tables has one round"
    tested = int(T.scale_tested(T.scale_bits(T.CHUNK_ROWS)).sum())
    assert -(-tested // 10240) == 3 and tested % 10240 and tested <= 65536
    # open heaps: one launch of 32 x tested pairs, two rounds, the second partial
    tested = int(T.scale_tested(T.scale_bits(T.SELECT_OPEN_ROWS)).sum())
    (launch,) = T.scan_geometry(np.ones(32 * tested, bool), 32 * tested)
    assert 32 * tested > 65536 and tested <= 10240 and [len(r) for r in launch] == [256, -(-32 * tested // 256) - 256]
    # closed heaps: launches of 32 x 3008 pairs = 376 blocks, two rounds, then the rest; the repeated rows a sub-chunk apart
    (launch,) = T.scan_geometry(np.ones(32 * T.SELECT_CHUNK, bool), 32 * T.SELECT_CHUNK)
    assert [len(r) for r in launch] == [256, 120]
    rule = T.scale_tested(T.scale_bits(T.SELECT_ROWS, True))
    assert int(rule.sum()) > 2 * T.SELECT_CHUNK
    place = np.cumsum(rule) - 1
    a, b = np.arange(T.TIE_FROM, T.TIE_FROM + T.TIE_COUNT), np.arange(T.TIE_TO, T.TIE_TO + T.TIE_COUNT)
    assert (T.scale_bits(T.SELECT_ROWS, True)[a] == T.scale_bits(T.SELECT_ROWS, True)[b]).all() and rule[a].sum() >= 40
    assert (place[a] // T.SELECT_CHUNK == 0).all() and (place[b] // T.SELECT_CHUNK == 1).all()


def test_scan_kernel_guards_its_lds_between_rounds():
    """lmm_table_scan_kernel writes s_wave once per round of 256 blocks and every wave reads all of it: a barrier must stand between
    the write and the reads, and one between the reads and the end of the round, or a wave that is a round ahead overwrites what a
    slower wave still reads. The outputs do not show the second one missing (without it the kernel passed every table test on an
    MI355X: the window is shorter than the next round's global load), so the source is read here."""
    src = open(os.path.join(os.path.dirname(os.path.abspath(capi.__file__)), "csrc", "lmm_table_kernels.hip")).read()
    src = "\n".join(l.split("//")[0] for l in src.split("\n"))
    body = src[src.index("lmm_table_scan_kernel("):]
    body = body[body.index("for (uint32_t b0"):body.index("total[0] = carry")]
    write, first_read, last_read = body.index("s_wave[wave] ="), body.index("s_wave[w]"), body.rindex("s_wave[w]")
    assert write < first_read
    assert "__syncthreads()" in body[write:first_read], "no barrier between the write of s_wave and its reads"
    assert "__syncthreads()" in body[last_read:], "no barrier between the reads of s_wave and the next round's write"
