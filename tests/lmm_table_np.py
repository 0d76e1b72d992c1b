"""Shared by the test_gpu_lmm_lrt_table*.py modules and test_lmm_lrt_table_cli.py (test infrastructure, not product): small k-mers
tables with chosen presence counts, the tested-set rule of lmm_lrt --kmers_table restated in numpy, the one fixture whose model gap
the CPU module asserts and whose statistics the GPU module checks against model E, and the block-structured fixture of
test_gpu_lmm_lrt_table_scale.py with the geometry (pieces, blocks of 256 rows, scan rounds of 256 blocks) the CPU module asserts."""
import functools

import numpy as np

import lmm_lrt_np as M

K_LEN = 31
# rows of M.fixture's G, from which K comes: more than n, so that K is not rank-starved (600 rows at n = 1135 leave
# 534 zero eigenvalues)
KIN_ROWS = {5: 400, 50: 400, 64: 400, 65: 400, 67: 400, 241: 600, 256: 600, 257: 600, 511: 1000, 512: 1000, 513: 1000, 1135: 1400}


def kmer_text(word, k=K_LEN):
    """bits2kmer31: the most significant base first"""
    return "".join("ACGT"[(int(word) >> (2 * (k - 1 - i))) & 3] for i in range(k))


def kmer_words(texts, k=K_LEN):
    """the inverse of kmer_text for a list of texts of k bases each, as uint64"""
    if not len(texts):
        return np.zeros(0, np.uint64)
    chars = np.frombuffer("".join(texts).encode(), np.uint8).reshape(len(texts), k)
    code = np.full(256, 255, np.uint8)
    code[np.frombuffer(b"ACGT", np.uint8)] = np.arange(4, dtype=np.uint8)
    base = code[chars]
    assert (base < 4).all()
    return (base.astype(np.uint64) << (2 * (k - 1 - np.arange(k))).astype(np.uint64)).sum(axis=1, dtype=np.uint64)


def table_from_bits(bits, S_f, pick, seed):
    """bits (rows x S, phenotype order) -> table rows [kmer, W_f words] with accession i of the phenotype order in column
    pick[i]; the other S_f - S columns get random bits; k-mer words ascending and unique."""
    bits = np.asarray(bits, bool)
    n_rows, S = bits.shape
    rng = np.random.default_rng([seed, S_f, n_rows])
    W = (S_f + 63) // 64
    pad = np.zeros((n_rows, W * 64), bool)
    pad[:, :S_f] = rng.random((n_rows, S_f)) < 0.5
    pad[:, np.asarray(pick)] = bits
    words = np.packbits(pad.reshape(n_rows, W, 64), axis=2, bitorder="little").view(np.uint64).reshape(n_rows, W)
    rows = np.empty((n_rows, 1 + W), np.uint64)
    rows[:, 0] = np.sort(rng.choice(1 << 40, size=n_rows, replace=False)).astype(np.uint64)
    rows[:, 1:] = words
    return rows


def random_bits(n_rows, S, seed, lo=0.01, hi=0.99):
    rng = np.random.default_rng([seed, S, n_rows, 3])
    f = rng.uniform(lo, hi, n_rows)
    return rng.random((n_rows, S)) < f[:, None]


def bits_with_counts(counts, S, seed):
    """one row per entry of counts, with exactly that many carriers, at random places"""
    rng = np.random.default_rng([seed, S, 5])
    bits = np.zeros((len(counts), S), bool)
    for r, c in enumerate(counts):
        bits[r, rng.permutation(S)[:c]] = True
    return bits


def af_of(n1, S):
    """lmm_prep_kernel's af of a presence row with n1 carriers among S, operation for operation"""
    mean = (2 * (S - np.asarray(n1, np.int64))).astype(np.float64) / np.float64(S)
    return 0.5 * mean


def tested_rule(n1, S, min_count, maf):
    """The rule in float64 numpy, operation for operation: kmers_table_to_bed's MAC filter and lmm_prep_kernel's af filter."""
    n1 = np.asarray(n1, np.int64)
    written = (S >= min_count) & (n1 >= min_count) & (n1 <= S - min_count)
    af = af_of(n1, S)
    return written & (n1 != 0) & (n1 != S) & (np.minimum(af, 1.0 - af) >= maf)


def kinship_and_phenotype(S):
    _, K, y = M.fixture(S, KIN_ROWS[S], 3.0)
    return K, y


# ---- the fixture checked against model E: S = 67 of a table of 70 accessions, 40 rows that are all tested at MAC 5, MAF 0.05 ----
MODEL_S, MODEL_S_F, MODEL_ROWS, MODEL_MIN_COUNT, MODEL_MAF = 67, 70, 40, 5, 0.05


@functools.lru_cache(maxsize=None)
def model_fixture():
    """(K, y, bits, pick, rows): bits 40 x 67 in phenotype order, frequencies 0.2 .. 0.8"""
    K, y = kinship_and_phenotype(MODEL_S)
    bits = random_bits(MODEL_ROWS, MODEL_S, 77, 0.2, 0.8)
    pick = np.random.default_rng(77).permutation(MODEL_S_F)[:MODEL_S]
    return K, y, bits, pick, table_from_bits(bits, MODEL_S_F, pick, 77)


def model_dosages(bits):
    """the .bed's values: absence 2, presence 0"""
    return 2.0 * (1.0 - np.asarray(bits, np.float64))


# ---- the block-structured fixture: tested flags with a prescribed shape per block of 256 rows (LMM_TABLE_BLOCK) -----------------
BLOCK = 256                      # rows per block of the flag and emit kernels, pairs per block of the select kernels
ROUND = 256                      # blocks per round of lmm_table_scan_kernel
DEFAULT_PIECE = 1 << 18          # table_pass's piece of a table of up to 32 words per row
MAX_PIECE = 1 << 20              # the most KGWAS_LMM_PIECE_ROWS takes
FULL, EMPTY, FIRST, LAST, RANDOM = range(5)  # a block's kind: all rows tested, none, its first row alone, its last row alone, random
SCALE_S, SCALE_S_F, SCALE_MIN_COUNT, SCALE_MAF = 67, 70, 5, 0.05
SCALE_ROWS = (1 << 18) + (1 << 16) + 77
SCALE_PIECES = (None, MAX_PIECE, 65536, 65537)  # KGWAS_LMM_PIECE_ROWS of the scale tests; None: unset
_KIND_CYCLE = (FULL, RANDOM, EMPTY, FIRST, RANDOM, LAST, RANDOM, EMPTY, RANDOM, FULL, RANDOM, RANDOM, FIRST, EMPTY, LAST, RANDOM)


def scale_kinds(n_rows=SCALE_ROWS):
    """The kind of every block of SCALE_ROWS rows: a cycle of 16, and where a piece of SCALE_PIECES starts a scan round with one
    row (pieces of 65537 rows: rows 65536, 131073, 196610, 262147 and 327684, the last in the table's partial last block) a kind
    that has that row tested."""
    n_blocks = -(-n_rows // BLOCK)
    kinds = np.array([_KIND_CYCLE[b % len(_KIND_CYCLE)] for b in range(n_blocks)], np.uint8)
    kinds[256] = FIRST
    kinds[[512, 768, 1024, n_blocks - 1]] = FULL
    return kinds


def block_counts(kinds, n_rows, S, min_count, maf, seed, density=0.05):
    """Carrier counts n1 per row whose tested flags under tested_rule(n1, S, min_count, maf) have the kind of every block of 256
    rows (the last block may be partial; its LAST is the table's last row). Rows of a RANDOM block are tested with probability
    `density`. A tested row's count is drawn from every count the rule keeps, an untested row's from 0, S, min_count - 1 and
    S - min_count + 1 in turn."""
    rng = np.random.default_rng([seed, S, n_rows, 7])
    counts = np.arange(S + 1)
    kept = counts[tested_rule(counts, S, min_count, maf)]
    out = np.array([0, S, min_count - 1, S - min_count + 1])
    assert len(kept) and not tested_rule(out, S, min_count, maf).any()
    r = np.arange(n_rows)
    kind = np.asarray(kinds)[r // BLOCK]
    last_of_block = np.minimum((r // BLOCK + 1) * BLOCK, n_rows) - 1
    want = (kind == FULL) | ((kind == FIRST) & (r % BLOCK == 0)) | ((kind == LAST) & (r == last_of_block))
    want |= (kind == RANDOM) & (rng.random(n_rows) < density)
    n1 = np.where(want, kept[rng.integers(0, len(kept), n_rows)], out[(r + r // BLOCK) % 4])
    assert (tested_rule(n1, S, min_count, maf) == want).all()
    return n1


def bits_of_counts(n1, S, seed):
    """bits_with_counts for many rows: row r has n1[r] carriers at random places"""
    rng = np.random.default_rng([seed, S, len(n1), 9])
    return rng.permuted(np.arange(S)[None, :] < np.asarray(n1)[:, None], axis=1)


@functools.lru_cache(maxsize=None)
def scale_fixture():
    """(bits, pick, rows, rule): SCALE_ROWS rows x 67 accessions of a table of 70, tested flags by scale_kinds()"""
    n1 = block_counts(scale_kinds(), SCALE_ROWS, SCALE_S, SCALE_MIN_COUNT, SCALE_MAF, 5)
    bits = bits_of_counts(n1, SCALE_S, 5)
    pick = np.random.default_rng(5).permutation(SCALE_S_F)[:SCALE_S]
    rows = table_from_bits(bits, SCALE_S_F, pick, 5)
    rule = tested_rule(bits.sum(axis=1), SCALE_S, SCALE_MIN_COUNT, SCALE_MAF)
    for a in (bits, pick, rows, rule):
        a.setflags(write=False)
    return bits, pick, rows, rule


def piece_rows(n_rows, forced, words_per_row):
    """table_pass's piece: rows per piece for a table of n_rows rows of 1 + W_f words; forced: KGWAS_LMM_PIECE_ROWS or None"""
    piece = max(1024, min(DEFAULT_PIECE, (64 << 20) // (8 * words_per_row)))
    if forced:
        piece = min(forced, MAX_PIECE)
    return min(piece, max(n_rows, 1))


def scan_geometry(flags, piece):
    """What lmm_table_scan_kernel sees when `flags` (one per row or per pair) are cut into pieces (launches) of `piece`: per piece
    the list of its rounds, each the array of the counts of its up to 256 blocks of up to 256 flags."""
    flags = np.asarray(flags, bool)
    out = []
    for pos in range(0, len(flags), piece):
        f = flags[pos:pos + piece]
        pad = np.zeros(-(-len(f) // BLOCK) * BLOCK, bool)
        pad[:len(f)] = f
        cnt = pad.reshape(-1, BLOCK).sum(axis=1)
        out.append([cnt[b:b + ROUND] for b in range(0, len(cnt), ROUND)])
    return out


# ---- the tables of the sub-chunk and select tests: S = 67 of 70, MAC 5, MAF 0.05, frequencies 0.1 .. 0.9, one piece each --------
CHUNK_ROWS, CHUNK_MIN_TESTED = 30000, 25000          # more tested rows than two default chunks of 10240
SELECT_OPEN_ROWS, SELECT_OPEN_MIN_TESTED = 2400, 2100  # 32 columns x tested rows > 65536 pairs in one select launch
SELECT_ROWS, SELECT_MIN_TESTED, SELECT_CHUNK = 6500, 6100, 3008  # 32 x 3008 = 96256 pairs, 376 blocks, in the first two launches
TIE_FROM, TIE_TO, TIE_COUNT = 10, 4000, 50           # rows 10 .. 59 are repeated as rows 4000 .. 4049, a sub-chunk further on


@functools.lru_cache(maxsize=None)
def scale_bits(n_rows, ties=False):
    """bits (n_rows x 67) of the sub-chunk and select tests; ties: with TIE_COUNT patterns repeated TIE_TO - TIE_FROM rows on"""
    bits = random_bits(n_rows, SCALE_S, 301, 0.1, 0.9)
    if ties:
        bits[TIE_TO:TIE_TO + TIE_COUNT] = bits[TIE_FROM:TIE_FROM + TIE_COUNT]
    bits.setflags(write=False)
    return bits


def scale_tested(bits):
    return tested_rule(np.asarray(bits).sum(axis=1), SCALE_S, SCALE_MIN_COUNT, SCALE_MAF)
