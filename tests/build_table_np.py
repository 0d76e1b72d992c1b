"""A literal Python restatement of the reference's build_kmers_table (src/build_kmers_table.cpp, src/kmers_merge_multiple_databaes.cpp,
KmersSingleDataBaseSortedFile in src/kmers_single_database.cpp:90-177, read_accessions_path_list in src/kmer_general.cpp:32-43): the
yardstick of tests/test_build_table.py and tests/test_gpu_build_table.py (test infrastructure, not product).

literal_rows follows the reader with its held last word and the 5001 windows with a dict per window, step by step; closed_rows is the
closed form of the same result in NumPy (fast enough for the large cases; the tests pin it to literal_rows). restate follows main()
from the file checks on and returns what the tool leaves: status or abort text, stderr, <o>.names and <o>.table bytes."""
import os

import numpy as np

WLEN = 64
MASK = 0x3FFFFFFFFFFFFFFF
NULL_KEY = 0xFFFFFFFFFFFFFFFF
TOTAL_ITER = 5000


class RefAbort(Exception):
    def __init__(self, what):
        super().__init__(what)
        self.what = what


def step_of(k: int) -> int:  # kmers_step_to_threshold (kmer_general.cpp:255-258): threshold = step * iteration
    return ((1 << (2 * k)) - 1) // TOTAL_ITER + 1


def words_of_bytes(data: bytes) -> np.ndarray:
    """The raw 64-bit words of a file: size >> 3 of them, trailing bytes ignored."""
    return np.frombuffer(data[:len(data) >> 3 << 3], "<u8")


class SortedFile:
    """KmersSingleDataBaseSortedFile: the next word is held in m_last_kmer, already masked."""

    def __init__(self, words, path="<memory>"):
        self.words = [int(w) for w in words]
        self.kmers_in_file = len(self.words)
        if self.kmers_in_file > 0:
            self.kmers_count = 0
            self.read_kmer()
        else:
            raise RefAbort("sorted kmer file is empty: " + path)

    def read_kmer(self):
        self.last_kmer = self.words[self.kmers_count] & MASK
        self.kmers_count += 1

    def load_kmers_upto_x(self, threshold):
        kmers = []
        while self.last_kmer <= threshold and self.kmers_count < self.kmers_in_file:
            kmers.append(self.last_kmer)
            self.read_kmer()
        if self.last_kmer <= threshold and self.kmers_count == self.kmers_in_file:
            if self.last_kmer != NULL_KEY:
                kmers.append(self.last_kmer)
            self.last_kmer = NULL_KEY
        return kmers


def literal_rows(all_words, acc_words, k):
    """main()'s loop (build_kmers_table.cpp:99-103) over load_kmers / output_to_table: the table's rows, n x (1 + ceil(S / 64))."""
    possible = SortedFile(all_words)
    files = [SortedFile(w) for w in acc_words]
    hash_words = (len(files) + WLEN - 1) // WLEN
    step = step_of(k)
    out = []
    for it in range(1, TOTAL_ITER + 2):
        threshold = step * it
        container_kmers = possible.load_kmers_upto_x(threshold)
        container = [0] * (hash_words * len(container_kmers))
        kmers_to_index = {}
        for kmer_index, kmer in enumerate(container_kmers):
            if kmer not in kmers_to_index:  # dense_hash_map::insert keeps the first
                kmers_to_index[kmer] = kmer_index * hash_words
        for acc_i, f in enumerate(files):
            hashmap_i, bit_i = acc_i // WLEN, acc_i % WLEN
            for kmer in f.load_kmers_upto_x(threshold):
                idx = kmers_to_index.get(kmer)
                if idx is not None:
                    container[idx + hashmap_i] |= 1 << bit_i
        for kmer_index, kmer in enumerate(container_kmers):
            out.append([kmer] + container[kmer_index * hash_words:(kmer_index + 1) * hash_words])
    return np.array(out, np.uint64).reshape(len(out), 1 + hash_words)


def windows_of(words, step):
    """(masked keys, window of each word): w(j) = max(1, ceil(max(keys[0..j]) / step))."""
    x = np.asarray(words, np.uint64) & np.uint64(MASK)
    if len(x) == 0:
        return x, np.zeros(0, np.int64)
    pm = np.maximum.accumulate(x)
    w = np.where(pm == 0, np.uint64(1), (pm - np.uint64(1)) // np.uint64(step) + np.uint64(1))
    return x, w.astype(np.int64)


def closed_rows(all_words, acc_words, k):
    """The closed form: rows = the all-k-mers words with window <= 5001, in file order; bit c of the row of word a is set iff a is
    the first all-k-mers word with its pair (window, key) and accession c's file has a word with the same pair."""
    step = step_of(k)
    S = len(acc_words)
    hash_words = (S + WLEN - 1) // WLEN
    xa, wa = windows_of(all_words, step)
    used = wa <= TOTAL_ITER + 1
    xa, wa = xa[used], wa[used]
    rows = np.zeros((len(xa), 1 + hash_words), np.uint64)
    rows[:, 0] = xa
    if len(xa) == 0:
        return rows
    ux = np.unique(xa)

    def codes(x, w):  # a pair as one integer: window * len(ux) + rank of the key among the all-k-mers keys (others dropped)
        r = np.searchsorted(ux, x)
        ok = r < len(ux)
        ok[ok] = ux[r[ok]] == x[ok]
        return w[ok] * len(ux) + r[ok]

    uc, first = np.unique(codes(xa, wa), return_index=True)
    for c, words in enumerate(acc_words):
        xc, wc = windows_of(words, step)
        keep = wc <= TOTAL_ITER + 1
        hit = np.isin(uc, codes(xc[keep], wc[keep]))
        rows[first[hit], 1 + c // WLEN] |= np.uint64(1 << (c % WLEN))
    return rows


def table_bytes(rows, S, k) -> bytes:
    """output_table_header + the rows (kmers_merge_multiple_databaes.cpp:54-73)."""
    return b"\xAA\xBB\xCC\xDD" + np.uint64(S).tobytes() + np.uint32(k).tobytes() + np.ascontiguousarray(rows, np.uint64).tobytes()


def read_accessions_path_list(data: bytes):
    """`while (fin >> path) { fin >> name; ... }`: a last path without a name keeps the name read before it."""
    toks = [t.decode("latin-1") for t in data.split()]
    res, name = [], ""
    for i in range(0, len(toks), 2):
        if i + 1 < len(toks):
            name = toks[i + 1]
        res.append((toks[i], name))
    return res


def is_file_exist(path) -> bool:
    return os.path.isfile(path) and os.access(path, os.R_OK)


def read_words(path):
    with open(path, "rb") as f:
        return words_of_bytes(f.read())


# stderr of the tool here: the reference's three milestones (its per-window progress lines are deliberately not printed)
MILESTONES = ("Create merger\n", "Opens file\n", "close file\n")


def restate(list_file, kmer_len, all_kmers, rows_fn=closed_rows):
    """main() from the file checks on (the options are given). Returns a dict: kind "exit" (status, stderr) / "abort" (what,
    stderr) / "ok" (stderr), and names / table: the bytes left in <o>.names / <o>.table (None: never created)."""
    for f in (list_file, all_kmers):
        if not is_file_exist(f):
            return dict(kind="exit", status=1, stderr="Couldn't find file: %s\n" % f, names=None, table=None)
    if kmer_len > 31 or kmer_len < 10:
        return dict(kind="exit", status=1, stderr="kmer length has to be between 10-31\n", names=None, table=None)
    with open(list_file, "rb") as f:
        handles = read_accessions_path_list(f.read())
    names = b""
    for path, name in handles:
        names += name.encode("latin-1") + b"\n"
        if not is_file_exist(path):
            return dict(kind="exit", status=1, stderr="Couldn't find file: %s\n" % path, names=names, table=None)
    err = MILESTONES[0]
    try:
        possible = read_words(all_kmers)
        if len(possible) == 0:
            raise RefAbort("sorted kmer file is empty: " + all_kmers)
        acc = []
        for path, _ in handles:
            w = read_words(path)
            if len(w) == 0:
                raise RefAbort("sorted kmer file is empty: " + path)
            acc.append(w)
    except RefAbort as e:
        return dict(kind="abort", what=e.what, stderr=err, names=names, table=None)
    err += MILESTONES[1]
    rows = rows_fn(possible, acc, kmer_len)
    err += MILESTONES[2]
    return dict(kind="ok", stderr=err, names=names, table=table_bytes(rows, len(acc), kmer_len), rows=rows)
