"""A literal Python restatement of the reference's filter_kmers (src/filter_kmers.cpp, src/kmer_general.cpp): the yardstick of
tests/test_filter_kmers.py and tests/test_gpu_filter_kmers.py (test infrastructure, not product).

restate(table_base, kmers_file) follows main() step by step and returns what the tool does: ("ok", stderr, output bytes),
("exit", status, stderr) or ("abort", what, stderr) for an uncaught std::logic_error."""
import os

import numpy as np

WLEN = 64


class RefAbort(Exception):
    def __init__(self, what, stderr=""):
        super().__init__(what)
        self.what, self.stderr = what, stderr


def words_of(data: bytes):
    """`fin >> word`: words split on any whitespace."""
    return [w.decode("latin-1") for w in data.split()]


def kmer_reverse_complement(x: int, k_len: int) -> int:  # kmer_general.h:102-109
    M = (1 << 64) - 1
    x = ((x & 0xFFFFFFFF00000000) >> 32) | ((x & 0x00000000FFFFFFFF) << 32)
    x &= M
    x = ((x & 0xFFFF0000FFFF0000) >> 16) | ((x & 0x0000FFFF0000FFFF) << 16)
    x &= M
    x = ((x & 0xFF00FF00FF00FF00) >> 8) | ((x & 0x00FF00FF00FF00FF) << 8)
    x &= M
    x = ((x & 0xF0F0F0F0F0F0F0F0) >> 4) | ((x & 0x0F0F0F0F0F0F0F0F) << 4)
    x &= M
    x = ((x & 0xCCCCCCCCCCCCCCCC) >> 2) | ((x & 0x3333333333333333) << 2)
    x &= M
    return ((~x) & M) >> (64 - k_len - k_len)


def kmer2bits(k: str) -> int:  # kmer_general.cpp:260-283
    b = 0
    for i in range(len(k)):
        c = k[len(k) - i - 1]
        if c == "A":
            d = 0
        elif c == "C":
            d = 1
        elif c == "G":
            d = 2
        elif c == "T":
            d = 3
        else:
            raise RefAbort("Ilegal kmer")
        b |= d << (i * 2)
    bt = kmer_reverse_complement(b, len(k))
    return bt if bt < b else b


def bits2kmer31(w: int, k: int) -> str:  # kmer_general.cpp:77-87
    res = ["X"] * k
    for i in range(k):
        res[k - 1 - i] = "ACGT"[w & 3]
        w >>= 2
    return "".join(res)


def read_and_sort_kmers(data: bytes):  # filter_kmers.cpp:30-50
    kmer_list, kmer_len, err = [], 0, ""
    for index, word in enumerate(words_of(data)):
        if index == 0:
            kmer_len = len(word)
        if len(word) != kmer_len:
            err += "all kmers should be of the same size: %s\n" % word
            raise RefAbort("kmers of different size", err)
        kmer_list.append(kmer2bits(word))
    return sorted(kmer_list), kmer_len


def merge_join(sorted_kmers, keys):
    """The loop of filter_kmers.cpp:152-177 as written: the file rows it emits, in order."""
    keys = [int(x) for x in keys]
    out = []
    i_kl, i_kt, n, rows = 0, 0, len(sorted_kmers), len(keys)
    advance_row, cur = True, None
    while i_kl < n and (i_kt < rows or not advance_row):
        if advance_row:
            cur = keys[i_kt]
            i_kt += 1
            advance_row = False
        if cur == sorted_kmers[i_kl]:
            out.append(i_kt - 1)
            i_kl += 1
            advance_row = True
        elif cur < sorted_kmers[i_kl]:
            advance_row = True
        else:
            i_kl += 1
    return out


def line_of(row, k, S_f) -> str:
    """One output line, literally: bits2kmer31(key, k), then "\\t" << bit per accession, then "\\n"."""
    s = bits2kmer31(int(row[0]), k)
    for c in range(S_f):
        s += "\t" + str((int(row[(c >> 6) + 1]) >> (c & (WLEN - 1))) & 1)
    return s + "\n"


def header(names) -> bytes:
    return ("kmer" + "".join("\t" + n for n in names) + "\n").encode()


def lines_bytes(rows, k, S_f) -> bytes:
    """line_of for many rows at once (numpy; tests pin it to line_of)."""
    rows = np.asarray(rows, np.uint64).reshape(-1, 1 + (S_f + 63) // 64)
    m, width = len(rows), k + 2 * S_f + 1
    buf = np.empty((m, width), np.uint8)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    for j in range(k):
        buf[:, j] = acgt[((rows[:, 0] >> np.uint64(2 * (k - 1 - j))) & np.uint64(3)).astype(np.int64)]
    if S_f:
        bits = np.unpackbits(np.ascontiguousarray(rows[:, 1:]).view(np.uint8).reshape(m, 8 * (rows.shape[1] - 1)), axis=1,
                             bitorder="little")[:, :S_f]
        buf[:, k:k + 2 * S_f:2] = ord("\t")
        buf[:, k + 1:k + 2 * S_f:2] = ord("0") + bits
    buf[:, -1] = ord("\n")
    return buf.tobytes()


def expected_output(names, k, rows, sorted_kmers):
    """(emitted file rows, output file bytes) of the tool on table rows `rows` (n x (1 + W_f)) and a sorted list."""
    emitted = merge_join(sorted_kmers, rows[:, 0] if len(rows) else [])
    sel = rows[emitted] if emitted else np.zeros((0, rows.shape[1] if rows.ndim == 2 else 1), np.uint64)
    return np.asarray(emitted, np.uint64), header(names) + lines_bytes(sel, k, len(names))


def restate(table_base: str, kmers_file: str):
    """main() from the file checks on (the options are given)."""
    err = ""
    for f in (table_base + ".names", table_base + ".table", kmers_file):
        if not os.path.isfile(f) or not os.access(f, os.R_OK):
            return ("exit", 1, "Couldn't find file: %s\n" % f)
    try:
        with open(kmers_file, "rb") as f:
            sorted_kmers, kmer_len = read_and_sort_kmers(f.read())
        if not sorted_kmers:
            return ("exit", 1, "kmers file is empty\n")
        with open(table_base + ".names", "rb") as f:
            names = words_of(f.read())
        words_per_kmer = (len(names) + WLEN - 1) // WLEN
        with open(table_base + ".table", "rb") as f:
            data = f.read()
        if len(data) <= 16:
            return ("exit", 1, "table file is too small\n")
        prefix = int(np.frombuffer(data[0:4], np.uint32)[0])
        file_accession_number = int(np.frombuffer(data[4:12], np.uint64)[0])
        file_kmer_len = int(np.frombuffer(data[12:16], np.uint32)[0])
        left_in_file = len(data) - 16
        if prefix != 0xDDCCBBAA:
            raise RefAbort("Incorrect prefix")
        if file_accession_number != len(names):
            raise RefAbort("number of accession in file not as defined in class")
        if file_kmer_len != kmer_len:
            raise RefAbort("kmer length in table and in list are not the same")
        size_per_kmer = 8 * (1 + words_per_kmer)
        if left_in_file % size_per_kmer != 0:
            raise RefAbort("size of file not valid")
        kmer_number = left_in_file // size_per_kmer
        err += "We have %d\n" % kmer_number
        rows = np.frombuffer(data[16:], np.uint64).reshape(kmer_number, 1 + words_per_kmer)
        _, out = expected_output(names, kmer_len, rows, sorted_kmers)
        return ("ok", err, out)
    except RefAbort as e:
        return ("abort", e.what, err + e.stderr)
