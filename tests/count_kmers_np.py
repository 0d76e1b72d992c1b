"""count_kmers_with_strand restated (include/kgwas.h): the rules of the count twice over, independently of each other
and of the library, and a reader of FASTA / FASTQ text.

  literal(reads, k, ci, cx)   pure Python: one window at a time, its code and its reverse complement's letter by letter, a dict
  closed(reads, k, ci, cx)    NumPy: the codes of all windows of the joined reads at once, np.unique with counts

Both return {"words": the file's words in order, "counts": the eight counters}. Reads are bytes; every byte other than A, C, G, T
(either case) ends a stretch of bases."""
import numpy as np

U = np.uint64
FLAG_CANON, FLAG_NON = 1 << 62, 2 << 62
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


class FormatError(Exception):
    pass


def literal(reads, k, ci, cx):
    seen = {}      # key -> [count, flags]
    oriented = {}  # the window's own code -> its key
    windows = 0
    for read in reads:
        s = bytes(read).decode("latin-1").upper()
        for i in range(len(s) - k + 1):
            w = s[i:i + k]
            if any(ch not in CODE for ch in w):
                continue
            a = 0
            for ch in w:
                a = a * 4 + CODE[ch]
            b = 0
            for ch in reversed(w):
                b = b * 4 + (3 - CODE[ch])
            key, flag = (a, FLAG_CANON) if a < b else (b, FLAG_NON)
            e = seen.setdefault(key, [0, 0])
            e[0] += 1
            e[1] |= flag
            oriented[a] = key
            windows += 1
    kept = {key for key, (c, _) in seen.items() if ci <= c <= cx}
    words = [key | seen[key][1] for key in sorted(kept)]
    by_flag = [sum(1 for w in words if w >> 62 == f) for f in range(4)]
    counts = (len(kept), len(oriented), sum(1 for key in oriented.values() if key in kept), *by_flag, windows)
    return {"words": words, "counts": counts}


def _window_codes(c, k, rc):
    """codes[i] of the k bases from i on, for every i (garbage where the window leaves the array or meets a separator): windows of
    1, 2, 4, ... bases put together. rc: of the reverse complement."""
    n = len(c)
    by_len = {1: (U(3) - c) if rc else c.copy()}
    L = 1
    while 2 * L <= k:
        x = by_len[L]
        sh = np.zeros(n, U)
        sh[:n - L] = x[L:]
        by_len[2 * L] = (sh << U(2 * L)) | x if rc else (x << U(2 * L)) | sh
        L *= 2
    out, have = None, 0
    for L in sorted(by_len, reverse=True):
        if have + L > k:
            continue
        x = by_len[L]
        if out is None:
            out = x.copy()
        else:
            sh = np.zeros(n, U)
            sh[:n - have] = x[have:]
            out = (sh << U(2 * have)) | out if rc else (out << U(2 * L)) | sh
        have += L
    assert have == k
    return out


def stream_of(reads):
    """The reads as one byte stream, a separator behind each."""
    return b"".join(bytes(r) + b"\n" for r in reads)


def closed(reads, k, ci, cx):
    return closed_stream(np.frombuffer(stream_of(reads), np.uint8), k, ci, cx)


def closed_stream(stream, k, ci, cx):
    lut = np.full(256, 4, np.uint8)
    for ch, v in CODE.items():
        lut[ord(ch)] = lut[ord(ch.lower())] = v
    c8 = lut[np.asarray(stream, np.uint8)]
    n = len(c8)
    empty = {"words": [], "counts": (0,) * 8}
    if n < k:
        return empty
    bad = np.concatenate([[0], np.cumsum(c8 == 4)])
    ok = (bad[k:] - bad[:n - k + 1]) == 0  # window i: no separator among its k bytes
    c = (c8 & 3).astype(U)
    a = _window_codes(c, k, False)[:n - k + 1][ok]
    b = _window_codes(c, k, True)[:n - k + 1][ok]
    if len(a) == 0:
        return empty
    canon = a < b
    sort_words = (np.where(canon, a, b) << U(1)) | (~canon).astype(U)
    uw, cnt = np.unique(sort_words, return_counts=True)  # one entry per oriented k-mer
    k_all = uw >> U(1)
    head = np.concatenate([[True], k_all[1:] != k_all[:-1]])
    first = np.flatnonzero(head)
    keys = k_all[first]
    count = np.add.reduceat(cnt, first)
    has0 = np.zeros(len(keys), bool)
    has1 = np.zeros(len(keys), bool)
    idx = np.cumsum(head) - 1
    has0[idx[(uw & U(1)) == 0]] = True
    has1[idx[(uw & U(1)) == 1]] = True
    keep = (count >= ci) & (count <= cx)
    flags = (has0.astype(U) << U(62)) | (has1.astype(U) << U(63))
    words = (keys | flags)[keep]
    f = (words >> U(62)).astype(np.int64)
    counts = (int(keep.sum()), len(uw), int((has0[keep].astype(np.int64) + has1[keep]).sum()),
              *[int((f == v).sum()) for v in range(4)], int(len(a)))
    return {"words": [int(w) for w in words] if len(words) < 100000 else words, "counts": counts}


def file_bytes(res):
    return np.asarray(res["words"], "<u8").tobytes()


def summary_of(counts):
    """The tool's stdout."""
    return ("Canonized kmers:\t%d\nNon-canon kmers:\t%d\nNon-canon kmers found:\t%d\nflag\t0\tcount is\t%d\nflag\t1\tcount is\t%d\n"
            "flag\t2\tcount is\t%d\nflag\t3\tcount is\t%d\nkmers to save:\t%d\n" % (counts[0], counts[1], counts[2], counts[3], counts[4],
                                                                                  counts[5], counts[6], counts[0])).encode()


def read_fastx(data, name="<input>"):
    """The reads of one FASTA or FASTQ file's bytes, by the tool's rules."""
    if len(data) == 0:
        return []
    if data[:1] not in (b">", b"@"):
        raise FormatError("%s: neither FASTA nor FASTQ" % name)
    lines = data.split(b"\n")
    if lines[-1] == b"":
        lines.pop()  # (the final newline; without one the last line is simply the last line)
    lines = [l[:-1] if l.endswith(b"\r") else l for l in lines]
    reads = []
    if data[:1] == b"@":
        if len(lines) % 4:
            raise FormatError("%s: the last FASTQ record has fewer than four lines" % name)
        for i in range(0, len(lines), 4):
            if lines[i][:1] != b"@" or lines[i + 2][:1] != b"+":
                raise FormatError("%s: a FASTQ record does not have '@' and '+' at the head of its first and third line" % name)
            reads.append(lines[i + 1])
    else:
        cur = None
        for l in lines:
            if l[:1] == b">":
                if cur is not None:
                    reads.append(b"".join(cur))
                cur = []
            else:
                cur.append(l)
        if cur is not None:
            reads.append(b"".join(cur))
    return reads
