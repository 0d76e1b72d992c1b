"""A brute-force model of locate_kmers in plain Python / NumPy (include/kgwas.h states the definitions).

Every window is compared with every pattern letter by letter: the letters are one-hot rows, so the product of the windows' matrix
and the patterns' counts the equal letters of each (window, pattern) pair, and a pair is a hit iff k minus that count is at most d.
Nothing here knows of half keys, sorted lists or pieces. Beside it: the FASTA rules, the three formats of the --kmers file and
the bytes of the tool's output and of its log's per-k-mer lines."""
import numpy as np

RECORD = np.dtype([("pos", np.uint64), ("kmer", np.uint32), ("strand", np.uint8), ("mismatches", np.uint8), ("offset", np.uint8), ("pad", np.uint8)])
COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}
_LETTER = np.full(256, 4, np.uint8)
for _i, _c in enumerate("ACGT"):
    _LETTER[ord(_c)] = _LETTER[ord(_c.lower())] = _i


def revcomp(word):
    return "".join(COMPLEMENT[c] for c in reversed(word))


def canonical(word):
    return min(word, revcomp(word))  # (A < C < G < T as letters and as codes)


def patterns_of(queries):
    """[(letters, kmer, strand)]: the query as spelled, +, and unless it is its own reverse complement, that one, -"""
    out = []
    for i, q in enumerate(queries):
        out.append((q, i, 0))
        if revcomp(q) != q:
            out.append((revcomp(q), i, 1))
    return out


def _one_hot(letters):
    """letters[n, k] in 0..4 -> float32[n, 4 k], a 1 where position j holds letter c (4: nowhere)"""
    return (letters[:, :, None] == np.arange(4, dtype=np.uint8)).reshape(len(letters), -1).astype(np.float32)


def locate(stream, queries, d, chunk=512):
    """The records of the base stream `stream` (bytes) for the queries (strings of one length) with at most d mismatches, in
    (pos, kmer, strand) order, and the count of windows of k base bytes."""
    k = len(queries[0])
    assert all(len(q) == k for q in queries) and len({canonical(q) for q in queries}) == len(queries)
    pats = patterns_of(queries)
    plet = _LETTER[np.frombuffer("".join(p[0] for p in pats).encode(), np.uint8)].reshape(len(pats), k)
    P = _one_hot(plet).T.copy()
    letters = _LETTER[np.frombuffer(bytes(stream), np.uint8)]
    if len(letters) < k:
        return np.zeros(0, RECORD), 0
    win = np.lib.stride_tricks.sliding_window_view(letters, k)
    valid = np.flatnonzero((win < 4).all(axis=1))
    found = []
    for c0 in range(0, len(valid), chunk):
        at = valid[c0:c0 + chunk]
        equal = _one_hot(win[at]) @ P  # [windows, patterns]: the letters the pair shares
        w, p = np.nonzero(equal >= k - d)
        for wi, pi in zip(w.tolist(), p.tolist()):
            differ = np.flatnonzero(win[at[wi]] != plet[pi])
            assert len(differ) <= d and len(differ) == k - int(equal[wi, pi])
            found.append((int(at[wi]), pats[pi][1], pats[pi][2], len(differ), int(differ[0]) + 1 if len(differ) else 0))
    found.sort()
    rec = np.zeros(len(found), RECORD)
    for name, col in zip(("pos", "kmer", "strand", "mismatches", "offset"), zip(*found) if found else [()] * 5):
        rec[name] = col
    return rec, len(valid)


# ---- the tool --------------------------------------------------------------------------------------------------------------------------

class Refused(Exception):
    pass


def read_fasta(data, path="ref"):
    """[(name, sequence bytes)] of a FASTA file's bytes, by the tool's rules"""
    if not data or data[:1] != b">":
        raise Refused(path + ": not FASTA")
    lines = data.split(b"\n")
    if lines[-1] == b"":
        lines.pop()  # (the final newline's)
    contigs = []
    for no, line in enumerate(lines, 1):
        if line.endswith(b"\r"):
            line = line[:-1]
        if line[:1] == b">":
            head = line[1:].decode("latin-1")
            name = head.replace("\t", " ").split(" ")[0]
            if not name:
                raise Refused("%s line %d: a contig without a name" % (path, no))
            if name in [c[0] for c in contigs]:
                raise Refused("%s line %d: the contig '%s' is given twice" % (path, no, name))
            contigs.append([name, b""])
        else:
            contigs[-1][1] += line
    if not any(seq for _, seq in contigs):
        raise Refused(path + ": no sequence")
    return [(n, s) for n, s in contigs]


def read_kmers(text, k, path="kmers"):
    """([(k-mer, p_lrt text or None)], has_p) of a --kmers file's text"""
    lines = text.split("\n")
    fields = [[f for f in l.replace("\r", " ").replace("\t", " ").split(" ") if f] for l in lines]
    head = fields[0] if fields else []
    table = "rs" in head or "kmer" in head
    distinct = table and "rs" not in head
    has_p = table and "p_lrt" in head
    col = head.index("rs" if "rs" in head else "kmer") if table else 0
    out, seen = [], {}
    for no, fl in list(enumerate(fields, 1))[1 if table else 0:]:
        if not fl:
            continue
        at = "%s line %d: " % (path, no)
        if table and len(fl) <= max(col, head.index("p_lrt") if has_p else 0):
            raise Refused(at + "too few fields (%d, the header has %d)" % (len(fl), len(head)))
        if not table and len(fl) != 1:
            raise Refused(at + "%d fields: a list of k-mers has one k-mer per line" % len(fl))
        w = fl[col]
        if len(w) != k:
            raise Refused(at + "k-mer '%s' has length %d, not %d" % (w, len(w), k))
        if set(w) - set("ACGT"):
            raise Refused(at + "k-mer '%s' has a letter other than A, C, G, T" % w)
        if canonical(w) in seen:
            if distinct:
                continue
            raise Refused(at + "duplicate k-mer '%s' (the k-mer of line %d)" % (w, seen[canonical(w)]))
        seen[canonical(w)] = no
        out.append((w, fl[head.index("p_lrt")] if has_p else None))
    if not out:
        raise Refused(path + ": no k-mer")
    return out, has_p


def run(fasta, kmers_text, k, d, max_per_kmer=100):
    """(the output's bytes, the log's per-k-mer lines, [(kept, found)], windows tested) of the tool"""
    queries, has_p = read_kmers(kmers_text, k)
    contigs = read_fasta(fasta)
    words = [q for q, _ in queries]
    hits = [[] for _ in queries]  # per k-mer, in contig order
    windows = 0
    for name, seq in contigs:
        rec, n_win = locate(seq, words, d)
        windows += n_win
        for r in rec:  # (pos, kmer, strand) order: within a k-mer by position, then + before -
            hits[int(r["kmer"])].append((name, seq, r))
    out = "kmer\tcontig\tpos\tstrand\tmismatches\toffset\tref\talt" + ("\tp_lrt\n" if has_p else "\n")
    log, counts = "", []
    for (w, p), mine in zip(queries, hits):
        kept = mine if not max_per_kmer else mine[:max_per_kmer]
        for name, seq, r in kept:
            pos, off, strand = int(r["pos"]), int(r["offset"]), int(r["strand"])
            ref = alt = "."
            if r["mismatches"]:
                ref = chr(seq[pos + off - 1]).upper()
                alt = w[off - 1] if strand == 0 else COMPLEMENT[w[k - off]]
                spelled = (w if strand == 0 else revcomp(w))
                assert spelled[off - 1] == alt and alt != ref
            out += "\t".join([w, name, str(pos + 1), "+-"[strand], str(int(r["mismatches"])), str(off), ref, alt] + ([p] if has_p else [])) + "\n"
        log += "kmer\t%s\t%d\t%d\n" % (w, len(kept), len(mine))
        counts.append((len(kept), len(mine)))
    return out.encode(), log.encode(), counts, windows
