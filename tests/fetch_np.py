"""A brute-force model of fetch_reads (include/kgwas.h): the stream split at newlines, every window's canonical code looked up in a
dict (min_hits >= 1); and the tool's three outputs from parsed records. Slow and plain on purpose; test_fetch_model.py pins it with hand-worked
cases."""
import numpy as np

FETCH_RECORD = np.dtype([("read", np.uint64), ("n_hits", np.uint32), ("first_pos", np.uint32), ("kmer", np.uint32), ("strand", np.uint8), ("pad", np.uint8, (3,))])
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def revcomp(w):
    return "".join(COMP[c] for c in reversed(w))


def code(w):
    c = 0
    for ch in w:
        c = c << 2 | CODE[ch]
    return c


def canonical(w):
    return min(code(w), code(revcomp(w)))


def reads_of(stream: bytes):
    """The reads: read r ends at the r-th newline; a last run without a newline is a read too."""
    runs = stream.split(b"\n")
    if runs[-1] == b"":
        runs.pop()
    return runs


def per_read(stream: bytes, words):
    """([(n_hits, first_pos, kmer, strand) per read; first_pos None without a hit], kmer_windows) for the queries `words` (letters as
    spelled). Every window of k bases has its code and its reverse complement's rolled along, and the smaller looked up."""
    k = len(words[0])
    table, spelled = {}, [code(w) for w in words]
    for i, w in enumerate(words):
        assert len(w) == k and set(w) <= set(CODE) and canonical(w) not in table
        table[canonical(w)] = i
    windows = np.zeros(len(words), np.uint64)
    mask, top = (1 << (2 * k)) - 1, 2 * (k - 1)
    out = []
    for read in reads_of(stream):
        n_hits, first, run, f, rc = 0, (None, 0, 0), 0, 0, 0
        for p, ch in enumerate(read.decode("latin-1").upper()):
            c = CODE.get(ch)
            if c is None:
                run = 0
                continue
            f, rc, run = (f << 2 | c) & mask, rc >> 2 | (3 - c) << top, run + 1
            if run < k:
                continue
            i = table.get(min(f, rc))
            if i is None:
                continue
            windows[i] += 1
            n_hits += 1
            if n_hits == 1:
                first = (p - k + 1, i, 0 if f == spelled[i] else 1)
        out.append((n_hits,) + first)
    return out, windows


def fetch(stream: bytes, words, min_hits=1, reads=None):
    """(records, kmer_windows); `reads`: per_read's result, where it is at hand."""
    reads, windows = per_read(stream, words) if reads is None else reads
    out = [(r, n, p, i, s, (0, 0, 0)) for r, (n, p, i, s) in enumerate(reads) if n >= min_hits]
    return (np.array(out, FETCH_RECORD) if out else np.zeros(0, FETCH_RECORD)), windows


def parse_records(data: bytes):
    """The records of a FASTA / FASTQ file: [(raw bytes with a final newline, name, sequence bytes)]."""
    if not data:
        return []
    lines = data.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    chop = lambda l: l[:-1] if l.endswith(b"\r") else l
    out = []
    if data[:1] == b"@":
        assert len(lines) % 4 == 0
        for i in range(0, len(lines), 4):
            assert lines[i][:1] == b"@" and lines[i + 2][:1] == b"+"
            out.append([b"\n".join(lines[i:i + 4]) + b"\n", lines[i], chop(lines[i + 1])])
    else:
        assert data[:1] == b">"
        for l in lines:
            if l[:1] == b">":
                out.append([b"", l, b""])
            else:
                out[-1][2] += chop(l)
            out[-1][0] += l + b"\n"
    name = lambda head: head[1:].replace(b"\t", b" ").replace(b"\r", b" ").split(b" ")[0].decode()
    return [(raw, name(head), seq) for raw, head, seq in out]


def tool(reads: bytes, words, min_hits=1, mates: bytes | None = None, max_reads_per_kmer=0):
    """The tool's outputs: {"reads": [bytes per output file], "tsv": bytes, "log": ["kmer <text> <written> <windows>" lines]}."""
    files = [parse_records(reads)] + ([parse_records(mates)] if mates is not None else [])
    m = len(files)
    assert all(len(f) == len(files[0]) for f in files)
    stream = b"".join(files[f][u][2] + b"\n" for u in range(len(files[0])) for f in range(m))
    rec, windows = fetch(stream, words, min_hits)
    by_unit = {}
    for r in rec:
        by_unit.setdefault(int(r["read"]) // m, []).append(r)
    written = [0] * len(words)
    outs = [b"" for _ in range(m)]
    tsv = b"read\tmate\tn_hits\tfirst_pos\tkmer\tstrand\n"
    for u in sorted(by_unit):
        owner = int(by_unit[u][0]["kmer"])
        if max_reads_per_kmer and written[owner] >= max_reads_per_kmer:
            continue
        written[owner] += 1
        for f in range(m):
            outs[f] += files[f][u][0]
        for r in by_unit[u]:
            f = int(r["read"]) % m
            tsv += ("%s\t%d\t%d\t%d\t%s\t%s\n" % (files[f][u][1], f + 1 if m == 2 else 0, r["n_hits"], r["first_pos"] + 1, words[int(r["kmer"])],
                                                  "-" if r["strand"] else "+")).encode()
    log = ["kmer\t%s\t%d\t%d" % (w, written[i], windows[i]) for i, w in enumerate(words)]
    return {"reads": outs, "tsv": tsv, "log": log, "records": rec}
