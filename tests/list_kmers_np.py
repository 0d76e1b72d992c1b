"""A literal Python restatement of the reference's list_kmers_found_in_multiple_samples (src/list_kmers_found_in_multiple_samples.cpp,
KmersSingleDataBaseSortedFile in src/kmers_single_database.cpp:90-177, read_accessions_path_list and bits2kmer31 in
src/kmer_general.cpp): the yardstick of tests/test_list_kmers.py and tests/test_gpu_list_kmers.py (test infrastructure, not product).

literal follows the reader with its held last word and flag, the 5001 windows, one dict per window with the packed adders, the sorted
distinct keys, the counts and the decisions, step by step; closed is the closed form of the same result in NumPy over (window, key)
pairs (fast enough for the large cases; the tests pin it to literal). restate follows main() from the file checks on and returns what
the tool leaves: status or abort text, the summary lines on stderr and the bytes of every output file. The three inputs on which the
reference has undefined behaviour raise RefUB in literal and closed and end restate with the tool's documented refusal."""
import numpy as np

from build_table_np import MASK, NULL_KEY, RefAbort, is_file_exist, read_accessions_path_list, read_words, step_of, windows_of

STEPS = 5000
EXTS = ("", ".no_pass_kmers", ".shareness", ".stats.only_canonical", ".stats.only_non_canonical", ".stats.both")
NO_PASS_HEADER = "kmer\tcount_all\tcanonical\tnon-canonical\tboth\n"
FLAG0_WHAT = "a k-mer word without strand flags (flag 0) in: %s"
ABOVE_N_WHAT = "k-mer %s is counted more often than there are files (%d): a file repeats it"
TOO_MANY_WHAT = "too many k-mer files: %d (at most 1048575)"


class RefUB(Exception):
    """An input on which the reference has undefined behaviour, the first one it meets. kind "flag0": file = index of the file with a
    used flag-0 word in the lowest window (the first such file in list order); kind "above_n": key = the smallest (window, key) counted
    more than N times, in a window below that one."""

    def __init__(self, kind, file=None, key=None):
        super().__init__("%s file=%s key=%s" % (kind, file, key))
        self.kind, self.file, self.key = kind, file, key


def bits2kmer31(w: int, k: int) -> str:
    return "".join("ACGT"[(w >> (2 * (k - 1 - i))) & 3] for i in range(k))


class SortedFile:
    """KmersSingleDataBaseSortedFile with its flags: the next word is held in m_last_kmer (masked) and m_flag."""

    def __init__(self, words, path="<memory>"):
        self.words = [int(w) for w in words]
        self.kmers_in_file = len(self.words)
        if self.kmers_in_file > 0:
            self.kmers_count = 0
            self.read_kmer()
        else:
            raise RefAbort("sorted kmer file is empty: " + path)

    def read_kmer(self):
        self.last_kmer = self.words[self.kmers_count]
        self.flag = self.last_kmer >> 62
        self.last_kmer &= MASK
        self.kmers_count += 1

    def load_kmers_upto_x(self, threshold):
        kmers, flags = [], []
        while self.last_kmer <= threshold and self.kmers_count < self.kmers_in_file:
            kmers.append(self.last_kmer)
            flags.append(self.flag)
            self.read_kmer()
        if self.last_kmer <= threshold and self.kmers_count == self.kmers_in_file:
            if self.last_kmer != NULL_KEY:
                flags.append(self.flag)
                kmers.append(self.last_kmer)
            self.last_kmer = NULL_KEY
            self.flag = NULL_KEY
        return kmers, flags


def passes(count_all, count_canon, count_non_canon, count_both, mac, p):
    """None below MAC, else the strand rule in IEEE double (:185-189)."""
    if count_all < mac:
        return None
    with np.errstate(all="ignore"):
        t = np.ceil(np.float64(p) * np.float64(count_all))
        return bool(np.float64(count_canon + count_both) >= t and np.float64(count_non_canon + count_both) >= t)


def _result(N):
    return dict(passed=[], no_pass=[], shareness=np.zeros(N + 1, np.uint64), only_canonical=np.zeros((N + 1, N + 1), np.uint64),
                only_non_canonical=np.zeros((N + 1, N + 1), np.uint64), both=np.zeros((N + 1, N + 1), np.uint64), low=0)


def literal(acc_words, k, mac, p):
    """main()'s loop (:146-201). Returns passed (keys in output order), no_pass (key, all, canon, non-canon, both), the statistics and
    low (keys below MAC)."""
    files = [SortedFile(w) for w in acc_words]
    N = len(files)
    res = _result(N)
    adders = [1 + (1 << 20), 1 + (1 << 40), 1]
    for step_i in range(1, STEPS + 2):
        kmers_hash, unique_kmers = {}, []
        current_threshold = step_of(k) * step_i
        for i, f in enumerate(files):
            kmers, flags = f.load_kmers_upto_x(current_threshold)
            for kmer, flag in zip(kmers, flags):
                if flag == 0:
                    raise RefUB("flag0", file=i)  # adders[-1]
                if kmer not in kmers_hash:
                    kmers_hash[kmer] = adders[flag - 1]
                    unique_kmers.append(kmer)
                else:
                    kmers_hash[kmer] += adders[flag - 1]
        unique_kmers.sort()
        for kmer in unique_kmers:
            counts = kmers_hash[kmer]
            count_all = counts & 0xFFFFF
            count_canon = (counts >> 20) & 0xFFFFF
            count_non_canon = (counts >> 40) & 0xFFFFF
            count_both = count_all - count_canon - count_non_canon
            if count_all > N:
                raise RefUB("above_n", key=kmer)  # outside the matrices
            res["only_canonical"][count_all][count_canon] += 1
            res["only_non_canonical"][count_all][count_non_canon] += 1
            res["both"][count_all][count_both] += 1
            ok = passes(count_all, count_canon, count_non_canon, count_both, mac, p)
            if ok is None:
                res["low"] += 1
            elif ok:
                res["passed"].append(kmer)
                res["shareness"][count_all] += 1
            else:
                res["no_pass"].append((kmer, count_all, count_canon, count_non_canon, count_both))
    return res


def closed(acc_words, k, mac, p):
    """The closed form: the counted items are the pairs (window, key) of the words with window <= 5001, w(j) = max(1, ceil(max(keys
    0..j) / step)) within their file; output order is (window, key)."""
    N = len(acc_words)
    res = _result(N)
    step = step_of(k)
    xs, ws, fs = [], [], []
    flag0 = (STEPS + 2, None)
    for i, words in enumerate(acc_words):
        words = np.asarray(words, np.uint64)
        x, w = windows_of(words, step)
        used = w <= STEPS + 1
        f = (words >> np.uint64(62)).astype(np.int64)[used]
        x, w = x[used], w[used]
        if (f == 0).any():  # the first one the reference meets: the lowest window, then the first file
            flag0 = min(flag0, (int(w[f == 0].min()), i))
        xs.append(x[f != 0])
        ws.append(w[f != 0])
        fs.append(f[f != 0])
    x, w, f = (np.concatenate(a) if a else np.zeros(0, t) for a, t in ((xs, np.uint64), (ws, np.int64), (fs, np.int64)))
    if len(x) == 0:
        if flag0[1] is not None:
            raise RefUB("flag0", file=flag0[1])
        return res
    order = np.lexsort((x, w))
    x, w, f = x[order], w[order], f[order]
    head = np.concatenate([[True], (x[1:] != x[:-1]) | (w[1:] != w[:-1])])
    gid = np.cumsum(head) - 1
    n = int(gid[-1]) + 1
    keys = x[head]
    count_all = np.bincount(gid, minlength=n)
    canon = np.bincount(gid, weights=f == 1, minlength=n).astype(np.int64)
    non = np.bincount(gid, weights=f == 2, minlength=n).astype(np.int64)
    both = count_all - canon - non
    above = (count_all > N) & (w[head] < flag0[0])  # (a window is written before the next one is read)
    if above.any():
        raise RefUB("above_n", key=int(keys[np.argmax(above)]))
    if flag0[1] is not None:
        raise RefUB("flag0", file=flag0[1])
    np.add.at(res["only_canonical"], (count_all, canon), 1)
    np.add.at(res["only_non_canonical"], (count_all, non), 1)
    np.add.at(res["both"], (count_all, both), 1)
    with np.errstate(all="ignore"):
        t = np.ceil(np.float64(p) * count_all.astype(np.float64))
        mac_ok = count_all.astype(np.uint64) >= np.uint64(mac)
        ok = mac_ok & ((canon + both).astype(np.float64) >= t) & ((non + both).astype(np.float64) >= t)
    res["low"] = int((~mac_ok).sum())
    res["passed"] = [int(v) for v in keys[ok]]
    np.add.at(res["shareness"], count_all[ok], 1)
    bad = mac_ok & ~ok
    res["no_pass"] = [tuple(int(v) for v in r) for r in zip(keys[bad], count_all[bad], canon[bad], non[bad], both[bad])]
    return res


def same(a, b):
    return (a["passed"] == b["passed"] and a["no_pass"] == b["no_pass"] and a["low"] == b["low"] and
            all(np.array_equal(a[m], b[m]) for m in ("shareness", "only_canonical", "only_non_canonical", "both")))


def counts_of(res):
    """(passed, passed MAC but not the strand filter, below MAC)"""
    return len(res["passed"]), len(res["no_pass"]), res["low"]


def matrix_bytes(M) -> bytes:
    return "".join("\t".join(map(str, row)) + "\n" for row in np.asarray(M).tolist()).encode()


def files_of(res, k):
    """The bytes of the output files, by extension (EXTS)."""
    return {
        "": np.array(res["passed"], "<u8").tobytes(),
        ".no_pass_kmers": (NO_PASS_HEADER + "".join("%s\t%d\t%d\t%d\t%d\n" % ((bits2kmer31(r[0], k),) + tuple(r[1:])) for r in res["no_pass"])).encode(),
        ".shareness": ("kmer appearance\tcount\n" + "".join("%d\t%d\n" % (i, int(v)) for i, v in enumerate(res["shareness"]))).encode(),
        ".stats.only_canonical": matrix_bytes(res["only_canonical"]),
        ".stats.only_non_canonical": matrix_bytes(res["only_non_canonical"]),
        ".stats.both": matrix_bytes(res["both"]),
    }


def summary_of(res) -> str:
    """The three closing lines of stderr ("kmers lower than MAC" is the true count here, not the reference's uninitialised variable)."""
    n_pass, n_no_pass, low = counts_of(res)
    return "kmers lower than MAC:\t%d\npassed kmers:\t%d\npassed MAC bot not pass strand filter:\t%d\n" % (low, n_pass, n_no_pass)


def restate(list_file, kmer_len, mac, p, fn=closed):
    """main() from the file checks on (the options are given). Returns a dict: kind "exit" (status, stderr) / "abort" (what) / "ok"
    (stderr = the summary lines, files = the outputs' bytes by extension, counts). Outputs exist only for kind "ok" (an abort in the
    middle of the counting leaves unspecified ones behind)."""
    if not is_file_exist(list_file):
        return dict(kind="exit", status=1, stderr="Couldn't find file: %s\n" % list_file)
    if kmer_len > 31 or kmer_len < 10:
        return dict(kind="exit", status=1, stderr="kmer length has to be between 10-31\n")
    with open(list_file, "rb") as f:
        paths = [path for path, _ in read_accessions_path_list(f.read())]
    acc, cache = [], {}
    for path in paths:  # each file is opened as it is checked
        if not is_file_exist(path):
            return dict(kind="exit", status=1, stderr="Couldn't find file: %s\n" % path)
        if path not in cache:
            cache[path] = read_words(path)
        if len(cache[path]) == 0:
            return dict(kind="abort", what="sorted kmer file is empty: " + path)
        acc.append(cache[path])
    if len(acc) >= 1 << 20:
        return dict(kind="abort", what=TOO_MANY_WHAT % len(acc))
    try:
        res = fn(acc, kmer_len, mac, p)
    except RefUB as e:
        if e.kind == "flag0":
            return dict(kind="abort", what=FLAG0_WHAT % paths[e.file])
        return dict(kind="abort", what=ABOVE_N_WHAT % (bits2kmer31(e.key, kmer_len), len(acc)))
    return dict(kind="ok", stderr=summary_of(res), files=files_of(res, kmer_len), counts=counts_of(res), res=res)
