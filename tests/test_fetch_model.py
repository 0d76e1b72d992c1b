"""fetch_np, the model the GPU tests of fetch_reads compare with, pinned by hand-worked cases."""
import fetch_np as FN


def rows(rec):
    return [(int(r["read"]), int(r["n_hits"]), int(r["first_pos"]), int(r["kmer"]), int(r["strand"])) for r in rec]


def test_codes():
    assert FN.code("ACGT") == 0b00011011 and FN.revcomp("AACG") == "CGTT" and FN.canonical("TTT") == 0
    assert FN.FETCH_RECORD.itemsize == 24


def test_short_reads_and_a_read_of_exactly_k():
    rec, win = FN.fetch(b"ACG\nACGT\nCGT\n", ["ACGT"])  # the read shorter than k has no window; ACGT is its own reverse complement
    assert rows(rec) == [(1, 1, 0, 0, 0)] and win.tolist() == [1]


def test_n_inside_a_would_be_window_and_lower_case():
    rec, win = FN.fetch(b"AANCGGT\nttaaccgg\n", ["ACCGG", "AACGG"])
    # read 0: AANCG, ANCGG hold the N; read 1: TTAACCGG in lower case holds AACCG, ACCGG at 3
    assert rows(rec) == [(1, 1, 3, 0, 0)] and win.tolist() == [1, 0]


def test_a_palindrome_counts_as_strand_0():
    rec, win = FN.fetch(b"TTACGTAA\n", ["TACGTA"])  # even k, its own reverse complement
    assert rows(rec) == [(0, 1, 1, 0, 0)] and win.tolist() == [1]


def test_a_hit_on_strand_minus():
    rec, win = FN.fetch(b"GGCCGTTCC\n", ["AACGG"])  # CCGTT at 2 is its reverse complement
    assert rows(rec) == [(0, 1, 2, 0, 1)] and win.tolist() == [1]


def test_min_hits_two_with_one_and_with_two_hits():
    stream = b"TTAACGGTT\nAACGGTAACGG\nAACGGCCGTT\n"
    rec, win = FN.fetch(stream, ["AACGG"], 2)
    assert rows(rec) == [(1, 2, 0, 0, 0), (2, 2, 0, 0, 0)] and win.tolist() == [5]  # the one hit of read 0 is counted, the read not kept
    rec1, _ = FN.fetch(stream, ["AACGG"], 1)
    assert rows(rec1) == [(0, 1, 2, 0, 0), (1, 2, 0, 0, 0), (2, 2, 0, 0, 0)]


def test_an_empty_read_keeps_the_numbering_and_a_last_run_without_newline_is_a_read():
    rec, _ = FN.fetch(b"AACGG\n\n\nAACGG", ["AACGG"])
    assert rows(rec) == [(0, 1, 0, 0, 0), (3, 1, 0, 0, 0)]
    assert FN.reads_of(b"\n") == [b""] and FN.reads_of(b"") == [] and FN.reads_of(b"A\n\n") == [b"A", b""]


def test_a_window_does_not_cross_a_newline_and_cr_breaks_windows_inside_its_read():
    rec, win = FN.fetch(b"AAC\nGG\nAAC\rGG\nAACGG\r\n", ["AACGG"])
    assert rows(rec) == [(3, 1, 0, 0, 0)] and win.tolist() == [1]


def test_two_queries_first_hit_decides():
    rec, win = FN.fetch(b"TTTTTAACGG\n", ["AACGG", "AAAAA"])  # TTTTT at 0 is AAAAA on strand -
    assert rows(rec) == [(0, 2, 0, 1, 1)] and win.tolist() == [1, 1]


FQ1 = b"@r0 first\nTTAACGGTT\n+\nIIIIIIIII\n@r1\nCCCCCCC\n+\nIIIIIII\n@r2\tx\nAACGGAACGG\n+r2\nIIIIIIIIII\n@r3\nCCCCCC\n+\nIIIIII"
FQ2 = b"@r0/2\nCCCCCCC\n+\nIIIIIII\n@r1/2\nGGCCGTTCC\n+\nIIIIIIIII\n@r2/2\nAACGG\n+\nIIIII\n@r3/2\nGGGGGGG\n+\nIIIIIII\n"


def test_parse_records():
    r = FN.parse_records(FQ1)
    assert [(n, s) for _, n, s in r] == [("r0", b"TTAACGGTT"), ("r1", b"CCCCCCC"), ("r2", b"AACGGAACGG"), ("r3", b"CCCCCC")]
    assert r[3][0] == b"@r3\nCCCCCC\n+\nIIIIII\n" and b"".join(x[0] for x in r) == FQ1 + b"\n"
    fa = FN.parse_records(b">a b\r\nAC\r\nGT\r\n>c\nAA\n\nCC")
    assert [(n, s) for _, n, s in fa] == [("a", b"ACGT"), ("c", b"AACC")] and fa[0][0] == b">a b\r\nAC\r\nGT\r\n" and fa[1][0] == b">c\nAA\n\nCC\n"


def test_tool_single():
    t = FN.tool(FQ1, ["AACGG"])
    assert t["reads"] == [b"@r0 first\nTTAACGGTT\n+\nIIIIIIIII\n@r2\tx\nAACGGAACGG\n+r2\nIIIIIIIIII\n"]
    assert t["tsv"] == b"read\tmate\tn_hits\tfirst_pos\tkmer\tstrand\nr0\t0\t1\t3\tAACGG\t+\nr2\t0\t2\t1\tAACGG\t+\n"
    assert t["log"] == ["kmer\tAACGG\t2\t3"]


def test_tool_pairs_kept_through_mate_1_mate_2_and_both():
    t = FN.tool(FQ1, ["AACGG"], mates=FQ2)
    # pair 0 through mate 1, pair 1 through mate 2 only (strand -), pair 2 through both, pair 3 not at all
    assert t["tsv"] == (b"read\tmate\tn_hits\tfirst_pos\tkmer\tstrand\nr0\t1\t1\t3\tAACGG\t+\nr1/2\t2\t1\t3\tAACGG\t-\n"
                        b"r2\t1\t2\t1\tAACGG\t+\nr2/2\t2\t1\t1\tAACGG\t+\n")
    assert t["reads"][0] == FQ1[:FQ1.index(b"@r3")] and t["reads"][1] == FQ2[:FQ2.index(b"@r3/2")]
    assert t["log"] == ["kmer\tAACGG\t3\t5"]


def test_tool_max_reads_per_kmer():
    t = FN.tool(FQ1, ["AACGG", "CCCCC"], max_reads_per_kmer=1)
    # r0 -> AACGG, r1 -> CCCCC (three windows), r2 and r3 are over the limit of their k-mers and only counted
    assert t["tsv"] == b"read\tmate\tn_hits\tfirst_pos\tkmer\tstrand\nr0\t0\t1\t3\tAACGG\t+\nr1\t0\t3\t1\tCCCCC\t+\n"
    assert t["log"] == ["kmer\tAACGG\t1\t3", "kmer\tCCCCC\t1\t5"]
