"""locate_np, the brute-force model of locate_kmers, against cases worked out by hand: what a hit is, which strands a query has,
where the offset, ref and alt of a mismatch come from, and what contigs, N runs and lower case do."""
import numpy as np
import pytest

import locate_np as LN


def records(stream, queries, d):
    rec, windows = LN.locate(stream.encode(), queries, d)
    return [(int(r["pos"]), int(r["kmer"]), "+-"[r["strand"]], int(r["mismatches"]), int(r["offset"])) for r in rec], windows


def test_exact_hits_on_both_strands():
    #         0123456789
    stream = "TTACGGATCC"
    got, windows = records(stream, ["ACGGA", "GATCC"], 0)
    assert windows == 6
    # GGATC at 4 is the reverse complement of GATCC; GATCC itself sits at 5
    assert got == [(2, 0, "+", 0, 0), (4, 1, "-", 0, 0), (5, 1, "+", 0, 0)]


def test_a_palindrome_has_only_plus():
    assert LN.revcomp("ACGT") == "ACGT" and LN.patterns_of(["ACGT", "AAAA"]) == [("ACGT", 0, 0), ("AAAA", 1, 0), ("TTTT", 1, 1)]
    got, _ = records("GGACGTGG", ["ACGT"], 0)
    assert got == [(2, 0, "+", 0, 0)]
    got, _ = records("GGACGAGG", ["ACGT"], 1)
    # ACGA differs from ACGT at base 4; CGAG and GACG differ in more than one base; no - record exists
    assert got == [(2, 0, "+", 1, 4)]


def test_a_window_that_hits_both_strands_of_one_query():
    # query AAT, reverse complement ATT: the window AAT... at d = 1 the window ATT hits + (AAT, base 2) and - (ATT, exact)
    got, _ = records("CCATTCC", ["AAT"], 1)
    assert (2, 0, "+", 1, 2) in got and (2, 0, "-", 0, 0) in got
    assert got.index((2, 0, "+", 1, 2)) + 1 == got.index((2, 0, "-", 0, 0))  # + before - at one position
    # the window AAT of another stream: + exact and - with one mismatch
    got, _ = records("CCAATCC", ["AAT"], 1)
    assert (2, 0, "+", 0, 0) in got and (2, 0, "-", 1, 2) in got


def test_the_offset_counts_in_the_window_as_the_reference_spells_it():
    # the query's reverse complement GTTCA sits at 3 with its base 2 changed (T -> G): strand -, offset 2
    got, _ = records("AAAGGTCAAAA", ["TGAAC"], 1)
    assert (3, 0, "-", 1, 2) in got
    out, log, counts, _ = LN.run(b">c\nAAAGGTCAAAA\n", "TGAAC\n", 5, 1)
    lines = out.decode().split("\n")
    assert lines[0] == "kmer\tcontig\tpos\tstrand\tmismatches\toffset\tref\talt"
    # ref is the reference's G; alt the k-mer's base there in the reference's orientation: the complement of TGAAC[5 - 2] = A -> T
    assert "TGAAC\tc\t4\t-\t1\t2\tG\tT" in lines
    # the same locus with the query spelled as the reference's strand
    out, _, _, _ = LN.run(b">c\nAAAGGTCAAAA\n", "GTTCA\n", 5, 1)
    assert "GTTCA\tc\t4\t+\t1\t2\tG\tT" in out.decode().split("\n")


def test_several_queries_at_one_window_come_in_query_order():
    got, _ = records("ACGTA", ["ACGTC", "ACGTA", "CCGTA"], 1)
    assert got == [(0, 0, "+", 1, 5), (0, 1, "+", 0, 0), (0, 2, "+", 1, 1)]


def test_separators_n_runs_and_lower_case():
    got, windows = records("acgNNacgt\nACG", ["ACG"], 0)
    # ACG at 0 (lower case), at 5, at 10; CGT at 6 is its reverse complement; no window spans N or the newline
    assert got == [(0, 0, "+", 0, 0), (5, 0, "+", 0, 0), (6, 0, "-", 0, 0), (10, 0, "+", 0, 0)]
    assert windows == 1 + 2 + 1
    assert records("AC", ["ACG"], 1) == ([], 0)


def test_fasta_rules():
    data = b">one first contig\r\nACGT\r\nAC\n>two\tx\nNNNN\n>three\n\n>four\nacgtn"
    assert LN.read_fasta(data) == [("one", b"ACGTAC"), ("two", b"NNNN"), ("three", b""), ("four", b"acgtn")]
    for bad, msg in ((b"", "not FASTA"), (b"ACGT\n", "not FASTA"), (b">a\n>b\n", "no sequence"), (b">a\nAC\n> x\nAC\n", "line 3: a contig without a name"),
                     (b">a\nAC\n>b\nAC\n>a 2\nAC\n", "line 5: the contig 'a' is given twice")):
        with pytest.raises(LN.Refused, match=msg):
            LN.read_fasta(bad)


def test_contig_boundaries_and_positions():
    fasta = b">c1\nAAACG\n>c2\nTTACG\nTTT\n>short\nAC\n>n\nNNNNNN\n"
    out, log, counts, windows = LN.run(fasta, "ACGTT\nAAACG\n", 5, 1)
    lines = out.decode().split("\n")[1:-1]
    # ACGTT: in c2 ACGTT at 3 (the lines of a contig are one sequence); CGTTT... its reverse complement AACGT hits AAACG of c1 with one mismatch? no:
    # AACGT vs AAACG differ in 3 bases. No window spans c1 | c2.
    assert "ACGTT\tc2\t3\t+\t0\t0\t.\t." in lines
    assert all(l.split("\t")[1] in ("c1", "c2") for l in lines)
    assert "AAACG\tc1\t1\t+\t0\t0\t.\t." in lines
    assert windows == 1 + 4 and log.decode().startswith("kmer\tACGTT\t")
    assert [c for c in counts if c[0] != c[1]] == []


def test_kmers_file_formats_and_max_per_kmer():
    assoc = "chr\trs\tps\tn_miss\tallele1\tallele0\taf\tl_mle\tp_lrt\n0\tACG\t0\t0\t0\t1\t0.3\t1.0\t1e-9\n0\tTTT\t0\t0\t0\t1\t0.3\t1.0\t2e-5\n"
    assert LN.read_kmers(assoc, 3) == ([("ACG", "1e-9"), ("TTT", "2e-5")], True)
    proxies = "lead\tkmer\tr2\tphase\tn1\tn11\trow\nACG\tTTT\t1.0\t+\t3\t3\t0\nACG\tAAA\t1.0\t+\t3\t3\t1\nCCC\tTTT\t1.0\t+\t3\t3\t0\n"
    assert LN.read_kmers(proxies, 3) == ([("TTT", None)], False)  # AAA is TTT's reverse complement: the same k-mer
    assert LN.read_kmers("ACG\n\nTTT\r\nCCC", 3) == ([("ACG", None), ("TTT", None), ("CCC", None)], False)
    for bad, msg in (("ACG\nCGT\n", "line 2: duplicate k-mer 'CGT' .the k-mer of line 1."), ("ACGT\n", "has length 4, not 3"), ("ACN\n", "a letter other than"),
                     ("ACG 1\n", "2 fields: a list of k-mers"), ("\n", "no k-mer"), (assoc + "0\tACC\n", "line 4: too few fields .2, the header has 9.")):
        with pytest.raises(LN.Refused, match=msg):
            LN.read_kmers(bad, 3)
    out, log, counts, _ = LN.run(b">c\n" + b"ACGA" * 5 + b"\n", assoc, 3, 0, max_per_kmer=2)
    assert counts == [(2, 5), (0, 0)] and log == b"kmer\tACG\t2\t5\nkmer\tTTT\t0\t0\n"
    assert out == b"kmer\tcontig\tpos\tstrand\tmismatches\toffset\tref\talt\tp_lrt\nACG\tc\t1\t+\t0\t0\t.\t.\t1e-9\nACG\tc\t5\t+\t0\t0\t.\t.\t1e-9\n"


def test_against_a_letter_loop():
    """the matrix product counts equal letters: the same records as two nested loops over windows and patterns"""
    rng = np.random.default_rng(5)
    for k, d in ((2, 1), (3, 1), (5, 0), (8, 1)):
        stream = "".join(rng.choice(list("ACGTacgtN\n"), 300, p=[0.2] * 4 + [0.04] * 4 + [0.02, 0.02]))
        words = sorted({LN.canonical("".join(rng.choice(list("ACGT"), k))) for _ in range(12)})
        want = []
        for p in range(len(stream) - k + 1):
            w = stream[p:p + k].upper()
            if set(w) - set("ACGT"):
                continue
            for text, i, s in LN.patterns_of(words):
                diff = [j for j in range(k) if w[j] != text[j]]
                if len(diff) <= d:
                    want.append((p, i, "+-"[s], len(diff), diff[0] + 1 if diff else 0))
        got, _ = records(stream, words, d)
        assert got == sorted(want) and len(got) > 0
