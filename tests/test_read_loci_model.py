"""tests/read_loci_model.py held to hand-written cases of the rule (the worked cases of the README's `read_loci` section
among them) and to what follows from the rule on the genome world of tests/read_loci_cases.py.  No GPU."""
import numpy as np
import pytest

import read_loci_cases as lc
import read_loci_model as lm

# the README's site table: entry -> (org, pos)
ORG = [3, 3, 3, 3, 9, 9]
POS = [100, 101, 102, 250, 40, 41]


def rec(**kw):
    d = dict.fromkeys(lm.FIELDS, 0)
    d.update(kw)
    return d


def test_the_readme_forward_case():
    got = lm.locus([10, 11, 12, 40, 60, 61], [0, 1, 2, 3, 4, 5], 121, ORG, POS)
    assert got == rec(org=3, strand=0, n_chain=3, n_org=4, n_other=2, n_hits=6, n_kmers=121, pos_first=10, pos_last=12, entry_first=0)
    assert POS[got["entry_first"]] - got["pos_first"] == 90
    assert lm.line(got, POS) == "3:0:3:4:2:10:12:100"


def test_the_readme_reverse_case():
    got = lm.locus([110, 109, 108, 80, 60, 59], [0, 1, 2, 3, 4, 5], 121, ORG, POS)
    assert got == rec(org=3, strand=1, n_chain=3, n_org=4, n_other=2, n_hits=6, n_kmers=121, pos_first=108, pos_last=110, entry_first=2)
    assert POS[got["entry_first"]] + got["pos_first"] == 90 + 150 - 30


def test_no_hit_and_one_hit():
    assert lm.locus([], [], 7, ORG, POS) == rec(n_kmers=7)
    assert lm.locus([5], [4], 1, ORG, POS) == rec(org=9, strand=0, n_chain=1, n_org=1, n_hits=1, n_kmers=1, pos_first=5, pos_last=5, entry_first=4)


def test_a_negative_forward_diagonal_floors_toward_minus_infinity():
    # x - r = 40 - 61 = -21 and 41 - 62 = -21: one diagonal at W = 1; at W = 4 floor(-21 / 4) = -6 (truncation gives -5)
    for w in (1, 4):
        got = lm.locus([61, 62, 1], [4, 5, 4], 3, ORG, POS, w)
        assert (got["strand"], got["n_chain"], got["pos_first"], got["pos_last"]) == (0, 2, 61, 62), w
    # entry 4 at r = 61: -21; entry 3 (x = 250) at r = 271: -21 as well, at r = 270: -20.  At W = 4 the bin -6 is [-24, -21]
    # and -20 opens the bin -5 (the reverse keys, 101 against 521 and 520, are far apart)
    org, pos = [9, 9, 9, 9, 9, 9], POS
    got = lm.locus([61, 271], [4, 3], 2, org, pos, 4)
    assert (got["strand"], got["n_chain"]) == (0, 2)
    assert lm.locus([61, 270], [4, 3], 2, org, pos, 4)["n_chain"] == 1
    # -1 and 1 (entry 4 at r = 41, entry 3 at r = 249): bins -1 and 0; truncation toward zero would put both into 0
    assert lm.locus([41, 249], [4, 3], 2, org, pos, 4)["n_chain"] == 1


def test_a_chain_that_straddles_a_bin_edge_at_width_7():
    # diagonals 90 (x3) and 91 (x2): 90 // 7 = 12, 91 // 7 = 13 -- at W = 7 the five hits fall into two bins, 3 against 2;
    # diagonals 84 .. 90 would be one bin
    pos, entry = [10, 11, 12, 9, 10], [0, 1, 2, 0, 1]
    assert lm.locus(pos, entry, 5, ORG, POS, 1)["n_chain"] == 3
    got = lm.locus(pos, entry, 5, ORG, POS, 7)
    assert (got["n_chain"], got["pos_first"], got["pos_last"], got["entry_first"]) == (3, 10, 12, 0)
    got = lm.locus([10, 11, 12, 15, 16], [0, 1, 2, 0, 1], 5, ORG, POS, 7)  # diagonals 90 x3, 85 x2: one bin
    assert (got["n_chain"], got["pos_first"], got["pos_last"], got["entry_first"]) == (5, 10, 16, 0)


def test_every_tie_order():
    # strand 0 before strand 1: two hits that share both their forward and their reverse key cannot exist with distinct
    # (pos, entry), so: forward pair (90, 90) against reverse pair (x + r = 300) of the same org
    got = lm.locus([10, 11, 200, 50], [0, 1, 0, 3], 4, ORG, POS)
    assert (got["strand"], got["n_chain"], got["pos_first"]) == (0, 2, 10)
    got = lm.locus([200, 50, 10, 11], [0, 3, 0, 1], 4, ORG, POS)  # ... in whatever order they come
    assert (got["strand"], got["n_chain"], got["pos_first"]) == (0, 2, 10)
    # the lowest org: org 9's pair stands first in the list, org 3 wins; n_other is the loser's count
    got = lm.locus([60, 61, 10, 11], [4, 5, 0, 1], 4, ORG, POS)
    assert (got["org"], got["n_chain"], got["n_other"], got["n_org"]) == (3, 2, 2, 2)
    # the lowest diagonal: entry 3 at r = 42 twice (208 forward, 292 reverse, each x2) in front of the pair on 90
    got = lm.locus([42, 42, 10, 11], [3, 3, 0, 1], 4, ORG, POS)
    assert (got["strand"], got["n_chain"], got["pos_first"], got["entry_first"]) == (0, 2, 10, 0)
    got = lm.locus([42, 10], [3, 0], 2, ORG, POS)  # all counts 1: strand 0, the lowest diagonal 90
    assert (got["strand"], got["n_chain"], got["pos_first"], got["entry_first"]) == (0, 1, 10, 0)
    got = lm.locus([0, 160], [3, 0], 2, ORG, POS)  # diagonals 250 and -60: the negative one is the lowest
    assert (got["n_chain"], got["pos_first"], got["entry_first"]) == (1, 160, 0)


def test_two_hits_at_one_pos_take_the_lowest_entry():
    org, pos = [3, 3, 3], [100, 100, 101]  # entries 0 and 1 lie at one site (a synthetic list alone has this)
    got = lm.locus([10, 10, 11], [1, 0, 2], 3, org, pos)
    assert (got["n_chain"], got["pos_first"], got["pos_last"], got["entry_first"]) == (3, 10, 11, 0)


def test_an_entry_out_of_range_counts_in_n_hits_alone():
    got = lm.locus([10, 11, 11, 13], [0, 6, 1, 2 ** 32 - 1], 9, ORG, POS)
    assert got == rec(org=3, strand=0, n_chain=2, n_org=2, n_hits=4, n_kmers=9, pos_first=10, pos_last=11, entry_first=0)
    assert lm.locus([1, 2], [6, 7], 2, ORG, POS) == rec(n_hits=2, n_kmers=2)


def test_the_4097th_hit_takes_no_part():
    # 2048 hits on diagonal -20 of org 9 and 2048 on 90 of org 3, alternating, org 3's last: the tie goes to org 3; one
    # more hit on org 9's diagonal would make that the best key
    pos = [60, 10] * 2048
    entry = [4, 0] * 2048
    tie = lm.locus(pos, entry, 0, ORG, POS)
    assert (tie["org"], tie["n_chain"], tie["n_other"], tie["n_hits"]) == (3, 2048, 2048, 4096)
    got = lm.locus(pos + [60], entry + [4], 0, ORG, POS)
    assert {f: got[f] for f in lm.FIELDS if f != "n_hits"} == {f: tie[f] for f in lm.FIELDS if f != "n_hits"} and got["n_hits"] == 4097
    first = lm.locus([60] + pos, [4] + entry, 0, ORG, POS)  # the same hit in front does count, and the last of the list drops out
    assert (first["org"], first["n_chain"], first["n_other"], first["n_hits"]) == (9, 2049, 2047, 4097)


def test_the_largest_site_and_the_largest_read_position():
    org, pos = [2 ** 24 - 1, 2 ** 24 - 1], [2 ** 31 - 1, 2 ** 31 - 2]
    got = lm.locus([2 ** 32 - 1, 2 ** 32 - 2], [0, 1], 2, org, pos)  # x - r = -2^31 twice; x + r = 2^31 + 2^32 - 2 and - 4
    assert got == rec(org=2 ** 24 - 1, strand=0, n_chain=2, n_org=2, n_hits=2, n_kmers=2, pos_first=2 ** 32 - 2, pos_last=2 ** 32 - 1, entry_first=1)
    got = lm.locus([2 ** 32 - 1, 2 ** 32 - 2], [1, 0], 2, org, pos, 2 ** 31 - 1)  # x + r = 2^31 + 2^32 - 3 twice
    # (x - r = -2^31 - 1 and -2^31 + 1: floor(. / (2^31 - 1)) = -2 and -1, two bins; the reverse key wins)
    assert (got["strand"], got["n_chain"], got["pos_first"], got["entry_first"]) == (1, 2, 2 ** 32 - 2, 0)
    assert lm.as_records([got]).dtype.itemsize == 40


# ------------------------------------------------------------------ what follows from the rule, on the genome world
@pytest.fixture(scope="module", params=[1, 7])
def placed(request):
    w = lc.world(request.param)
    hits = w.hm.batch(w.bases, w.off)
    return w, hits, lm.batch(hits, w.org, w.pos, 1)


def test_the_genomes_hold_no_repeated_kmer_and_reads_hit_their_own_windows(placed):
    w, hits, recs = placed
    for i, (kind, seq, what) in enumerate(w.reads):
        if kind in ("forward", "reverse"):
            assert int(recs["n_hits"][i]) == w.own_windows(*what).size, (i, kind)


def test_forward_reads_lie_on_strand_0_at_their_offset(placed):
    w, hits, recs = placed
    seen = 0
    for i, (kind, seq, what) in enumerate(w.reads):
        if kind != "forward" or recs["n_hits"][i] == 0:
            continue
        gi, a, n = what
        r = recs[i]
        assert (int(r["org"]), int(r["strand"]), int(r["n_chain"]), int(r["n_org"]), int(r["n_other"])) == (gi, 0, int(r["n_hits"]), int(r["n_hits"]), 0)
        assert int(w.pos[r["entry_first"]]) - int(r["pos_first"]) == a
        seen += 1
    assert seen >= 30


def test_reverse_complements_lie_on_strand_1_with_the_same_chain(placed):
    w, hits, recs = placed
    by_what = {(kind, what): i for i, (kind, seq, what) in enumerate(w.reads)}
    seen = 0
    for (kind, what), i in by_what.items():
        if kind != "reverse" or recs["n_hits"][i] < 2:
            continue
        gi, a, n = what
        r = recs[i]
        assert (int(r["org"]), int(r["strand"]), int(r["n_chain"])) == (gi, 1, int(r["n_hits"]))
        assert int(w.pos[r["entry_first"]]) + int(r["pos_first"]) == a + n - lc.K
        if ("forward", what) in by_what:
            assert int(recs["n_chain"][by_what["forward", what]]) == int(r["n_chain"])
        seen += 1
    assert seen >= 30


def common_prefix(x, y):
    n = 0
    while n < min(len(x), len(y)) and x[n] == y[n]:
        n += 1
    return n


def test_a_chimera_shows_both_chains(placed):
    w, hits, recs = placed
    for i, (kind, seq, what) in enumerate(w.reads):
        if kind != "chimera":
            continue
        (ga, a, na), (gb, b, nb) = what
        # a window across the junction is a window of genome A when B's stretch happens to go on as A does (and the other
        # way round in front of B's stretch): it lengthens that chain
        ext_a = common_prefix(w.genomes[ga][a + na:a + na + lc.K - 1], w.genomes[gb][b:b + nb])
        ext_b = common_prefix(w.genomes[gb][max(b - lc.K + 1, 0):b][::-1], w.genomes[ga][a:a + na][::-1])
        ca, cb = w.own_windows(ga, a, na + ext_a).size, w.own_windows(gb, b - ext_b, nb + ext_b).size
        r = recs[i]
        assert int(r["n_hits"]) == ca + cb and {int(r["n_chain"]), int(r["n_other"])} == {ca, cb} and int(r["n_org"]) == int(r["n_chain"])
        if ca != cb:
            assert int(r["org"]) == (ga if ca > cb else gb)


def test_the_record_does_not_depend_on_the_order_of_the_hits():
    c = lc.case()
    plain, shuffled = c.expected("hits", 7), c.expected("shuffled", 7)
    small = np.array([m <= lm.MAX_HITS for m, s in c.what])
    assert plain[small].tobytes() == shuffled[small].tobytes() and small.sum() == len(c.what) - 2 * len(lc.SHAPES)
    assert plain[~small].tobytes() != shuffled[~small].tobytes()  # ... beyond that it is the first 4096 of the list
    assert len({(int(r["n_chain"]), int(r["n_other"])) for r in plain}) > 30
