"""The model of kid_db_read_fragment_loci* (tests/read_fragment_loci_model.py) against the rule's own text: the worked case of
include/kmer_id_amd.h and its three variants field by field, every level of the tie order by a case only that level
decides, and on seeded random fragments (0..9 hits per mate, three orgs, W in {1, 7, 100}, max_span in {0, 50, 500, 5000})
the four statements that follow from the rule: the record is a function of the two multisets; a batch may be split; with one
mate without a participant it is that mate's read_loci record and the pileup's interval; exchanging the mates flips orient
and swaps the _1 / _2 fields when the best score is unique.  No GPU."""
import functools

import numpy as np

import read_fragment_loci_model as fm
import read_loci_model as lm
import read_pileup_model as pm
from read_hits_model import Hits

K = 30
WORKED_ORG, WORKED_POS = [3, 3, 3, 9, 3], [100, 130, 400, 40, 5000]
M1, M2 = [(10, 0), (40, 1), (5, 3)], [(60, 2), (20, 4)]
WORKED = dict(org=3, orient=0, mates=3, n_chain=3, n_chain_1=2, n_chain_2=1, n_org=4, n_other=1, n_hits=5, n_kmers=242, lo=100, hi=429,
              pos_first_1=10, pos_last_1=40, pos_first_2=60, pos_last_2=60)
SWAP = {"n_chain_1": "n_chain_2", "pos_first_1": "pos_first_2", "pos_last_1": "pos_last_2"}
SWAP.update({b: a for a, b in list(SWAP.items())})


def rec(m1, m2, org, pos, w=1, span=1000, nk=242, **kw):
    return fm.record([h[0] for h in m1], [h[1] for h in m1], [h[0] for h in m2], [h[1] for h in m2], nk, org, pos, K, w, span, **kw)


def exchanged(r):
    """the record with the mates exchanged, by the statement: orient flips, mates 1 <-> 2, the _1 / _2 fields swap"""
    out = {SWAP.get(f, f): v for f, v in r.items()}
    if r["mates"]:
        out["orient"] = 1 - r["orient"]
        out["mates"] = {1: 2, 2: 1, 3: 3}[r["mates"]]
    return out


def test_the_record_is_the_library_s():
    from kmer_id_amd import FRAGMENT_LOCUS_DTYPE
    assert FRAGMENT_LOCUS_DTYPE == fm.FRAGMENT_LOCUS_DTYPE and FRAGMENT_LOCUS_DTYPE.itemsize == 64
    assert set(WORKED) == set(fm.FIELDS)


def test_the_worked_case_and_its_variants():
    assert rec(M1, M2, WORKED_ORG, WORKED_POS) == WORKED
    assert rec(M2, M1, WORKED_ORG, WORKED_POS) == exchanged(WORKED)
    assert rec(M1, M2, WORKED_ORG, WORKED_POS, span=370) == WORKED
    solo = dict(WORKED, mates=1, n_chain=2, n_chain_2=0, hi=159, pos_first_2=0, pos_last_2=0)
    assert rec(M1, M2, WORKED_ORG, WORKED_POS, span=369) == solo
    one_each = dict(WORKED, n_chain=2, n_chain_1=1, n_org=2, n_other=0, n_hits=2, pos_last_1=10)
    assert rec(M1[:1], M2[:1], WORKED_ORG, WORKED_POS) == one_each
    for m, read in ((M1[:1], 0), (M2[:1], 1)):  # placed separately, each mate is a chain of one whose strand says nothing
        alone = lm.locus([m[0][0]], [m[0][1]], 121, WORKED_ORG, WORKED_POS)
        assert (alone["n_chain"], alone["strand"]) == (1, 0)
    empty = dict.fromkeys(fm.FIELDS, 0)
    assert rec([], [], WORKED_ORG, WORKED_POS, nk=7) == dict(empty, n_kmers=7)
    assert rec([(3, 5), (4, 99)], [(1, 5)], WORKED_ORG, WORKED_POS, nk=2 ** 32 + 5) == dict(empty, n_hits=3, n_kmers=5)


def test_every_level_of_the_tie_order():
    # sites: entry e of org[e] at pos[e]
    org = [1, 1, 1, 1, 2, 2, 1, 1]
    pos = [1000, 1400, 3000, 3400, 1000, 1400, 1010, 1390]
    # score first: a solo of 2 beats a pair of ... nothing else: mate 1 has two hits on D = 1000 (entries 0 and 0 at r = 0: the same hit twice)
    r = rec([(0, 0), (0, 0), (5, 2)], [], org, pos)
    assert (r["mates"], r["n_chain"], r["lo"]) == (1, 2, 1000)
    # a paired placement before a solo one of the same score: the solo of two on D = 3000 against the pair (D 1000, E 1400)
    r = rec([(0, 2), (0, 2), (0, 0)], [(0, 1)], org, pos)
    assert (r["mates"], r["n_chain"], r["n_chain_1"], r["lo"], r["hi"]) == (3, 2, 1, 1000, 1429)
    # paired: o = 0 before o = 1.  Mate 1 (0, e0) and mate 2 (0, e1): o = 0 is (D 1000, E 1400); exchanged, the same two hits
    # pair as o = 1 only -- and with both orientations on offer (each mate has both entries) o = 0 wins
    r = rec([(0, 0), (0, 1)], [(0, 0), (0, 1)], org, pos)
    assert (r["mates"], r["orient"], r["n_chain"]) == (3, 0, 2)
    # paired: the lowest g.  The same pair on org 1 and on org 2
    r = rec([(0, 0), (0, 4)], [(0, 1), (0, 5)], org, pos)
    assert (r["mates"], r["org"], r["n_other"], r["n_chain"]) == (3, 1, 2, 2)
    # paired: the lowest D, then the lowest E: forward keys 1000 and 1010, reverse keys 1390 and 1400, all four pairs allowed
    r = rec([(0, 6), (0, 0)], [(0, 1), (0, 7)], org, pos)
    assert (r["mates"], r["lo"], r["hi"]) == (3, 1000, 1419)  # (D 1000, E 1390)
    r = rec([(0, 6)], [(0, 1), (0, 7)], org, pos)
    assert (r["mates"], r["lo"], r["hi"]) == (3, 1010, 1419)  # D 1010 alone: E 1390 before E 1400
    # solo: t = 0 before t = 1 (one hit: its forward key wins, as in read_loci)
    r = rec([(7, 0)], [], org, pos, span=0)
    assert (r["mates"], r["orient"], r["lo"], r["hi"]) == (1, 0, 1000, 1029)
    r = rec([], [(7, 0)], org, pos, span=0)
    assert (r["mates"], r["orient"]) == (2, 1)  # mate 2 forward: mate 1 would read reverse
    # solo: the lowest g, then the lowest d, then mate 1 before mate 2 (max_span = 0 and r > 0: no pair of these is allowed)
    r = rec([(5, 4)], [(5, 0)], org, pos, span=0)
    assert (r["mates"], r["org"], r["n_other"]) == (2, 1, 1)
    r = rec([(5, 1)], [(5, 0)], org, pos, span=0)
    assert (r["mates"], r["lo"]) == (2, 1000)
    r = rec([(5, 0)], [(5, 0)], org, pos, span=0)
    assert (r["mates"], r["orient"], r["n_chain"]) == (1, 0, 1)


# ---------------------------------------------------------------- seeded random fragments
N_ORGS, GRID, GENOME = 3, 10, 3000
PER_ORG = GENOME // GRID
WIDTHS, SPANS = (1, 7, 100), (0, 50, 500, 5000)
N_RANDOM = 4000


@functools.lru_cache(maxsize=None)
def world():
    """three orgs with an entry every 10 bases (entry = g * 300 + x / 10), and N_RANDOM fragments: half of them uniform hits,
    half a fragment cut from an org (mate 1 forward or reverse, an insert of 100..700) with noise, a quarter with a mate absent"""
    org = [g for g in range(N_ORGS) for _ in range(PER_ORG)]
    pos = [GRID * i for _ in range(N_ORGS) for i in range(PER_ORG)]
    rng = np.random.default_rng(20)
    ent = lambda g, x: g * PER_ORG + x // GRID  # noqa: E731
    noise = lambda n: [(int(rng.integers(0, 121)), int(rng.integers(0, len(org)))) for _ in range(n)]  # noqa: E731
    out = []
    for i in range(N_RANDOM):
        n1, n2 = int(rng.integers(0, 10)), int(rng.integers(0, 10))
        if rng.integers(0, 4) == 0:
            n1, n2 = (0, n2) if rng.integers(0, 2) else (n1, 0)
        if i % 2:
            m1, m2 = noise(n1), noise(n2)
        else:
            g, start, insert = int(rng.integers(0, N_ORGS)), GRID * int(rng.integers(0, 200)), K + GRID * int(rng.integers(7, 68))
            good1, good2 = int(rng.integers((n1 + 1) // 2, n1 + 1)), int(rng.integers((n2 + 1) // 2, n2 + 1))  # (at least half of a mate's hits)
            fwd = [(r, ent(g, start + r)) for r in (GRID * int(v) for v in rng.integers(0, 10, good1))]
            rev = [(r, ent(g, start + insert - K - r)) for r in (GRID * int(v) for v in rng.integers(0, 10, good2))]
            m1, m2 = fwd + noise(n1 - good1), rev + noise(n2 - good2)
            if rng.integers(0, 2):
                m1, m2 = m2, m1
                m1, m2 = m1[:n1] + noise(max(0, n1 - len(m1))), m2[:n2] + noise(max(0, n2 - len(m2)))
        p1, p2 = rng.permutation(len(m1)), rng.permutation(len(m2))
        out.append(([m1[j] for j in p1], [m2[j] for j in p2], int(rng.integers(0, 300)),
                    WIDTHS[int(rng.integers(0, 3))], SPANS[int(rng.integers(0, 4))]))
    return org, pos, out


@functools.lru_cache(maxsize=None)
def records():
    org, pos, frags = world()
    return [rec(m1, m2, org, pos, w, s, nk, want_unique=True) for m1, m2, nk, w, s in frags]


def test_the_generator_yields_paired_and_solo_bests():
    mates = np.array([r["mates"] for r, u in records()])
    paired, solo = int((mates == 3).sum()), int(((mates == 1) | (mates == 2)).sum())
    print("paired %d, solo %d, none %d of %d" % (paired, solo, int((mates == 0).sum()), mates.size))
    assert 4 * paired >= N_RANDOM and 4 * solo >= N_RANDOM
    assert {0, 1} == {r["orient"] for r, u in records() if r["mates"] == 3}


def test_a_function_of_the_two_multisets():
    org, pos, frags = world()
    rng = np.random.default_rng(21)
    for (m1, m2, nk, w, s), (r, u) in zip(frags, records()):
        p1, p2 = rng.permutation(len(m1)), rng.permutation(len(m2))
        assert rec([m1[j] for j in p1], [m2[j] for j in p2], org, pos, w, s, nk) == r
        assert r["n_chain"] == r["n_chain_1"] + r["n_chain_2"] and r["n_hits"] == len(m1) + len(m2) and r["n_kmers"] == nk


def test_a_batch_may_be_split_and_run_again():
    org, pos, frags = world()
    w, s = 7, 500
    some = frags[:300]
    ms = np.array([len(m) for m1, m2, *_ in some for m in (m1, m2)], np.int64)
    off = np.zeros(ms.size + 1, np.uint64)
    off[1:] = np.cumsum(ms)
    hp = np.array([h[0] for m1, m2, *_ in some for m in (m1, m2) for h in m], np.uint32)
    he = np.array([h[1] for m1, m2, *_ in some for m in (m1, m2) for h in m], np.uint32)
    nk = np.array([v for m1, m2, n, *_ in some for v in (n // 2, n - n // 2)], np.uint32)
    whole = fm.batch(Hits(off, nk, hp, np.ones_like(hp), he), org, pos, K, w, s)
    assert fm.batch(Hits(off, nk, hp, np.ones_like(hp), he), org, pos, K, w, s).tobytes() == whole.tobytes()
    parts = []
    for a, b in ((0, 14), (14, 400), (400, 600)):  # cuts at even read indexes; offsets stay absolute
        parts.append(fm.batch(Hits(off[a:b + 1], nk[a:b], hp, np.ones_like(hp), he), org, pos, K, w, s))
    assert np.concatenate(parts).tobytes() == whole.tobytes()
    for i in (0, 7, 150, 299):
        m1, m2, n, _, _ = some[i]
        assert tuple(whole[i]) == tuple(rec(m1, m2, org, pos, w, s, n)[f] for f in fm.FIELDS)


def test_with_one_mate_absent_it_is_read_loci_and_the_pileup_s_interval():
    org, pos, frags = world()
    n = 0
    for m1, m2, nk, w, s in frags:
        for solo, which in ((m1, 1), (m2, 2)):
            other = [(3, len(org) + 5)] if nk % 2 else []  # (a mate without a participant: no hit, or a hit outside the database)
            r = rec(solo, other, org, pos, w, s, nk) if which == 1 else rec(other, solo, org, pos, w, s, nk)
            L = lm.locus([h[0] for h in solo], [h[1] for h in solo], nk, org, pos, w)
            strand = r["orient"] if which == 1 else 1 - r["orient"]
            if not L["n_chain"]:
                assert r["mates"] == 0 and r["n_chain"] == 0
                continue
            got = (r["org"], strand, r["n_chain"], r["n_org"], r["n_other"], r["pos_first_%d" % which], r["pos_last_%d" % which])
            assert got == (L["org"], L["strand"], L["n_chain"], L["n_org"], L["n_other"], L["pos_first"], L["pos_last"])
            assert (r["lo"], r["hi"]) == pm.interval(L, pos, K) and r["mates"] == which and r["n_chain_%d" % (3 - which)] == 0
            n += 1
    assert n > N_RANDOM


def test_exchanging_the_mates_when_the_best_score_is_unique():
    org, pos, frags = world()
    paired = unique_paired = 0
    for (m1, m2, nk, w, s), (r, unique) in zip(frags, records()):
        paired += r["mates"] == 3
        if not unique:
            continue
        unique_paired += r["mates"] == 3
        assert rec(m2, m1, org, pos, w, s, nk) == exchanged(r)
    print("paired %d, of them with a unique best score %d" % (paired, unique_paired))
    assert 2 * unique_paired >= paired
