"""The read-fragments model (tests/read_fragments_model.py) before any GPU is involved, on the case set the GPU tests use:
the cases hold every situation the fragment rule was written for, and a fragment with an absent mate is the SupportModel
record of the other.  The GPU tests then hold kid_db_read_fragments* against this model."""
import numpy as np

import read_fragments_cases as fc
import read_support_cases as sc
from helpers import concat_reads, oracle_db
from read_fragments_model import FragmentModel, fragment_csr
from read_hits_model import HitModel
from read_support_model import SupportModel


def world():
    parent, cum, keys, targets = sc.database()
    odb = oracle_db(parent, keys, targets, 20)
    hm = HitModel(odb, keys, targets, 30)
    sm = SupportModel(hm, parent)
    bases, off, where = fc.fragments(parent, cum, keys, targets)
    return parent, keys, targets, odb, hm, sm, FragmentModel(sm), bases, off, where


def test_the_cases_hold_what_the_rule_was_written_for():
    parent, keys, targets, odb, hm, sm, fm, bases, off, where = world()
    hits = hm.batch(bases, off)
    nf = (off.size - 1) // 2
    per = np.diff(hits.offsets.astype(np.int64))
    p, q = per[0::2], per[1::2]
    exp = {rule: fm.batch(hits, rule) for rule in fc.RULES}
    e0 = exp[(0, 0)]
    # final != msca(final_1, final_2): the hand-built pair, and how it folds
    a = e0[where["8|X_6"]]
    assert (int(a["final"]), int(a["final_1"]), int(a["final_2"])) == (6, 8, 1)
    assert odb.msca(int(a["final_1"]), int(a["final_2"])) == 8
    both = np.flatnonzero((e0["final_1"] > 0) & (e0["final_2"] > 0))
    assert any(int(e0["final"][i]) != odb.msca(int(e0["final_2"][i]), int(e0["final_1"][i])) for i in both)
    # swapping the mates changes final
    b = e0[where["X_6|8"]]
    assert (int(b["final"]), int(b["final_1"]), int(b["final_2"])) == (8, 1, 8) and int(a["final"]) != int(b["final"])
    # p = 0, q = 0, both 0 -- with and without windows
    assert ((p == 0) & (q > 0)).any() and ((p > 0) & (q == 0)).any() and ((p == 0) & (q == 0)).any()
    assert (p[where["6_8|"]], q[where["6_8|"]]) == (2, 0) and (p[where["|6_8"]], q[where["|6_8"]]) == (0, 2)
    assert int(e0[where["|"]]["n_kmers"]) == 0 and int(e0[where["|"]]["final"]) == 0
    # every outcome of the climb
    seen = set()
    for rule, e in exp.items():
        f, c = e["final"].astype(np.int64), e["confident"].astype(np.int64)
        anc = np.array([c[r] > 1 and c[r] != f[r] and sm.under(f[r], c[r]) for r in range(nf)])
        seen |= {name for name, m in (("same", (c == f) & (f > 1)), ("ancestor", anc), ("root", (f > 1) & (c == 1)),
                                      ("none", (f > 0) & (c == 0))) if m.any()}
    assert seen == {"same", "ancestor", "root", "none"}
    e3 = exp[(3, 0)]
    assert (int(e3[where["6_36|8"]]["final"]), int(e3[where["6_36|8"]]["confident"])) == (8, 5)
    assert (int(e3[where["X|8_6"]]["final"]), int(e3[where["X|8_6"]]["confident"])) == (6, 1)
    assert int(exp[(2, 25)][where["36|36"]]["confident"]) == 36  # two mates that agree pass where one alone would not
    assert np.array_equal(e0["confident"], e0["final"])
    # one database k-mer in both mates: two hits of one entry
    ent = np.concatenate([hits.of(2 * where["same_kmer"])[2], hits.of(2 * where["same_kmer"] + 1)[2]])
    assert np.unique(ent).size == ent.size - 1
    # the six fields are the support record of the concatenated hit list, whatever the split: n and m add up
    assert np.array_equal(e0["n_hits"], p + q) and np.array_equal(e0["n_kmers"], fragment_csr(hits).n_kmers)


def test_an_absent_mate_2_leaves_the_support_record_of_mate_1():
    parent, keys, targets, odb, hm, sm, fm, bases, off, where = world()
    raw = bytes(bases)
    mates = [raw[int(off[2 * i]):int(off[2 * i + 1])] for i in range((off.size - 1) // 2)]
    b1, o1 = concat_reads(mates)
    h1 = hm.batch(b1, o1)
    finals = sm.finals(h1)
    b2, o2 = concat_reads([s for m in mates for s in (m, b"")])
    h2 = hm.batch(b2, o2)
    for rule in fc.RULES:
        sup = sm.batch_literal(h1, rule, finals)
        frag = fm.batch(h2, rule)
        for f in sup.dtype.names:
            assert np.array_equal(frag[f], sup[f]), (rule, f)
        assert np.array_equal(frag["final_1"], finals) and not frag["final_2"].any()
