"""The read-support model (tests/read_support_model.py) before any GPU is involved: the literal form (S(c) by climbing
parent[] from every hit) against the vectorised form (the d_i identity the kernel uses), on the reads the GPU tests use
and on a tree of depth 12; and under the rule (0, 0) the model's tally against OracleSample.classify + counts().  The GPU
tests then hold kid_db_read_support* against this model."""
import numpy as np

import read_support_cases as sc
from helpers import concat_reads, ob, oracle_db
from read_hits_model import HitModel
from read_support_model import RULES, SupportModel


def test_literal_and_identity_forms_agree_and_the_rule_00_tally_is_the_oracles():
    parent, cum, keys, targets = sc.database()
    odb = oracle_db(parent, keys, targets, 20)
    hm = HitModel(odb, keys, targets, 30)
    model = SupportModel(hm, parent)
    bases, off, where = sc.reads(parent, cum, keys, targets)
    hits = hm.batch(bases, off)
    finals = model.finals(hits)
    smp = ob.OracleSample(odb)
    assert np.array_equal(smp.classify(bases, off), finals)
    for rule in RULES:
        lit = model.batch_literal(hits, rule, finals)
        ident = model.batch_identity(hits, rule, finals)
        bad = np.flatnonzero(lit != ident)
        assert bad.size == 0, (rule, int(bad[0]), lit[bad[0]], ident[bad[0]])
        if rule == (0, 0):
            assert np.array_equal(lit["confident"], finals)
            g, u = model.tally(hits, lit, np.ones(finals.size, bool), targets)
            og, ou = smp.counts()
            assert np.array_equal(g, og) and np.array_equal(u, ou)
            assert int(g[0]) > 100 and int(u.sum()) > 1000
    # the hand-built reads do what they were built for
    r3 = model.batch_literal(hits, (3, 0), finals)
    a, b, c = r3[where["6_36_8"]], r3[where["X_8_6"]], r3[where["root_only"]]
    assert (int(a["final"]), int(a["confident"]), int(a["s_final"]), int(a["s_confident"])) == (8, 5, 1, 3)
    assert (int(b["final"]), int(b["confident"]), int(b["s_final"]), int(b["s_confident"])) == (6, 1, 2, 3)
    assert (int(c["final"]), int(c["confident"]), int(c["n_hits"])) == (1, 1, 3)
    e = model.batch_literal(hits, (2, 0), finals)[where["6_8"]]
    assert (int(e["final"]), int(e["confident"]), int(e["s_final"]), int(e["s_confident"])) == (8, 6, 1, 2)


def test_a_tree_of_depth_12():
    parent, spine, sibs = sc.chain_taxonomy(12)
    rng = np.random.default_rng(12)
    nodes = spine + sibs
    tg = np.repeat(np.array(nodes, np.uint32), 4)
    keys = sc.random_keys(rng, tg.size)
    odb = oracle_db(parent, keys, tg, 12)
    hm = HitModel(odb, keys, tg, 30)
    model = SupportModel(hm, parent)
    assert int(model.depth.max()) == 12
    seqs = []
    for _ in range(200):
        pick = rng.integers(0, keys.size, int(rng.integers(1, 7)))
        seqs.append(sc.implanted(rng, [sc.cases.key_seq(keys[j], 30) for j in pick]))
    bases, off = concat_reads(seqs)
    hits = hm.batch(bases, off)
    finals = model.finals(hits)
    assert np.array_equal(ob.OracleSample(odb).classify(bases, off), finals)
    outcomes = set()
    for rule in RULES:
        lit = model.batch_literal(hits, rule, finals)
        assert np.array_equal(lit, model.batch_identity(hits, rule, finals)), rule
        outcomes |= {"same" if c == f else "up" if c > 1 else "root" if c == 1 else "none" for f, c in zip(lit["final"], lit["confident"])}
    assert outcomes == {"same", "up", "root", "none"}
