"""The read-votes model (tests/read_votes_model.py) before any GPU is involved: the literal form (root paths by climbing
parent[], Python integers) against the vectorised form (the anc table), on the reads the GPU tests use and on a tree of
depth 12; the worked cases of the rule; the outcome classes the cases must show; and the property the rule exists for:
the record does not depend on the order of a read's hits, while `final` does."""
import numpy as np
import pytest

import read_support_cases as sc
import read_votes_cases as vc
from helpers import concat_reads, oracle_db
from read_hits_model import HitModel, Hits
from read_support_model import RULES, SupportModel
from read_votes_model import VOTE_DTYPE, VoteModel


class Cases:
    def __init__(self):
        self.parent, cum, self.keys, self.targets = sc.database()
        odb = oracle_db(self.parent, self.keys, self.targets, 20)
        self.hm = HitModel(odb, self.keys, self.targets, 30)
        self.sm = SupportModel(self.hm, self.parent)
        self.vm = VoteModel(self.sm)
        self.bases, self.off, self.where, self.x = vc.reads(self.parent, cum, self.keys, self.targets)
        self.hits = self.hm.batch(self.bases, self.off)
        self.finals = self.sm.finals(self.hits)
        self.rec00 = self.vm.batch_anc(self.hits, (0, 0))


@pytest.fixture(scope="module")
def cases():
    return Cases()


def same(a, b, what=""):
    assert a.dtype == VOTE_DTYPE and b.dtype == VOTE_DTYPE and a.shape == b.shape
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, (what, int(bad[0]), a[bad[0]], b[bad[0]])


def test_literal_and_vectorised_forms_agree_under_every_rule(cases):
    calls = cases.vm.calls_anc(cases.hits)
    for rule in RULES:
        same(cases.vm.batch_literal(cases.hits, rule), cases.vm.batch_anc(cases.hits, rule, calls), rule)


def test_the_two_forms_agree_on_a_tree_of_depth_12():
    parent, spine, sibs = sc.chain_taxonomy(12)
    rng = np.random.default_rng(12)
    nodes = spine + sibs
    tg = np.repeat(np.array(nodes, np.uint32), 4)
    keys = sc.random_keys(rng, tg.size)
    hm = HitModel(oracle_db(parent, keys, tg, 12), keys, tg, 30)
    vm = VoteModel(SupportModel(hm, parent))
    seqs = []
    for _ in range(200):
        pick = rng.integers(0, keys.size, int(rng.integers(1, 9)))
        seqs.append(sc.implanted(rng, [sc.cases.key_seq(keys[j], 30) for j in pick]))
    bases, off = concat_reads(seqs)
    hits = hm.batch(bases, off)
    ties = set()
    for rule in RULES:
        lit = vm.batch_literal(hits, rule)
        same(lit, vm.batch_anc(hits, rule), rule)
        ties |= {"unique" if nb == 1 else "root" if c == 1 else "inner" for c, nb in zip(lit["call"], lit["n_best"])}
    assert ties == {"unique", "root", "inner"}


def test_the_worked_cases_give_the_stated_records(cases):
    x, rec, w = cases.x, cases.rec00, cases.where
    field = lambda name, *fs: tuple(int(rec[w[name]][f]) for f in fs)  # noqa: E731
    assert field("6_8", "call", "p_best", "n_best", "n_hits") == (8, 2, 1, 2)
    assert field("X_8_6", "call", "p_best", "n_best") == (8, 2, 1) and int(cases.finals[w["X_8_6"]]) == 6
    assert field("v_8_36", "call", "p_best", "n_best", "s_call") == (5, 1, 2, 2)
    assert field("v_X_8", "call", "p_best", "n_best", "s_call") == (1, 1, 2, 2)
    assert field("v_1_X", "call", "p_best", "n_best", "s_call") == (x, 2, 1, 1)
    assert field("v_8_8_36_36_X", "call", "p_best", "n_best", "n_hits", "s_call") == (5, 2, 2, 5, 4)
    assert int(cases.finals[w["v_8_8_36_36_X"]]) == 1
    assert field("v_6_8_36", "call", "p_best", "n_best") == (8, 2, 1) and int(cases.finals[w["v_6_8_36"]]) == 5
    assert field("root_only", "call", "p_best", "n_best", "s_call") == (1, 3, 1, 3)
    assert cases.hits.of(w["X_8_6"])[1].tolist() == [x, 8, 6] and cases.hits.of(w["v_8_8_36_36_X"])[1].tolist() == [8, 8, 36, 36, x]
    # the climb starts at call: X_8_6 under min_hits 2 is confident at 8's parent 6, under 3 at the root
    r2, r3 = cases.vm.batch_anc(cases.hits, (2, 0))[w["X_8_6"]], cases.vm.batch_anc(cases.hits, (3, 0))[w["X_8_6"]]
    assert (int(r2["confident"]), int(r2["s_confident"]), int(r3["confident"]), int(r3["s_confident"])) == (6, 2, 1, 3)


def test_no_outcome_class_is_missing_from_the_cases(cases):
    rec, fin = cases.rec00, cases.finals
    kind = np.where(rec["n_hits"] == 0, 0, np.where(rec["n_best"] == 1, 1, np.where(rec["call"] != 1, 2, 3)))
    seen = {(("none", "unique", "inner tie", "root tie")[k], bool(c == f)) for k, c, f in zip(kind, rec["call"], fin)}
    assert seen == {("none", True), ("unique", True), ("unique", False), ("inner tie", True), ("inner tie", False), ("root tie", True),
                    ("root tie", False)}
    assert np.all(rec["call"][rec["n_hits"] == 0] == 0) and np.all(rec["call"][rec["n_hits"] > 0] > 0)


def test_under_rule_00_confident_is_call(cases):
    assert np.array_equal(cases.rec00["confident"], cases.rec00["call"])
    assert np.array_equal(cases.rec00["s_confident"], cases.rec00["s_call"])


def test_the_record_does_not_depend_on_the_order_of_the_hits_and_final_does(cases):
    hits = cases.hits
    rev = vc.reversed_hits(hits)
    assert np.array_equal(np.sort(rev.target), np.sort(hits.target)) and not np.array_equal(rev.target, hits.target)
    rng = np.random.default_rng(5)
    idx = np.concatenate([int(hits.offsets[r]) + rng.permutation(int(hits.offsets[r + 1] - hits.offsets[r])) for r in range(hits.offsets.size - 1)])
    shuf = Hits(hits.offsets, hits.n_kmers, hits.pos[idx], hits.target[idx], hits.entry[idx])
    for rule in [(0, 0), (2, 25), (3, 0)]:
        exp = cases.vm.batch_anc(hits, rule)
        same(cases.vm.batch_anc(rev, rule), exp, "reversed")
        same(cases.vm.batch_anc(shuf, rule), exp, "shuffled")
    same(cases.vm.batch_literal(rev, (2, 25)), cases.vm.batch_anc(hits, (2, 25)), "reversed, literal")
    moved = np.flatnonzero(cases.sm.finals(rev) != cases.finals)
    assert moved.size >= 1 and cases.where["X_8_6"] in moved.tolist()


def test_hits_on_one_root_path_are_called_as_final(cases):
    hits, sm = cases.hits, cases.sm
    n_line = 0
    for r in range(hits.offsets.size - 1):
        t = hits.of(r)[1].astype(np.int64)
        if t.size == 0:
            continue
        deepest = int(t[np.argmax(sm.depth[t])])
        if all(sm.under(deepest, int(c)) for c in t):
            n_line += 1
            assert int(cases.rec00[r]["call"]) == int(cases.finals[r]) == deepest, r
    assert n_line > 500
