"""The fragment-votes model (tests/read_fragment_votes_model.py) before any GPU is involved: the literal form (Python
lists, root paths by climbing parent[]) against the vectorised form on every tree and list of tests/hit_list_cases.py
(reads 2i and 2i + 1 are the mates of fragment i; n_1 + n_2 wraps there); the worked cases of the rule on the tree
5 -> 6 -> 8, 5 -> 35 -> 36; and the identities the rule promises: a permutation inside a mate changes nothing, an exchange
of the mates exchanges call_1 and call_2 alone, a fragment without mate 2 is mate 1's vote record."""
import numpy as np
import pytest

import hit_list_cases as hc
import read_support_cases as sc
import read_votes_cases as vc
from helpers import oracle_db
from read_fragment_votes_model import FRAGMENT_VOTE_DTYPE, FragmentVoteModel, exchanged, exchanged_records
from read_fragments_model import fragment_csr
from read_hits_model import HitModel, Hits
from read_support_model import SupportModel
from read_votes_model import VoteModel


def same(a, b, what=""):
    assert a.dtype == FRAGMENT_VOTE_DTYPE and b.dtype == FRAGMENT_VOTE_DTYPE and a.shape == b.shape
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, (what, int(bad[0]), a[bad[0]], b[bad[0]])


@pytest.mark.parametrize("name", sorted(hc.TREES))
def test_literal_and_vectorised_forms_agree_on_the_hit_lists(name):
    c = hc.case(name)
    fvm = FragmentVoteModel(c.models.vm)
    per = np.diff(c.hits.offsets.astype(np.int64))
    m = per[0::2] + per[1::2]
    for edge in (hc.LANE_HITS, 64, hc.WAVE_HITS):  # p, q and p + q on both sides of every edge
        for x in (per[0::2], per[1::2], m):
            assert (x <= edge).any() and (x > edge).any()
    nk = c.hits.n_kmers.astype(np.int64)
    assert ((nk[0::2] + nk[1::2]) >= 2 ** 32).any()  # n_1 + n_2 wraps
    for rule in ([(0, 0), (0, 1000)] if name.startswith("wide") else hc.RULES):
        same(fvm.batch_literal(c.hits, rule), fvm.batch_anc(c.hits, rule, c.plain.calls), (name, rule))


@pytest.fixture(scope="module")
def readme():
    """the database of the read-support cases: its tree holds 5 -> 6 -> 8 and 5 -> 35 -> 36; X is on another lineage"""
    parent, cum, keys, targets = sc.database()
    hm = HitModel(oracle_db(parent, keys, targets, 20), keys, targets, 30)
    sm = SupportModel(hm, parent)
    _, x = vc.hand_built(parent, keys, targets, np.random.default_rng(78))
    assert [int(parent[8]), int(parent[6]), int(parent[36]), int(parent[35])] == [6, 5, 35, 5] and sc.top_level(parent, x) != 5
    return FragmentVoteModel(VoteModel(sm)), hm, x


def test_the_worked_cases_give_the_stated_records(readme):
    fvm, hm, x = readme
    pick = lambda rec: tuple(int(rec[i]) for i in (0, 4, 5, 8, 9))  # noqa: E731  call, p_best, n_best, call_1, call_2
    assert pick(fvm.fragment_literal([8], 121, [36], 121, (0, 0))) == (5, 1, 2, 8, 36)
    assert pick(fvm.fragment_literal([x, 8], 121, [6], 121, (0, 0))) == (8, 2, 1, 1, 6)  # mate 1 alone is a tie
    assert pick(fvm.fragment_literal([8], 121, [x, 6], 121, (0, 0))) == (8, 2, 1, 8, 1)
    assert hm.fold([8, x, 6]) == 6  # ... where the fragment's left fold says 6
    assert pick(fvm.fragment_literal([], 0, [6, 8], 121, (0, 0))) == (8, 2, 1, 0, 8)
    rec = fvm.fragment_literal([8], 121, [x, 6], 121, (0, 0))
    assert rec[2:4] == (242, 3) and rec[1] == 8 and rec[6] == 1  # n, m; under (0, 0) confident = call; S(8) = 1
    assert fvm.fragment_literal([], 0, [], 0, (0, 0)) == (0,) * 10


def small_batch(name="rows8"):
    c = hc.case(name)
    return c, FragmentVoteModel(c.models.vm)


def test_a_permutation_inside_a_mate_changes_nothing():
    c, fvm = small_batch()
    sh, _ = c.shuffled  # every read's hits in another order: every mate's
    assert not np.array_equal(sh.target, c.hits.target)
    for rule in [(0, 0), (2, 25)]:
        same(fvm.batch_anc(sh, rule), fvm.batch_anc(c.hits, rule, c.plain.calls), rule)
    same(fvm.batch_literal(sh, (2, 25)), fvm.batch_anc(c.hits, (2, 25)), "literal")


def test_an_exchange_of_the_mates_exchanges_the_per_mate_calls_alone():
    c, fvm = small_batch()
    ex = exchanged(c.hits)
    assert np.array_equal(ex.offsets[::2], c.hits.offsets[::2]) and not np.array_equal(ex.offsets, c.hits.offsets)
    for rule in [(0, 0), (2, 25)]:
        rec = fvm.batch_anc(c.hits, rule)
        assert (rec["call_1"] != rec["call_2"]).any()
        same(fvm.batch_anc(ex, rule), exchanged_records(rec), rule)
    same(fvm.batch_literal(ex, (2, 25)), exchanged_records(fvm.batch_literal(c.hits, (2, 25))), "literal")


def test_without_mate_2_the_record_is_mate_1s_vote_record_with_both_mates_windows():
    c, fvm = small_batch()
    h = c.hits
    n = h.offsets.size - 1
    off = np.empty(2 * n + 1, np.uint64)  # read r becomes mate 1 of fragment r; every mate 2 is empty with n_2 = 7
    off[0::2], off[1::2] = h.offsets, h.offsets[1:]
    nk = np.stack([h.n_kmers, np.full(n, 7, np.uint32)], 1).reshape(-1)
    lone = Hits(off, nk, h.pos, h.target, h.entry)
    assert np.array_equal(fragment_csr(lone).offsets, h.offsets)
    for rule in [(0, 0), (2, 25), (0, 1000)]:
        rec = fvm.batch_anc(lone, rule)
        with_n = Hits(h.offsets, (h.n_kmers.astype(np.int64) + 7).astype(np.uint32), h.pos, h.target, h.entry)
        votes = c.models.vm.batch_anc(with_n, rule)
        for f in votes.dtype.names:
            assert np.array_equal(rec[f], votes[f]), (rule, f)
        assert np.array_equal(rec["call_1"], rec["call"]) and not rec["call_2"].any()
        assert np.array_equal(rec["call"], c.plain.votes(rule)["call"])  # n plays no part in the call


@pytest.mark.parametrize("name", ["rows8", "climb9", "flat"])
def test_hits_on_one_root_path_are_called_as_the_fragments_final(name):
    c, fvm = small_batch(name)
    rec = fvm.batch_anc(c.hits, (0, 0))
    sm, n_line = c.models.sm, 0
    for i in range(rec.size):
        t = np.concatenate([c.hits.of(2 * i)[1], c.hits.of(2 * i + 1)[1]]).astype(np.int64)
        if t.size == 0:
            continue
        deepest = int(t[np.argmax(sm.depth[t])])
        if all(sm.under(deepest, int(x)) for x in np.unique(t)):
            n_line += 1
            assert int(rec[i]["call"]) == int(c.plain.fragment_finals[i]) == deepest, i
    assert n_line >= 3  # (the lists draw the shapes "one_path" and "one_deepest" for both mates of a few fragments per tree)
