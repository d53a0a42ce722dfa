"""The segment-vote model (tests/read_segment_votes_model.py) before any GPU is involved: the literal form (every segment
a read of its own on copied text, through HitModel.batch and VoteModel.batch_literal) against the direct form (the
read's hits sliced by pos), the geometry fields against SegmentModel.direct, one segment per read against the VoteModel
record, and the property the rule is there for: a record and its reverse complement get mirrored segment records,
where the fold's `final` does not.  The GPU tests then hold kid_db_read_segment_votes* against the direct form."""
import numpy as np
import pytest

import read_support_cases as sc
from helpers import concat_reads, oracle_db
from read_calls import RC_SETTINGS, mirrored, strand_world
from read_hits_model import HitModel
from read_segment_votes_model import VOTE_FIELDS, SegmentVoteModel, segment_votes_line
from read_segments_model import SegmentModel
from read_support_model import SupportModel

SETTINGS = [(63, 63), (64, 64), (65, 13), (100, 50), (121, 121), (10 ** 6, 10 ** 6)]


@pytest.fixture(scope="module")
def world():
    parent, cum, keys, targets = sc.database()
    bases, off, where = sc.reads(parent, cum, keys, targets)
    hm = HitModel(oracle_db(parent, keys, targets, 20), keys, targets, 30)
    sm = SupportModel(hm, parent)
    return sm, bases, off, parent, targets


def same(a, b, what):
    assert np.array_equal(a[0], b[0]), what
    bad = np.flatnonzero(a[1] != b[1])
    assert bad.size == 0, (what, int(bad[0]), a[1][bad[0]], b[1][bad[0]])


def test_literal_and_direct_forms_agree(world):
    sm, bases, off = world[:3]
    whole = SegmentVoteModel(sm, bases, off)
    fold = SegmentModel(sm, bases, off)
    lifted = differ = 0
    for seg_len, seg_step in SETTINGS:
        for rule in [(0, 0), (2, 25)]:
            what = (seg_len, seg_step, rule)
            dire = whole.direct(seg_len, seg_step, rule)
            same(whole.literal(seg_len, seg_step, rule), dire, what)
            # the geometry is the segment model's
            fo, frec = fold.direct(seg_len, seg_step, rule)
            assert np.array_equal(fo, dire[0]), what
            for f in ("pos", "n_pos", "n_kmers", "n_hits"):
                assert np.array_equal(frec[f], dire[1][f]), (what, f)
            rec = dire[1]
            none = rec["n_hits"] == 0
            for f in ("call", "confident", "p_best", "n_best", "s_call", "s_confident"):
                assert not rec[f][none].any(), (what, f)
            assert np.all(rec["call"][~none] > 0) and np.all(rec["p_best"][~none] >= 1) and np.all(rec["n_best"][~none] >= 1), what
            if rule == (0, 0):
                assert np.array_equal(rec["confident"], rec["call"]), what
            lifted += int((rec["confident"] != rec["call"]).sum())
            differ += int((rec["call"] != frec["final"]).sum())
    assert lifted > 0  # the rule (2, 25) un-calls or lifts some segment
    assert differ > 0  # and somewhere the vote is not the fold
    # trimmed ranges: pos counts from the first byte of the read
    pick = np.arange(0, off.size - 1, 5)
    b, o = concat_reads([bases[int(off[r]):int(off[r + 1])].tobytes() for r in pick])
    lens = np.diff(o.astype(np.int64))
    start = np.minimum(7, np.maximum(lens - 1, 0)).astype(np.int32)
    stop = np.maximum(lens - 4, 0).astype(np.int32)
    mt = SegmentVoteModel(sm, b, o, start, stop)
    same(mt.literal(40, 20, (2, 25)), mt.direct(40, 20, (2, 25)), "trimmed")


def test_one_segment_per_read_is_the_vote_record(world):
    sm, bases, off = world[:3]
    m = SegmentVoteModel(sm, bases, off)
    hits = sm.hm.batch(bases, off)
    for rule in [(0, 0), (2, 25), (3, 0)]:
        so, seg = m.direct(10 ** 6, 10 ** 6, rule)
        exp = m.vm.batch_anc(hits, rule)
        has = m.P > 0
        assert np.array_equal(np.diff(so.astype(np.int64)), has.astype(np.int64))
        assert not seg["pos"].any() and np.array_equal(seg["n_pos"], m.P[has])
        for f in VOTE_FIELDS:
            assert np.array_equal(seg[f], exp[f][has]), (rule, f)


def test_one_root_path_gives_the_fold(world):
    sm, bases, off = world[:3]
    m = SegmentVoteModel(sm, bases, off)
    fold = SegmentModel(sm, bases, off)
    hits, _ = m._whole()
    so, rec = m.direct(100, 50, (0, 0))
    frec = fold.direct(100, 50, (0, 0))[1]
    checked = 0
    for r in range(m.n):
        hp, ht, _ = hits.of(r)
        for s in range(int(so[r]), int(so[r + 1])):
            tg = ht[(hp >= rec["pos"][s]) & (hp < rec["pos"][s] + rec["n_pos"][s])].tolist()
            if len(set(tg)) < 2:
                continue
            deepest = max(tg, key=lambda t: len(m.vm.root_path(t)))
            if set(tg) <= set(m.vm.root_path(deepest)):  # all hits on one root path
                assert rec["call"][s] == frec["final"][s] == deepest, (r, s, tg)
                checked += 1
    assert checked > 20


def test_reverse_complement_mirrors_the_votes_and_not_the_fold(world):
    sm0, _, _, parent, targets = world
    keys, tg, bases, off = strand_world(parent, targets)
    hm = HitModel(oracle_db(parent, keys, tg, 16), keys, tg, 30)
    sm = SupportModel(hm, parent)
    votes, fold = SegmentVoteModel(sm, bases, off), SegmentModel(sm, bases, off)
    assert votes.P.tolist() == [2000, 2000]
    for seg in RC_SETTINGS:
        for rule in [(0, 0), (2, 25)]:
            so, rec = votes.direct(seg[0], seg[1], rule)
            a, b = mirrored(so, rec, (seg, rule))
            assert a.size == {100: 39, 500: 7, 2000: 1}[seg[0]]
            for f in VOTE_FIELDS:
                assert np.array_equal(a[f], b[f]), (seg, rule, f)
            assert np.array_equal(a["n_hits"], a["n_pos"])  # every window of either strand is in the database
        fo, frec = fold.direct(seg[0], seg[1], (0, 0))
        fa, fb = mirrored(fo, frec, seg)
        # what the rule is for: the fold depends on the strand (without this the test above would show nothing)
        assert int((fa["final"] != fb["final"]).sum()) >= 1, seg


def test_segment_votes_line():
    rec = np.zeros(3, [(f, np.uint32) for f in ("pos", "n_pos") + tuple(VOTE_FIELDS)])
    rec[0] = (0, 100, 8, 6, 100, 3, 2, 1, 3, 3)
    rec[2] = (100, 71, 5, 0, 70, 2, 1, 2, 2, 0)
    assert segment_votes_line(6, 200, rec, b"@r1 x") == b"6\t200\t3\t2\t0:100:100:3:8:6:2:1 100:71:70:2:5:0:1:2\t@r1 x\n"
    assert segment_votes_line(6, 200, rec[1:2], b"@r1") == b""
