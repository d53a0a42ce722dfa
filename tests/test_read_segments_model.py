"""The segment model (tests/read_segments_model.py) before any GPU is involved: the geometry's properties, the literal
form (every segment a read of its own on copied text, through HitModel.batch and SupportModel.batch_literal) against the
direct form (the read's hits sliced by pos), and one segment per read against the SupportModel record.  The GPU tests
then hold kid_db_read_segments* against the direct form."""
import numpy as np
import pytest

import read_support_cases as sc
from helpers import concat_reads, oracle_db
from read_hits_model import HitModel
from read_segments_model import MAX_OVERLAP, SegmentModel, geometry
from read_support_model import SUPPORT_DTYPE, SupportModel

SETTINGS = [(1, 1), (63, 63), (64, 64), (65, 13), (100, 50), (121, 121), (10 ** 6, 10 ** 6)]


def test_geometry_properties():
    for seg_len in (1, 2, 63, 64, 65, 100):
        for seg_step in sorted({1, 2, 13, seg_len // 2, seg_len - 1, seg_len}):
            if not 1 <= seg_step <= seg_len:
                continue
            assert geometry(0, seg_len, seg_step)[0].size == 0
            for P in range(1, 300):
                q, m = geometry(P, seg_len, seg_step)
                what = (P, seg_len, seg_step)
                assert q.size >= 1 and q[0] == 0 and np.all(m >= 1), what
                assert np.array_equal(q, np.arange(q.size) * seg_step), what
                assert q[-1] + m[-1] == P, what                       # the last segment ends at P
                assert np.all(m[:-1] == seg_len), what                # only the last may be shorter
                assert np.all(q[1:] <= q[:-1] + m[:-1]), what         # every position is covered
                assert np.all(q[1:] + m[1:] > q[:-1] + m[:-1]), what  # no segment lies inside the one before it
                assert (q.size == 1) == (P <= seg_len), what
    with pytest.raises(AssertionError):
        geometry(10, MAX_OVERLAP + 1, 1)
    assert geometry(5000, MAX_OVERLAP, 1)[0].size == 5000 - MAX_OVERLAP + 1


@pytest.fixture(scope="module")
def world():
    parent, cum, keys, targets = sc.database()
    bases, off, where = sc.reads(parent, cum, keys, targets)
    hm = HitModel(oracle_db(parent, keys, targets, 20), keys, targets, 30)
    sm = SupportModel(hm, parent)
    return sm, bases, off


def same(a, b, what):
    assert np.array_equal(a[0], b[0]), what
    bad = np.flatnonzero(a[1] != b[1])
    assert bad.size == 0, (what, int(bad[0]), a[1][bad[0]], b[1][bad[0]])


def test_literal_and_direct_forms_agree(world):
    sm, bases, off = world
    whole = SegmentModel(sm, bases, off)
    called = 0
    for seg_len, seg_step in SETTINGS[1:]:
        for rule in [(0, 0), (2, 25)]:
            dire = whole.direct(seg_len, seg_step, rule)
            same(whole.literal(seg_len, seg_step, rule), dire, (seg_len, seg_step, rule))
            called += int((dire[1]["confident"] != dire[1]["final"]).sum())
    assert called > 0  # the rule (2, 25) un-calls or lifts some segment
    # (1, 1) makes every window a read of its own: 315 000 of them for the literal form -- on every 5th read of the world
    pick = np.arange(0, off.size - 1, 5)
    b, o = concat_reads([bases[int(off[r]):int(off[r + 1])].tobytes() for r in pick])
    m = SegmentModel(sm, b, o)
    for rule in [(0, 0), (2, 25)]:
        same(m.literal(1, 1, rule), m.direct(1, 1, rule), (1, 1, rule))
    # trimmed ranges: pos counts from the first byte of the read
    lens = np.diff(o.astype(np.int64))
    start = np.minimum(7, np.maximum(lens - 1, 0)).astype(np.int32)
    stop = np.maximum(lens - 4, 0).astype(np.int32)
    mt = SegmentModel(sm, b, o, start, stop)
    la, lit = mt.literal(40, 20, (2, 25))
    da, dire = mt.direct(40, 20, (2, 25))
    assert np.array_equal(la, da) and np.array_equal(lit, dire)
    first = la[:-1][np.diff(la.astype(np.int64)) > 0].astype(np.int64)
    assert np.array_equal(dire["pos"][first], start[np.diff(la.astype(np.int64)) > 0])


def test_one_segment_per_read_is_the_support_record(world):
    sm, bases, off = world
    m = SegmentModel(sm, bases, off)
    hits = sm.hm.batch(bases, off)
    finals = sm.finals(hits)
    for rule in [(0, 0), (2, 25), (3, 0)]:
        so, seg = m.direct(10 ** 6, 10 ** 6, rule)
        exp = sm.batch_identity(hits, rule, finals)
        has = m.P > 0
        assert np.array_equal(np.diff(so.astype(np.int64)), has.astype(np.int64))
        assert not seg["pos"].any() and np.array_equal(seg["n_pos"], m.P[has])
        for f in SUPPORT_DTYPE.names:
            assert np.array_equal(seg[f], exp[f][has]), (rule, f)
        assert not exp["n_hits"][~has].any()
