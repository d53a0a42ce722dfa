"""The depth model (tests/read_depth_model.py) on hand-made cases, before any GPU is involved: the edges of the bins,
targets without a hit, all entries equal, the tie rule of the quartiles, saturation, and -- on the reads the GPU tests
use -- depth > 0 exactly where the support model's tally sees an entry.  The GPU tests hold the library against this."""
import numpy as np

import read_depth_model as dm
import read_support_cases as sc
from helpers import oracle_db
from read_hits_model import HitModel, Hits
from read_support_model import SUPPORT_DTYPE, SupportModel


def test_bin_edges_and_the_last_column():
    targets = np.array([2, 2, 2, 2, 3, 0, 2], np.uint32)
    for bins in (2, 3, 5, 256):
        depth = np.array([0, bins - 2, bins - 1, bins, 7, 0, dm.DEPTH_MAX], np.uint32)
        s, ksum, dmax = dm.spectrum_of(depth, targets, 4, bins)
        assert s.shape == (4, bins) and np.array_equal(s.sum(axis=1), np.bincount(targets, minlength=4))
        row = np.zeros(bins, np.uint64)
        row[0] += 1
        row[bins - 2] += 1       # (bins = 2: column 0 again, depth 0)
        row[bins - 1] += 3       # bins - 1, bins and the saturated counter
        assert np.array_equal(s[2], row)
        assert int(s[3, min(7, bins - 1)]) == 1 and int(s[0, 0]) == 1 and not s[1].any()
        assert int(ksum[2]) == 3 * bins - 3 + dm.DEPTH_MAX and int(dmax[2]) == dm.DEPTH_MAX and (int(ksum[3]), int(dmax[3])) == (7, 7)


def test_a_target_without_a_hit_and_all_entries_equal():
    s, ksum, dmax = dm.spectrum_of(np.array([0, 0, 5, 5, 5], np.uint32), np.array([2, 2, 3, 3, 3], np.uint32), 4, 256)
    assert dm.quartiles(s[2]) == (0, 0, 0, 0) and dm.quartiles(s[3]) == (3, 5, 5, 5) and dm.quartiles(s[0]) == (0, 0, 0, 0)
    assert dm.depth_lines(s, ksum, dmax) == "0,0,0,0,0,0,0\n1,0,0,0,0,0,0\n2,0,0,0,0,0,0\n3,15,3,5,5,5,5\n"


def test_the_quartile_tie_rule():
    """q_p is the SMALLEST d with 4 * #{1 <= depth <= d} >= p * distinct: with four entries at 1, 2, 3, 4 the quarter is
    reached exactly at d = 1, the half at d = 2; with two entries at 1 and 9 the half is reached at d = 1"""
    row = lambda depths: dm.spectrum_of(np.array(depths, np.uint32), np.full(len(depths), 1, np.uint32), 2, 256)[0][1]  # noqa: E731
    assert dm.quartiles(row([1, 2, 3, 4])) == (4, 1, 2, 3)
    assert dm.quartiles(row([1, 9])) == (2, 1, 1, 9)
    assert dm.quartiles(row([1, 1, 1, 1, 1])) == (5, 1, 1, 1)
    assert dm.quartiles(row([0, 0, 7])) == (1, 7, 7, 7)          # entries never hit do not enter
    assert dm.quartiles(row([3, 254, 255, 256, 70000])) == (5, 254, 255, 255)  # the last column is taken as d = 255
    assert dm.quartiles(row([1, 2, 3])) == (3, 1, 2, 3)          # 4 * 1 >= 1 * 3; 4 * 2 >= 2 * 3; 4 * 3 >= 3 * 3


def test_depth_of_counts_hits_not_reads_and_saturates():
    # three reads: hits (entry, target); read 1 has confident 0, read 2 is not counted
    hits = Hits(np.array([0, 4, 6, 7], np.uint64), np.array([50, 50, 50], np.uint32), np.zeros(7, np.uint32),
                np.array([5, 5, 1, 6, 5, 6, 5], np.uint32), np.array([3, 3, 0, 4, 3, 4, 3], np.uint32))
    rec = np.zeros(3, SUPPORT_DTYPE)
    rec["confident"] = [5, 0, 5]
    d = dm.depth_of(hits, rec, np.array([True, True, False]), 6)
    assert d.tolist() == [0, 0, 0, 2, 1, 0]  # the k-mer met twice adds 2; the target-1 hit adds nothing
    assert dm.saturating_add([0xFFFFFFF0, 1, 0xFFFFFFFE], [0x20, 2, 1]).tolist() == [dm.DEPTH_MAX, 3, dm.DEPTH_MAX]


def test_depth_is_positive_exactly_where_the_tally_sees_an_entry():
    parent, cum, keys, targets = sc.database()
    odb = oracle_db(parent, keys, targets, 20)
    hm = HitModel(odb, keys, targets, 30)
    model = SupportModel(hm, parent)
    bases, off, _ = sc.reads(parent, cum, keys, targets)
    hits = hm.batch(bases, off)
    finals = model.finals(hits)
    counted = np.ones(finals.size, bool)
    for rule in ((0, 0), (2, 25)):
        rec = model.batch_identity(hits, rule, finals)
        d = dm.depth_of(hits, rec, counted, keys.size)
        g, u = model.tally(hits, rec, counted, targets)
        s, ksum, dmax = dm.spectrum_of(d, targets, parent.size, 256)
        assert np.array_equal(s[:, 1:].sum(axis=1).astype(np.int64), u) and int(d.max()) > 1
        assert np.array_equal(s.sum(axis=1), np.bincount(targets, minlength=parent.size))
        assert int(ksum.sum()) == int(d.sum()) and int(dmax.max()) == int(d.max())
        lines = dm.depth_lines(s, ksum, dmax).splitlines()
        assert len(lines) == parent.size and all(int(x.split(",")[2]) == int(u[i]) for i, x in enumerate(lines))
