"""tests/read_pileup_model.py held to the worked case of include/kmer_id_amd.h field by field, to the properties the rule
promises (any order, the sum of parts) and to the step-array form the kernels use; and the synthetic records of
tests/read_pileup_cases.py checked for covering what they are for.  No GPU."""
import numpy as np

import read_loci_model as lm
import read_pileup_cases as pc
import read_pileup_model as pm
from kmer_id_amd import PILEUP_DTYPE

K, W = 30, 100
# organism 3 with entries at positions 0, 100, 250, 990; an entry of organism 1 in front so that entry numbers and positions differ
ORG = np.array([1, 3, 3, 3, 3], np.uint32)
POS = np.array([40, 0, 100, 250, 990], np.uint32)


def worked_records():
    a = pc.locus(3, 0, 5, 0, 10, 130, 2)   # forward at pos 100: [100, 249], bins 1..2
    b = pc.locus(3, 1, 3, 2, 0, 120, 3)    # reverse at pos 250: [130, 279], bins 1..2
    c = pc.locus(3, 0, 2, 2, 7, 107, 4)    # forward at pos 990, margin 0
    return np.array([a, b, c], lm.LOCUS_DTYPE)


def test_the_record_layout_is_the_bindings():
    assert PILEUP_DTYPE == pm.PILEUP_DTYPE and PILEUP_DTYPE.itemsize == 48
    assert [PILEUP_DTYPE.fields[f][1] for f in PILEUP_DTYPE.names] == [4 * i for i in range(9)] + [40]
    assert PILEUP_DTYPE.names[-1] == "depth_sum" and PILEUP_DTYPE.fields["depth_sum"][0] == np.uint64


def test_the_worked_case_field_by_field():
    loci = worked_records()
    span, bin_base = pm.geometry(ORG, POS, W)
    assert span.tolist() == [0, 1, 0, 10] and bin_base.tolist() == [0, 0, 1, 1, 11]
    assert [pm.placed(L, ORG, 2, 1) for L in loci] == [True, True, False]
    assert pm.interval(loci[0], POS, K) == (100, 249) and pm.interval(loci[1], POS, K) == (130, 279)
    s, d, n1 = pm.walk(loci, ORG, POS, K, W, span, 2, 1)
    assert pm.placed(loci[2], ORG, 2, 0) and pm.interval(loci[2], POS, K) == (990, 1119)
    s, d, n2 = pm.walk(loci[2:], ORG, POS, K, W, span, 2, 0, s, d)  # the third once more under (2, 0): both ends clamp to bin 9
    assert (n1, n2) == (2, 1)
    starts, depth = pm.dense(s, span, bin_base), pm.dense(d, span, bin_base)
    assert starts[1:].tolist() == [0, 2, 0, 0, 0, 0, 0, 0, 0, 1] and starts[0] == 0
    assert depth[1:].tolist() == [0, 2, 2, 0, 0, 0, 0, 0, 0, 1] and depth[0] == 0
    rec = pm.records(span, bin_base, starts, depth)
    assert rec[3].tolist() == (3, 10, 3, 6, 2, 1, 2, 1, 0, 5)
    assert rec[1].tolist() == (0, 1, 0, 1, 0, 0, 0, 0, 0, 0)  # nothing placed: max_gap = span_bins
    assert rec[0].tolist() == rec[2].tolist() == (0,) * 10    # no entries: all zero


def test_what_is_not_placed_changes_nothing():
    ok = pc.locus(3, 0, 5, 0, 10, 130, 2)
    bad = []
    for field, value in (("strand", 2), ("entry_first", 5), ("entry_first", 0xFFFFFFFF), ("org", 1), ("n_chain", 1), ("n_other", 5)):
        r = ok.copy()
        r[field] = value
        bad.append(r)
    out = pm.batch(np.array(bad, lm.LOCUS_DTYPE), ORG, POS, K, W, 2, 1)
    assert out[4] == 0 and not out[1].any() and not out[2].any()
    assert pm.batch(np.array([ok]), ORG, POS, K, W, 2, 1)[4] == 1
    r = ok.copy()
    r["pos_first"], r["pos_last"] = 130, 10  # pos_last < pos_first: d = 0
    assert pm.interval(r, POS, K) == (100, 129)
    r = pc.locus(3, 1, 5, 0, 0, 400, 3)      # reverse at pos 250 with d = 400: lo = max(0, -150)
    assert pm.interval(r, POS, K) == (0, 279)


def same(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[4] == b[4]
    assert a[3].tobytes() == b[3].tobytes()


def test_any_order_and_the_sum_of_parts():
    org, pos = pc.small()
    loci, exp = pc.small_case(7)
    rule = pc.RULE
    whole = pm.batch(loci, org, pos, K, 7, *rule)
    assert whole[4] == exp.n_placed and 50 < whole[4] < loci.size - 50
    same(whole, pm.batch(loci[np.random.default_rng(3).permutation(loci.size)], org, pos, K, 7, *rule))
    parts = [pm.batch(loci[a:b], org, pos, K, 7, *rule) for a, b in ((0, 1), (1, 150), (150, loci.size))]
    assert np.array_equal(sum(p[1].astype(np.uint64) for p in parts), whole[1])
    assert np.array_equal(sum(p[2].astype(np.uint64) for p in parts), whole[2])
    assert sum(p[4] for p in parts) == whole[4]


def test_the_step_array_form_equals_the_walk():
    for w in pc.SMALL_WIDTHS:
        org, pos = pc.small()
        loci, exp = pc.small_case(w)
        starts, step = pm.steps(loci, org, pos, K, w, *pc.RULE)
        span, bin_base = pm.geometry(org, pos, w)
        assert np.array_equal(starts, exp.starts)
        assert np.array_equal(pm.depth_of_steps(step, span, bin_base), exp.depth)
        assert np.array_equal(step, exp.steps)
        # every organism's steps sum to zero: the sentinel closes them
        for g in range(span.size):
            a = int(bin_base[g]) + g
            assert int(step[a:a + int(span[g]) + 1].astype(np.uint64).sum()) % 2 ** 32 == 0
    # a chain whose b_hi is its organism's last bin uses the sentinel, and the one-bin neighbours see nothing of it
    org, pos = pc.small()
    one = np.array([pc.locus(0, 0, 9, 0, 0, 500, 0), pc.locus(3, 0, 9, 0, 0, 500, 301)], lm.LOCUS_DTYPE)
    starts, step = pm.steps(one, org, pos, K, 1, 2, 1)
    assert step.tolist()[:4] == [1, 2 ** 32 - 1, 0, 0] and step[-2] == 1 and step[-1] == 2 ** 32 - 1
    span, bin_base = pm.geometry(org, pos, 1)
    assert pm.depth_of_steps(step, span, bin_base).tolist() == [1, 0] + [0] * 299 + [1]


def test_the_cases_cover_what_they_are_for():
    assert pc.SCAN_TILE >= 64 and pc.SCAN_SLOTS[-1] == pc.SCAN_TILE ** 2 + 1
    for (org, pos), (loci, exp), w in [(pc.small(), pc.small_case(1), 1), (pc.big(), pc.big_case(4096), 4096)]:
        mc, mm = pc.RULE
        ne = org.size
        assert {mc - 1, mc, mc + 1} <= set(loci["n_chain"].tolist())
        assert (loci["n_other"] < loci["n_chain"]).any() and (loci["n_other"] == loci["n_chain"]).any() and (loci["n_other"] > loci["n_chain"]).any()
        margin = loci["n_chain"].astype(np.int64) - loci["n_other"]
        assert {mm - 1, mm, mm + 1} <= set(margin.tolist())
        assert {0, 1, 2} == set(loci["strand"].tolist())
        assert {ne - 1, ne, 0xFFFFFFFF} <= set(loci["entry_first"].tolist())
        inside = loci["entry_first"] < ne
        assert (loci["org"][inside] != org[loci["entry_first"][inside]]).sum() >= 5
        assert (loci["pos_last"] < loci["pos_first"]).sum() >= 5
        assert int(loci["pos_first"].max()) == 2 ** 32 - 1 and int(loci["pos_last"].max()) == 2 ** 32 - 1
        span = exp.span
        sel = [L for L in loci if pm.placed(L, org, mc, mm)]
        assert 40 < len(sel) < loci.size - 40 and len(sel) == exp.n_placed
        lo_hi = [(L, pm.interval(L, pos, K)) for L in sel]
        a_minus_d = [int(pos[int(L["entry_first"])]) - max(int(L["pos_last"]) - int(L["pos_first"]), 0) for L in sel if int(L["strand"]) == 1]
        assert min(a_minus_d) < 0, "lo below 0 on the reverse strand"
        assert any(hi // w > int(span[int(L["org"])]) - 1 for L, (lo, hi) in lo_hi), "hi past the span"
        assert any(hi // w == int(span[int(L["org"])]) - 1 for L, (lo, hi) in lo_hi), "b_hi exactly the last bin"
        assert any(lo // w == 0 and hi // w >= int(span[int(L["org"])]) - 1 and span[int(L["org"])] > 1 for L, (lo, hi) in lo_hi), "a whole span"
    org, pos = pc.small()
    assert pm.geometry(org, pos, 1)[0].tolist() == [1, 1, 0, 300] and pm.geometry(org, pos, 7)[0].tolist() == [1, 1, 0, 43]
    for n in pc.SCAN_SLOTS:
        span, bin_base = pm.geometry(*pc.scan_table(n), 1)
        assert int(bin_base[-1]) + span.size == n
    span, bin_base = pm.geometry(*pc.big(), 1)
    assert int(bin_base[-1]) > 2 ** 28 and span.size == 2 ** 24
    hot, exp = pc.shape_case("hot_spot", 7)
    assert np.count_nonzero(exp.starts) == 1 and exp.n_placed == int(exp.depth.max()) == int(exp.starts.max()) and 99000 < exp.n_placed < 100000
    uni, exp = pc.shape_case("uniform", 7)
    assert np.count_nonzero(exp.depth) == exp.depth.size and exp.n_placed > 60000
