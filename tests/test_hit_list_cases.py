"""The synthetic hit lists of tests/hit_list_cases.py before any GPU is involved: the trees have the stated shapes, the
lists hold the cases they exist for -- stated as conditions on the models' records, not on the code under test -- and the
literal and the vectorised forms of the vote and support models agree on these trees."""
import numpy as np
import pytest

import hit_list_cases as hc

DECIDING = ("rows8", "climb9", "wide_rows", "wide_climb")


@pytest.mark.parametrize("name", sorted(hc.TREES))
def test_trees_have_the_stated_shape(name):
    c = hc.case(name)
    ntar, max_depth = hc.TREES[name]
    assert c.parent.size == ntar and c.parent.dtype == np.int32 and int(c.depth.max()) == max_depth
    assert np.array_equal(c.depth[1:], c.models.sm.depth[1:])  # the generator's depths are the model's
    deepest = np.flatnonzero(c.depth == max_depth)
    if name == "rows8":
        parents, counts = np.unique(c.parent[deepest], return_counts=True)
        assert deepest.size >= 6 and parents.size >= 2 and int(counts.max()) >= 2 and np.all(c.depth[parents] == 7)
    if name == "flat":
        assert np.all(c.parent == 1)
    p2, d2 = hc.tree(name, hc.SEEDS[name])
    assert np.array_equal(p2, c.parent) and np.array_equal(d2, c.depth)  # seeded


@pytest.mark.parametrize("name", sorted(hc.TREES))
def test_lists_have_the_stated_shape(name):
    c = hc.case(name)
    h = c.hits
    per = np.diff(h.offsets.astype(np.int64))
    assert per.size == hc.N_READS == 204
    for cyc in range(hc.N_CYCLES):
        assert sorted(per[cyc * 17:(cyc + 1) * 17].tolist()) == sorted(hc.M_VALUES)
    assert set(c.shapes) == set(hc.SHAPES)
    assert h.target.min() >= 1 and h.target.max() < c.ntar
    nk = h.n_kmers.astype(np.int64)
    for kind in (nk == per, nk == per + 91, nk == 0, nk == 1, nk == hc.WRAP_N, nk == 2 ** 32 - 1):
        assert int(kind.sum()) >= 10
    # every work split of the three kernels, as reads and as fragments
    L, W = hc.LANE_HITS, hc.WAVE_HITS
    p, q = per[0::2], per[1::2]
    lo, hi = np.minimum(p, q), np.maximum(p, q)
    assert ((p == 0) & (q > 0)).any() and ((p > 0) & (q == 0)).any()
    assert ((lo > 0) & (lo <= L) & (hi > L)).any() and ((lo > 0) & (lo < 64) & (hi > 64)).any()
    assert ((p > 0) & (q > 0) & (p + q <= L)).any() and ((p % 64 != 0) & (q > 0) & (p > 64)).any()
    if name.startswith("wide"):
        assert (h.target == c.ntar - 1).any() and (h.target == 32768).any() and int((h.target >= 32768).sum()) > 1000
    big = np.flatnonzero(per > W)
    assert big.size == 36 and {c.shapes[r] for r in big} == set(hc.SHAPES)
    # the variants
    raw, exp = c.out_of_range
    moved = raw.target != h.target
    assert 0.01 < moved.mean() < 0.03 and set(np.unique(raw.target[moved]).tolist()) == {0, c.ntar, 0xFFFFFFFF}
    assert np.all(exp.hits.target[moved] == 1) and np.array_equal(exp.hits.target[~moved], h.target[~moved])
    sh, _ = c.shuffled
    assert not np.array_equal(sh.target, h.target)
    for r in range(hc.N_READS):
        assert np.array_equal(np.sort(sh.of(r)[1]), np.sort(h.of(r)[1]))


@pytest.mark.parametrize("name", sorted(hc.TREES))
def test_the_cases_decide_something(name):
    c = hc.case(name)
    e, per = c.plain.votes((0, 0)), np.diff(c.hits.offsets.astype(np.int64))
    tie = e["n_best"] > 1
    counts = (int((tie & (e["call"] > 1)).sum()), int((tie & (e["call"] == 1)).sum()), int((e["call"] != c.plain.finals).sum()),
              int((c.depth[e["call"].astype(np.int64)] == c.max_depth).sum()))
    all_or_nothing = c.plain.votes((0, 1000))
    flips = int((e["confident"] != all_or_nothing["confident"]).sum())
    wrap = (c.hits.n_kmers == hc.WRAP_N) & (per > 0) & (per < 4000) & (e["call"] > 0)
    print("%s: ties below the root %d, ties at the root %d, call != final %d, call at the deepest level %d, confident flips %d, "
          "largest n_best %d, wrap reads %d" % ((name,) + counts + (flips, int(e["n_best"].max()), int(wrap.sum()))))
    if name not in DECIDING:
        assert counts[0] == 0 and counts[1] >= 5  # flat: no tie below the root by construction
        return
    assert counts[0] >= 5 and counts[1] >= 5 and counts[2] >= 20 and counts[3] >= 20 and flips >= 20 and int(wrap.sum()) >= 1
    # a read with that n_kmers passes (0, 1000) only by a product that wraps
    assert not all_or_nothing["confident"][wrap].any()
    s = c.plain.support((0, 1000))
    assert not s["confident"][wrap & (c.plain.finals > 0)].any()


@pytest.mark.parametrize("name", sorted(hc.TREES))
def test_the_models_vouch_for_each_other(name):
    c = hc.case(name)
    rule, n = (2, 25), 40
    h = c.hits
    sub = hc.Hits(h.offsets[:n + 1], h.n_kmers[:n], h.pos, h.target, h.entry)
    assert int(np.diff(sub.offsets.astype(np.int64)).max()) == 5000
    lit = c.models.vm.batch_literal(sub, rule)
    vec = c.plain.votes(rule)[:n]
    for f in lit.dtype.names:
        assert np.array_equal(lit[f], vec[f]), (name, f)
    lit = c.models.sm.batch_literal(sub, rule, c.plain.finals[:n])
    vec = c.plain.support(rule)[:n]
    for f in lit.dtype.names:
        assert np.array_equal(lit[f], vec[f]), (name, f)
    # the fragment record of read_fragments_model.FragmentModel on the pairs whose n_1 + n_2 fits 32 bits
    from read_fragments_model import FragmentModel
    fm, frag = FragmentModel(c.models.sm), c.plain.fragments(rule)
    fits = h.n_kmers[0:n:2].astype(np.int64) + h.n_kmers[1:n:2].astype(np.int64) < 2 ** 32
    assert int(fits.sum()) >= 10
    for i in np.flatnonzero(fits):
        one = fm.fragment(h.of(2 * i)[1].tolist(), h.n_kmers[2 * i], h.of(2 * i + 1)[1].tolist(), h.n_kmers[2 * i + 1], rule)
        assert tuple(int(x) for x in frag[i]) == tuple(int(x) for x in one), (name, int(i))
