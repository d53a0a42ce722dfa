"""Breadth of coverage per organism (kid_seen_coverage / kid_seen_coverage_bins) against the models of
tests/seen_coverage_model.py: every field of every record and the per-bin arrays, exactly, for entry counts at the edges
of a word, a tile and a workgroup's span, for entries in (org, pos) order and under a seeded shuffle (the same bytes), for
runs of one bin across those edges, organisms of 0 .. 3000 bins and 70 000 organisms, a bin of 70 000 seen entries, the
bin widths at their extremes, 1 .. 64 bitmaps, a live sample; the argument errors write nothing."""
import ctypes as C

import numpy as np
import pytest

import seen_coverage_model as cm
import shared_kmers_model as sm
from helpers import small_db
from kmer_id_amd import COVERAGE_DTYPE, KidError, KmerDB, _lib, seen_coverage, seen_coverage_bins, synth
from read_calls import header_constant

pytestmark = pytest.mark.gpu

TILE = header_constant("kid_coverage.hip.h", "KID_COV_TILE")
SPAN = TILE * header_constant("kid_coverage.hip.h", "KID_COV_MIN_SPAN")  # entries a workgroup takes at least


def same_records(got, exp, what):
    assert got.dtype == COVERAGE_DTYPE and got.shape == exp.shape, what
    for name in cm.FIELDS:
        bad = np.argwhere(got[name] != exp[name])
        assert bad.size == 0, "%s: %s of bitmap %d, organism %d: got %d, the model %d" % (
            (what, name) + tuple(bad[0]) + (int(got[name][tuple(bad[0])]), int(exp[name][tuple(bad[0])])))


def check(org, pos, maps, width, n_orgs, what, model=cm.coverage, bins=True):
    """both calls against the model -> the records"""
    org, pos = np.asarray(org, np.uint32), np.asarray(pos, np.uint32)
    got = seen_coverage(org, pos, maps, bin_width=width, n_orgs=n_orgs)
    same_records(got, model(org, pos, maps, width, n_orgs), what)
    if bins:
        base, probes, seen = seen_coverage_bins(org, pos, maps, bin_width=width, n_orgs=n_orgs)
        e_base, e_probes, e_seen = cm.bins_model(org, pos, maps, width, n_orgs)
        assert base.dtype == np.uint64 and probes.dtype == seen.dtype == np.uint32, what
        assert np.array_equal(base, e_base) and np.array_equal(probes, e_probes) and np.array_equal(seen, e_seen), what
    return got


def check_both_orders(org, pos, bits, width, n_orgs, what, seed=7, **kw):
    """bits: bool[n_entries] per bitmap.  In the order given and under a seeded shuffle: the same bytes"""
    org, pos = np.asarray(org, np.uint32), np.asarray(pos, np.uint32)
    first = check(org, pos, [sm.pack(b, pad_ones=True) for b in bits], width, n_orgs, what, **kw)
    perm = np.random.default_rng(seed).permutation(org.size)
    again = check(org[perm], pos[perm], [sm.pack(np.asarray(b)[perm], pad_ones=True) for b in bits], width, n_orgs, what + ", shuffled", **kw)
    assert again.tobytes() == first.tobytes(), what
    return first


def some_bits(n, seed, extra=()):
    """no bit, every bit, 2 % and 50 % of them (the last one twice), then `extra`"""
    rng = np.random.default_rng(seed)
    dense = rng.random(n) < 0.5
    return [np.zeros(n, bool), np.ones(n, bool), rng.random(n) < 0.02, dense, dense] + list(extra)


# ------------------------------------------------------------------ 1. genomes of 0 .. 3000 bins, about 200 000 entries
def genomes():
    """organism 0 without an entry, then organisms of 1, 63, 64, 65 and 3000 bins of 1000 bases, in (org, pos) order; the big
    one has a stretch without probes.  200 003 entries: no multiple of 128"""
    org, pos = [], []
    for g, (last, step) in enumerate([(999, 1), (62999, 5), (63999, 5), (64999, 5), (2999999, 21)], start=1):
        p = np.arange(0, last, step)
        p[-1] = last  # the last bin is occupied whatever the step
        if g == 5:
            p = p[(p < 500000) | (p >= 520000)]
        org.append(np.full(p.size, g))
        pos.append(p)
    org, pos = np.concatenate(org), np.concatenate(pos)
    more = 200003 - org.size  # the rest goes to organism 1, bin 0
    assert more > 0
    org, pos = np.concatenate([np.full(more, 1), org]), np.concatenate([np.arange(more) % 1000, pos])
    order = np.lexsort((pos, org))
    return org[order].astype(np.uint32), pos[order].astype(np.uint32)


@pytest.fixture(scope="module")
def genome_case():
    org, pos = genomes()
    locus = (org == 5) & (pos // 1000 >= 1000) & (pos // 1000 <= 1010)  # one locus of the big organism alone
    return org, pos, some_bits(org.size, 1, [locus])


def test_genomes_in_order_and_shuffled(genome_case):
    org, pos, bits = genome_case
    assert org.size % 128 != 0 and org.size > 100 * SPAN
    recs = check_both_orders(org, pos, bits, 1000, 6, "genomes")
    assert recs["span_bins"][0].tolist() == [0, 1, 63, 64, 65, 3000]
    assert np.all(recs["bins"][1][1:5] == recs["span_bins"][1][1:5]) and recs["bins"][1][5] == 3000 - 20
    assert np.all(recs["max_gap"][0] == recs["bins"][0]) and np.all(recs["max_gap"][1] == 0)
    assert recs[5][5]["bins_seen"] == 11 and recs[5][5]["max_gap"] == 3000 - 1011 and recs[5][5]["max_bin"] in range(1000, 1011)


@pytest.mark.parametrize("width", [1, 500, 3000000, 1 << 31])
def test_genomes_at_other_bin_widths(genome_case, width):
    org, pos, bits = genome_case
    recs = check(org, pos, [sm.pack(b, pad_ones=True) for b in bits[2:4]], width, 6, "genomes, W = %d" % width, bins=width >= 500)
    if width >= 3000000:  # above every position: one bin per organism
        assert recs["span_bins"][0].tolist() == [0, 1, 1, 1, 1, 1] and np.all(recs["max_bin"] == 0)
        assert np.array_equal(recs["max_bin_seen"], recs["n_seen"])


def test_two_calls_give_the_same_bytes(genome_case):
    org, pos, bits = genome_case
    maps = [sm.pack(b, pad_ones=True) for b in bits[2:]]
    a, b = seen_coverage(org, pos, maps, n_orgs=6), seen_coverage(org, pos, maps, n_orgs=6)
    assert a.tobytes() == b.tobytes() and a["n_seen"].sum() > 0
    x, y = seen_coverage_bins(org, pos, maps, n_orgs=6), seen_coverage_bins(org, pos, maps, n_orgs=6)
    assert all(p.tobytes() == q.tobytes() for p, q in zip(x, y))


# ------------------------------------------------------------------ 2. few entries
@pytest.mark.parametrize("n_entries", [0, 1, 31, 127, 129])
def test_few_entries_with_every_padding_bit_set(n_entries):
    o = np.arange(n_entries)
    org, pos = (o * 3 // max(n_entries, 1)).astype(np.uint32), (o * 977 % 5000).astype(np.uint32)
    order = np.lexsort((pos, org))
    recs = check_both_orders(org[order], pos[order], some_bits(n_entries, n_entries), 1000, 4, "%d entries" % n_entries)
    assert recs["n_probes"][1].sum() == n_entries == recs["n_seen"][1].sum() and recs["n_seen"][0].sum() == 0
    assert not any(recs[:, 3].tobytes())  # organism 3 has no entry: all zero
    full = np.full(sm.seen_bytes(n_entries), 255, np.uint8)
    assert seen_coverage(org, pos, [full], n_orgs=4)["n_seen"].sum() == n_entries  # padding bits are ignored


# ------------------------------------------------------------------ 3. runs of one bin across a tile's and a span's edge
def test_runs_of_one_bin_across_the_edges_of_tiles_and_spans():
    runs, at = [], 0
    for start, length in ((40, 63), (TILE * 3 - 20, 64), (TILE * 6 - 1, 65), (SPAN - 30, 5000), (SPAN * 7 - 62, 63), (SPAN * 8 - 1, 64),
                          (SPAN * 9 - 64, 65), (SPAN * 10, 64)):
        assert start >= at
        runs += [1] * (start - at) + [length]  # single-entry bins up to `start`, then the run
        at = start + length
    runs += [1] * 77
    bin_of = np.repeat(np.arange(len(runs)), runs)  # ascending: the entries are in order
    org, pos = (bin_of // 4000).astype(np.uint32), (bin_of % 4000 * 1000 + 17).astype(np.uint32)
    rng = np.random.default_rng(3)
    run_entries = np.repeat(np.asarray(runs) > 1, runs)
    bits = some_bits(org.size, 3, [run_entries, ~run_entries, run_entries & (rng.random(org.size) < 0.9)])
    n_orgs = int(org.max()) + 1
    recs = check_both_orders(org, pos, bits, 1000, n_orgs, "runs")
    assert recs["max_bin_seen"][5].max() == 5000 and recs["max_bin_seen"][6].max() == 1


def test_two_organisms_whose_entries_alternate():
    o = np.arange(3001)
    org, pos = (o & 1).astype(np.uint32), (o // 2 * 7).astype(np.uint32)
    for width in (1, 100, 1000):
        check(org, pos, [sm.pack(b, pad_ones=True) for b in some_bits(o.size, 5, [org == 1])], width, 2, "alternating, W = %d" % width)


# ------------------------------------------------------------------ 4. many organisms; one heavy bin
def test_70000_organisms_of_one_or_two_entries():
    rng = np.random.default_rng(70000)
    org = np.sort(np.concatenate([np.arange(70000), rng.choice(70000, 35000, replace=False)])).astype(np.uint32)
    pos = rng.integers(0, 5000, org.size).astype(np.uint32)
    bits = [rng.random(org.size) < 0.5, np.ones(org.size, bool)]
    recs = check_both_orders(org, pos, bits, 1000, 70001, "70 000 organisms", model=cm.coverage_literal)
    assert recs["n_probes"][0].max() == 2 and recs["n_probes"][0][:70000].min() == 1 and recs["n_probes"][0][70000] == 0


def test_a_bin_of_70000_seen_entries():
    n = 70000 + 300
    org = np.zeros(n, np.uint32)
    pos = np.concatenate([np.arange(300) * 10, np.full(70000, 5123)]).astype(np.uint32)
    order = np.lexsort((pos, org))
    recs = check_both_orders(org[order], pos[order], [np.ones(n, bool), pos[order] == 5123], 1000, 1, "a heavy bin")
    assert recs[1][0]["max_bin_seen"] == 70000 and recs[1][0]["max_bin"] == 5 and recs[0][0]["n_seen"] == 70300


# ------------------------------------------------------------------ 5. the extremes of position and width
def test_the_largest_position_and_the_cap_on_bins():
    org = np.array([0, 0, 1], np.uint32)
    pos = np.array([5, (1 << 32) - 1, 1 << 20], np.uint32)
    maps = [sm.pack([0, 1, 1], pad_ones=True)]
    recs = check(org, pos, maps, 1 << 20, 2, "pos = 2^32 - 1, W = 2^20")
    assert recs[0][0]["span_bins"] == 4096 and recs[0][0]["max_bin"] == 4095 and recs[0][0]["max_gap"] == 1
    # pos = 2^28 with W = 1: B = 2^28 + 1, one bin too many.  Nothing is written (and nothing of that size is allocated)
    org = np.zeros(3, np.uint32)
    pos = np.array([0, 1 << 28, 0], np.uint32)
    lib = _lib.load()
    ptrs = (C.c_void_p * 1)(maps[0].ctypes.data)
    out = np.full((1, 1, 8), 0xABABABAB, np.uint32)
    args = (0, org.ctypes.data_as(C.c_void_p), pos.ctypes.data_as(C.c_void_p), 3, 1)
    assert lib.kid_seen_coverage(*args, 1, ptrs, 1, out.ctypes.data_as(C.c_void_p)) == -1 and np.all(out == 0xABABABAB)  # KID_ERR_ARG
    with pytest.raises(KidError):
        seen_coverage(org, pos, maps, bin_width=1)
    base, n_bins = np.full(2, 77, np.uint64), C.c_uint64(77)
    assert lib.kid_seen_coverage_bins(*args, 1, ptrs, 1, base.ctypes.data_as(C.c_void_p), None, None, 0, C.byref(n_bins)) == -1
    assert np.all(base == 77) and n_bins.value == 77
    pos[1] = (1 << 28) - 1  # exactly the cap: the sizing call, which allocates nothing of that size, says so
    assert lib.kid_seen_coverage_bins(*args, 1, ptrs, 1, base.ctypes.data_as(C.c_void_p), None, None, 0, C.byref(n_bins)) == 0
    assert n_bins.value == 1 << 28 == _lib.KID_COVERAGE_MAX_BINS and base.tolist() == [0, 1 << 28]


# ------------------------------------------------------------------ 6. bitmap counts
@pytest.fixture(scope="module")
def cohort():
    """64 bitmaps, from empty to full, over the entries of three organisms across two spans"""
    n = 2 * SPAN + 133
    o = np.arange(n)
    org, pos = (o * 3 // n).astype(np.uint32), (o * 37 % 90000).astype(np.uint32)
    order = np.lexsort((pos, org))
    org, pos = org[order], pos[order]
    rng = np.random.default_rng(64)
    maps = [sm.pack(rng.random(n) < d, pad_ones=bool(i & 1)) for i, d in enumerate(np.linspace(0.0, 1.0, 64))]
    return org, pos, maps, cm.coverage(org, pos, maps, 1000, 3)


@pytest.mark.parametrize("n", [1, 2, 3, 64])
def test_bitmap_counts(cohort, n):
    org, pos, maps, exp = cohort
    pick = list(range(64)) if n == 64 else [40, 9, 40][:n]  # (n = 3: one bitmap named twice)
    got = seen_coverage(org, pos, [maps[i] for i in pick], n_orgs=3)
    same_records(got, exp[pick], "n = %d" % n)
    if n == 3:
        assert got[0].tobytes() == got[2].tobytes()
    if n == 64:
        assert got["n_seen"][0].sum() == 0 and got["n_seen"][63].sum() == org.size
        base, probes, seen = seen_coverage_bins(org, pos, [maps[i] for i in pick], n_orgs=3)
        e_base, e_probes, e_seen = cm.bins_model(org, pos, maps, 1000, 3)
        assert np.array_equal(base, e_base) and np.array_equal(probes, e_probes) and np.array_equal(seen, e_seen)


# ------------------------------------------------------------------ 7. the per-bin call's sizes
def test_the_sizing_call_and_too_little_room(cohort):
    org, pos, maps, exp = cohort
    lib = _lib.load()
    ptrs = (C.c_void_p * 2)(maps[20].ctypes.data, maps[50].ctypes.data)
    args = (0, org.ctypes.data_as(C.c_void_p), pos.ctypes.data_as(C.c_void_p), org.size, 3, 1000, ptrs, 2)
    e_base, e_probes, e_seen = cm.bins_model(org, pos, [maps[20], maps[50]], 1000, 3)
    B = int(e_base[-1])
    base, n_bins = np.zeros(4, np.uint64), C.c_uint64(0)
    assert lib.kid_seen_coverage_bins(*args, base.ctypes.data_as(C.c_void_p), None, None, 0, C.byref(n_bins)) == 0
    assert n_bins.value == B and np.array_equal(base, e_base)
    probes, seen = np.full(B + 1, 0xCDCDCDCD, np.uint32), np.full(2 * B + 1, 0xCDCDCDCD, np.uint32)
    p, s = probes.ctypes.data_as(C.c_void_p), seen.ctypes.data_as(C.c_void_p)
    base2, n2 = np.full(4, 5, np.uint64), C.c_uint64(5)
    for cap in (B - 1, 0):
        assert lib.kid_seen_coverage_bins(*args, base2.ctypes.data_as(C.c_void_p), p, s, cap, C.byref(n2)) == -1  # KID_ERR_ARG
        assert np.all(probes == 0xCDCDCDCD) and np.all(seen == 0xCDCDCDCD) and np.all(base2 == 5) and n2.value == 5
    assert lib.kid_seen_coverage_bins(*args, base2.ctypes.data_as(C.c_void_p), p, None, B, C.byref(n2)) == -1  # one array without the other
    assert lib.kid_seen_coverage_bins(*args, base2.ctypes.data_as(C.c_void_p), None, None, B, C.byref(n2)) == -1  # no array, yet room
    assert lib.kid_seen_coverage_bins(*args, base2.ctypes.data_as(C.c_void_p), p, s, B, C.byref(n2)) == 0
    assert n2.value == B and np.array_equal(base2, e_base) and np.array_equal(probes[:B], e_probes) and probes[B] == 0xCDCDCDCD
    assert np.array_equal(seen[:2 * B].reshape(2, B), e_seen) and seen[2 * B] == 0xCDCDCDCD


# ------------------------------------------------------------------ 8. errors
def test_argument_errors_write_nothing(cohort):
    org, pos, maps, exp = cohort
    lib = _lib.load()
    ok = [m.ctypes.data for m in maps]
    untouched = np.full((65, 3, 8), 0xABABABAB, np.uint32)
    o, p = org.ctypes.data_as(C.c_void_p), pos.ctypes.data_as(C.c_void_p)
    bad_org = org.copy()
    bad_org[org.size // 2] = 3  # = n_orgs
    cases = [("n = 0", o, p, 1000, ok[:1], 0), ("n = 65", o, p, 1000, ok + ok[:1], 65), ("n = -1", o, p, 1000, ok[:1], -1),
             ("a null bitmap", o, p, 1000, [ok[0], None, ok[2]], 3), ("bin_width = 0", o, p, 0, ok[:2], 2), ("org is null", None, p, 1000, ok[:2], 2),
             ("pos is null", o, None, 1000, ok[:2], 2), ("an org = n_orgs", bad_org.ctypes.data_as(C.c_void_p), p, 1000, ok[:2], 2)]
    for what, org_p, pos_p, width, bitmaps, n in cases:
        out = untouched.copy()
        ptrs = (C.c_void_p * len(bitmaps))(*bitmaps)
        assert lib.kid_seen_coverage(0, org_p, pos_p, org.size, 3, width, ptrs, n, out.ctypes.data_as(C.c_void_p)) == -1, what  # KID_ERR_ARG
        assert np.array_equal(out, untouched), what
        base, n_bins = np.full(4, 9, np.uint64), C.c_uint64(9)
        assert lib.kid_seen_coverage_bins(0, org_p, pos_p, org.size, 3, width, ptrs, n, base.ctypes.data_as(C.c_void_p), None, None, 0,
                                          C.byref(n_bins)) == -1, what
        assert np.all(base == 9) and n_bins.value == 9, what
    ptrs = (C.c_void_p * 2)(*ok[:2])
    out = untouched.copy()
    assert lib.kid_seen_coverage(0, o, p, org.size, 3, 1000, None, 2, out.ctypes.data_as(C.c_void_p)) == -1
    assert lib.kid_seen_coverage(0, o, p, org.size, 3, 1000, ptrs, 2, None) == -1 and np.array_equal(out, untouched)
    n_bins = C.c_uint64(9)
    assert lib.kid_seen_coverage_bins(0, o, p, org.size, 3, 1000, ptrs, 2, None, None, None, 0, C.byref(n_bins)) == -1 and n_bins.value == 9
    with pytest.raises(KidError):
        seen_coverage(bad_org, pos, maps[:2], n_orgs=3)
    with pytest.raises(ValueError):
        seen_coverage(org, pos, [maps[0][:-16]])
    with pytest.raises(ValueError):
        seen_coverage(org, pos[:-1], maps[:1])
    same_records(seen_coverage(org, pos, maps[:2]), exp[:2], "after the errors")


# ------------------------------------------------------------------ 9. a live sample
def test_a_live_sample_against_its_exported_bitmap():
    parent, cum, keys, targets = small_db(2e-4)
    db = KmerDB(keys, targets, parent, k=30, log2_slots=18)
    s = db.sample()
    s.classify(synth.reads(cum, parent, 600, 150, read_seed=11), synth.fixed_offsets(600, 150))
    g, u = s.end()
    org = (targets % 37).astype(np.uint32)  # any sites will do: the entries of a target in a few organisms
    pos = (np.arange(targets.size) * 13 % 200000).astype(np.uint32)
    live = db.seen_coverage([s], org, pos)
    bitmap = s.seen_export(0, s.seen_bytes())
    both = db.seen_coverage([bitmap, s], org, pos, bin_width=1000)
    assert live.shape == (1, 37) and live[0].tobytes() == both[0].tobytes() == both[1].tobytes()
    same_records(seen_coverage(org, pos, [bitmap]), cm.coverage(org, pos, [bitmap], 1000, 37), "a sample's bitmap")
    assert live.tobytes() == seen_coverage(org, pos, [bitmap]).tobytes() and live["n_seen"].sum() == u.sum() > 0
    with pytest.raises(ValueError):
        db.seen_coverage([s], org[:-1], pos[:-1])
    g2, u2 = s.end()  # the sample was not touched
    assert np.array_equal(u2, u)
    s.close(), db.close()
