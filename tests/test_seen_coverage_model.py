"""The two models of tests/seen_coverage_model.py against the rule's worked case and its corner cases, and against each
other on seeded inputs (entry order must not matter)."""
import numpy as np

import seen_coverage_model as cm
import shared_kmers_model as sm

MODELS = (cm.coverage, cm.coverage_literal)


def record(org, pos, seen_entries, bin_width, n_orgs, g=0):
    """the record of organism g under both models, which must agree"""
    bits = np.zeros(len(org), bool)
    bits[list(seen_entries)] = True
    recs = [m(np.asarray(org, np.uint32), np.asarray(pos, np.uint32), [sm.pack(bits, pad_ones=True)], bin_width, n_orgs) for m in MODELS]
    assert recs[0].tobytes() == recs[1].tobytes()
    return {name: int(recs[0][0, g][name]) for name in cm.FIELDS}


def test_the_worked_case_field_by_field():
    pos = [0, 10, 1500, 3999, 7000, 7001, 12000]
    r = record([0] * 7, pos, [1, 4, 5], 1000, 2)
    assert r == dict(n_probes=7, n_seen=3, span_bins=13, bins=5, bins_seen=2, max_gap=2, max_bin_seen=2, max_bin=7)
    # the organism without an entry: all zero
    assert record([0] * 7, pos, [1, 4, 5], 1000, 2, g=1) == dict.fromkeys(cm.FIELDS, 0)


def test_ties_for_max_bin_go_to_the_lowest_bin():
    pos = [5000, 5001, 2000, 2001, 9000, 9001, 100]
    r = record([0] * 7, pos, [0, 1, 2, 3, 4, 5, 6], 1000, 1)
    assert (r["max_bin_seen"], r["max_bin"]) == (2, 2)


def test_gaps_at_the_start_at_the_end_and_over_everything():
    pos = [0, 1000, 2000, 5000, 6000, 7000, 8000]  # occupied bins 0 1 2 5 6 7 8
    assert record([0] * 7, pos, [3], 1000, 1)["max_gap"] == 3           # bins 0..2 in front of it, 6..8 behind
    assert record([0] * 7, pos, [2, 3], 1000, 1)["max_gap"] == 3        # at the end: 6, 7, 8
    assert record([0] * 7, pos, [3, 4, 5, 6], 1000, 1)["max_gap"] == 3  # at the start: 0, 1, 2
    assert record([0] * 7, pos, [0, 6], 1000, 1)["max_gap"] == 5        # bins 3 and 4 are unoccupied and transparent
    r = record([0] * 7, pos, [], 1000, 1)
    assert r == dict(n_probes=7, n_seen=0, span_bins=9, bins=7, bins_seen=0, max_gap=7, max_bin_seen=0, max_bin=0)
    assert record([0] * 7, pos, range(7), 1000, 1)["max_gap"] == 0


def test_an_organism_with_one_entry():
    assert record([1], [4321], [0], 1000, 2, g=1) == dict(n_probes=1, n_seen=1, span_bins=5, bins=1, bins_seen=1, max_gap=0, max_bin_seen=1,
                                                          max_bin=4)
    assert record([1], [4321], [], 1000, 2, g=1) == dict(n_probes=1, n_seen=0, span_bins=5, bins=1, bins_seen=0, max_gap=1, max_bin_seen=0,
                                                         max_bin=0)


def test_the_models_agree_on_seeded_cases_and_under_a_shuffle():
    rng = np.random.default_rng(20261019)
    for case in range(6):
        n, n_orgs, width = int(rng.integers(1, 900)), int(rng.integers(1, 7)), int(rng.choice([1, 7, 100, 1000, 10 ** 6]))
        org = np.sort(rng.integers(0, n_orgs, n)).astype(np.uint32)
        pos = rng.integers(0, 3000, n).astype(np.uint32)
        maps = [sm.pack(rng.random(n) < p, pad_ones=bool(case & 1)) for p in (0.0, 0.03, 0.5, 1.0)]
        a, b = cm.coverage(org, pos, maps, width, n_orgs), cm.coverage_literal(org, pos, maps, width, n_orgs)
        assert a.tobytes() == b.tobytes(), case
        assert int(a["n_probes"][0].sum()) == n and np.all(a["n_seen"][3] == a["n_probes"][3]) and np.all(a["max_gap"][0] == a["bins"][0])
        perm = rng.permutation(n)
        shuffled = [sm.pack(sm.bits_of(m, n)[perm], pad_ones=True) for m in maps]
        for model in MODELS:
            assert model(org[perm], pos[perm], shuffled, width, n_orgs).tobytes() == a.tobytes(), case


def test_the_printed_lines():
    recs = cm.coverage(np.array([0, 0, 2], np.uint32), np.array([0, 1000, 5], np.uint32), [sm.pack([1, 0, 1]), sm.pack([0, 0, 0])], 1000, 3)
    assert cm.cli_lines(["a", "b"], recs) == b"#0\ta\t2\n#1\tb\t0\n0,0,2,1,2,2,1,1,1,0\n0,2,1,1,1,1,1,0,1,0\n"
    assert cm.cli_lines(["a", "b"], recs, 0).count(b"\n") == 2 + 6
    base, probes, seen = cm.bins_model(np.array([0, 0, 2], np.uint32), np.array([0, 1000, 5], np.uint32), [sm.pack([1, 0, 1])], 1000, 3)
    assert base.tolist() == [0, 2, 2, 3] and probes.tolist() == [1, 1, 1] and seen.tolist() == [[1, 0, 1]]
    assert cm.cli_bins_lines(["a"], base, probes, seen, 0) == b"#0\ta\t2\n0,0,0,1,1\n0,0,1,1,0\n"
