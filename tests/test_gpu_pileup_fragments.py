"""kid_pileup_add_fragments and its device form: kid_fragment_locus records piled up per genome bin, against the model
(fragment_walk of tests/read_fragment_loci_model.py over the geometry of tests/read_pileup_model.py) on the small table of
tests/read_pileup_cases.py; the worked case of include/kmer_id_amd.h; paired_only; a record that fails one placement
condition changes nothing; read records and fragment records added to one pileup sum; export and merge."""
import numpy as np
import pytest

import read_fragment_loci_model as fm
import read_pileup_cases as pc
import read_pileup_model as pm
from helpers import DeviceBatch
from kmer_id_amd import FRAGMENT_LOCUS_DTYPE, KmerDB, _lib
from read_calls import status
from read_support_cases import random_keys

pytestmark = pytest.mark.gpu

X = 991  # organism 3's last entry lies at 990: ten bins of 100 bases
RULES = [(2, 1, False), (1, 0, True), (3, 2, False)]


class DeviceRecords(DeviceBatch):
    """kid_fragment_locus records resident in HBM"""

    def __init__(self, recs):
        self.lib, self.bufs, self.n = _lib.load(), [], recs.size
        recs = np.ascontiguousarray(recs, FRAGMENT_LOCUS_DTYPE)
        self.ptr = self.dev(max(recs.nbytes, 16), recs if recs.size else None).value


@pytest.fixture(scope="module")
def db():
    keys = random_keys(np.random.default_rng([5, pc.N_SMALL]), pc.N_SMALL)
    d = KmerDB(keys, (1 + np.arange(pc.N_SMALL) % 7).astype(np.uint32), np.ones(8, np.int32), k=pc.K, log2_slots=12)
    d.set_sites(*pc.small(X))
    yield d
    d.close()


def rec(**kw):
    r = np.zeros(1, FRAGMENT_LOCUS_DTYPE)
    for f, v in kw.items():
        r[f] = v
    return r


def random_records(n, seed):
    """records as a caller may hand them in: orgs with and without bins and beyond the table, every value of mates and more,
    intervals inside the genome, across its end, up to 2^32 - 1 and with lo above hi"""
    rng = np.random.default_rng([seed, n])
    r = np.zeros(n, FRAGMENT_LOCUS_DTYPE)
    r["org"] = np.array([0, 1, 2, 3, 3, 3, 3, 4, 2 ** 24 - 1, 2 ** 32 - 1], np.uint32)[rng.integers(0, 10, n)]
    r["mates"] = rng.integers(0, 5, n)
    r["n_chain"], r["n_other"] = rng.integers(0, 7, n), rng.integers(0, 7, n)
    lo = rng.integers(0, 1200, n)
    hi = lo + rng.integers(-40, 700, n)
    far = rng.integers(0, 20, n) == 0
    hi[far] = 2 ** 32 - 1
    r["lo"], r["hi"] = lo, np.maximum(hi, 0)
    r["orient"], r["n_hits"] = rng.integers(0, 2, n), rng.integers(0, 50, n)
    return r


def expected(recs, w, rule, more=None):
    """-> bin_base, starts, depth, n_placed of the records under rule = (min_chain, min_margin, paired_only); more: read
    records (LOCUS_DTYPE) walked into the same dictionaries under the same (min_chain, min_margin)"""
    org, pos = pc.small(X)
    span, bin_base = pm.geometry(org, pos, w)
    s, d, n_placed = fm.fragment_walk(recs, w, span, *rule)
    if more is not None:
        s, d, n_more = pm.walk(more, org, pos, pc.K, w, span, rule[0], rule[1], s, d)
        n_placed += n_more
    return bin_base, pm.dense(s, span, bin_base), pm.dense(d, span, bin_base), n_placed


def same(p, exp, n_records, what=""):
    base, starts, depth = p.bins()
    assert np.array_equal(base, exp[0]) and np.array_equal(starts, exp[1]) and np.array_equal(depth, exp[2]), what
    assert p.counts() == (n_records, exp[3]), what


@pytest.mark.parametrize("w", [1, 7, 100])
def test_host_and_device_forms_equal_the_model(db, w):
    recs = random_records(5000, w)
    for rule in RULES:
        exp = expected(recs, w, rule)
        assert 200 < exp[3] < 3000
        with db.pileup(w) as p:
            p.add_fragments(recs, *rule)
            same(p, exp, recs.size, "host form, %s" % (rule,))
        with db.pileup(w) as p, DeviceRecords(recs) as d:  # in two calls, the second of a number that is no multiple of a wave
            p.add_fragments_device(d.ptr, 3001, *rule)
            p.add_fragments_device(d.ptr + 64 * 3001, recs.size - 3001, *rule)
            same(p, exp, recs.size, "device form, %s" % (rule,))
            ms, calls, n = p.time()
            assert ms > 0 and (calls, n) == (2, recs.size)


def test_the_worked_case(db):
    recs = np.concatenate([rec(org=3, mates=3, n_chain=3, n_other=1, lo=100, hi=429), rec(org=3, mates=1, n_chain=2, lo=100, hi=159),
                           rec(org=3, mates=3, n_chain=2, n_other=2, lo=100, hi=429), rec(org=3, lo=100, hi=429, n_chain=5)])
    with db.pileup(100) as p:
        p.add_fragments(recs, 2, 1)
        base, starts, depth = p.bins()
        a = int(base[3])
        assert int(base[4]) - a == 10
        assert starts[a:a + 10].tolist() == [0, 2, 0, 0, 0, 0, 0, 0, 0, 0] and depth[a:a + 10].tolist() == [0, 2, 1, 1, 1, 0, 0, 0, 0, 0]
        assert p.counts() == (4, 2) and not starts[:a].any() and not depth[:a].any()
        p.reset()
        p.add_fragments(recs, 2, 1, paired_only=True)
        base, starts, depth = p.bins()
        assert starts[a:a + 10].tolist() == [0, 1, 0, 0, 0, 0, 0, 0, 0, 0] and depth[a:a + 10].tolist() == [0, 1, 1, 1, 1, 0, 0, 0, 0, 0]
        assert p.counts() == (4, 1)


def test_a_record_that_fails_one_condition_changes_nothing(db):
    good = dict(org=3, mates=3, n_chain=4, n_other=1, lo=250, hi=700)
    bad = [dict(good, mates=0), dict(good, mates=4), dict(good, mates=2 ** 32 - 1), dict(good, n_chain=2), dict(good, n_other=2),
           dict(good, n_other=9), dict(good, org=2), dict(good, org=4), dict(good, org=2 ** 32 - 1), dict(good, lo=701), dict(good, lo=2 ** 32 - 1, hi=0)]
    recs = np.concatenate([rec(**b) for b in bad])
    with db.pileup(7) as p:
        p.add_fragments(recs, 3, 3)
        starts, steps = p.export()
        assert not starts.any() and not steps.any() and p.counts() == (len(bad), 0)
        p.add_fragments(rec(**dict(good, mates=1)), 3, 3, paired_only=True)  # paired_only is one more
        assert p.counts() == (len(bad) + 1, 0)
        p.add_fragments(rec(**good), 3, 3, paired_only=True)
        starts, steps = p.export()
        assert p.counts() == (len(bad) + 2, 1) and int(starts.sum()) == 1 and np.flatnonzero(steps).size == 2


def test_read_records_and_fragment_records_sum_in_one_pileup(db):
    w, rule = 7, (2, 1, False)
    loci = pc.small_case(7)[0][:3000]
    recs = random_records(3000, 9)
    org, pos = pc.small(X)
    loci = loci[loci["entry_first"] < org.size]
    exp = expected(recs, w, rule, more=loci)
    alone = expected(recs, w, rule)
    assert exp[3] > alone[3] > 0
    with db.pileup(w) as p:
        p.add(loci[:1000], 2, 1)
        p.add_fragments(recs, *rule)
        p.add(loci[1000:], 2, 1)
        same(p, exp, loci.size + recs.size)


def test_export_of_two_merged_into_a_third(db):
    w, rule = 7, (1, 0, False)
    recs = random_records(4000, 3)
    exp = expected(recs, w, rule)
    with db.pileup(w) as a, db.pileup(w) as b, db.pileup(w) as c:
        a.add_fragments(recs[:1500], *rule)
        b.add_fragments(recs[1500:], *rule)
        for part in (a, b):
            starts, steps = part.export()
            c.merge(starts, steps, *part.counts())
        same(c, exp, recs.size)
        c.add_fragments(recs[:10], *rule)  # and goes on counting
        assert c.counts()[0] == recs.size + 10


def test_statuses_are_those_of_add(db):
    recs = random_records(10, 1)
    with db.pileup(7) as p:
        assert status(lambda: p.add_fragments(recs, 0, 0)) == -1  # min_chain = 0
        assert status(lambda: p.add_fragments_device(0, 5, 2, 1)) == -1  # a null pointer with records
        p.add_fragments(recs[:0], 2, 1)
        p.add_fragments_device(0, 0, 2, 1)
        assert p.counts() == (0, 0)
        org, pos = pc.small(X)
        db.set_sites(org, pos)  # the sites set again: the pileup's geometry is stale
        assert status(lambda: p.add_fragments(recs, 2, 1)) == -10
        assert p.counts() == (0, 0)
