"""kid_pileup_add_device, kid_pileup_summary, _bins, _export, _merge, _reset, _counts and _time on the synthetic records of
tests/read_pileup_cases.py against the model (tests/read_pileup_model.py): the site table of the loci tests (n_orgs = 2^24,
positions up to 2^31 - 1) at three widths, and refused at W = 1; a table of four organisms with span_bins 1, 1, 0 and 300
whose one-bin neighbours would show a step that leaks past a sentinel; records at every value the rule changes its mind at;
100 000 records in one bin and 100 000 spread out; lists of 0 to 257 records; tables whose B + n_orgs sits at every edge of
the scan's tile.  Every output is taken through the C ABI into arrays with a guard behind them."""
import ctypes as C

import numpy as np
import pytest

import read_loci_cases as lc
import read_loci_model as lm
import read_pileup_cases as pc
import read_pileup_model as pm
from helpers import DeviceBatch
from kmer_id_amd import PILEUP_DTYPE, KmerDB, _lib
from read_calls import status
from read_support_cases import random_keys

pytestmark = pytest.mark.gpu

CANARY, GUARD = 0xA5A5A5A5, 64


class DeviceRecords(DeviceBatch):
    """kid_locus records resident in HBM"""

    def __init__(self, loci):
        self.lib, self.bufs, self.n = _lib.load(), [], loci.size
        loci = np.ascontiguousarray(loci, lm.LOCUS_DTYPE)
        self.ptr = self.dev(max(loci.nbytes, 16), loci if loci.size else None).value

    def at(self, first):
        return self.ptr + lm.LOCUS_DTYPE.itemsize * first


@pytest.fixture(scope="module")
def big_db():
    c = lc.case()
    d = KmerDB(c.keys, c.targets, np.ones(8, np.int32), k=pc.K, log2_slots=15)
    d.set_sites(*pc.big())
    yield d
    d.close()


@pytest.fixture(scope="module")
def small_db():
    keys = random_keys(np.random.default_rng([5, pc.N_SMALL]), pc.N_SMALL)
    d = KmerDB(keys, (1 + np.arange(pc.N_SMALL) % 7).astype(np.uint32), np.ones(8, np.int32), k=pc.K, log2_slots=12)
    assert d.info.n_entries == pc.N_SMALL
    yield d
    d.close()


def guarded(n_words):
    return np.full(n_words + GUARD, CANARY, np.uint32)


def untouched(a, n_words, what):
    assert np.all(a[n_words:] == CANARY), "a write behind the end of " + what
    return a[:n_words]


def outputs(p):
    """-> records, bin_base, starts, depth, export's starts, export's steps, (n_records, n_placed): every array through the
    C ABI with a guard behind it"""
    lib, h, no, nb = p._lib, p._h, p.n_orgs, p.n_bins
    recs, base = guarded(no * 12), guarded((no + 1) * 2)
    starts, depth, x_starts, x_steps = guarded(nb), guarded(nb), guarded(nb), guarded(nb + no)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    _lib.check(lib.kid_pileup_summary(h, ptr(recs)))
    _lib.check(lib.kid_pileup_bins(h, ptr(base), ptr(starts), ptr(depth), nb))
    _lib.check(lib.kid_pileup_export(h, ptr(x_starts), ptr(x_steps)))
    return (untouched(recs, no * 12, "summary").view(PILEUP_DTYPE), untouched(base, (no + 1) * 2, "bin_base").view(np.uint64),
            untouched(starts, nb, "starts"), untouched(depth, nb, "depth"), untouched(x_starts, nb, "export's starts"),
            untouched(x_steps, nb + no, "export's steps"), p.counts())


def check(p, exp, what=""):
    recs, base, starts, depth, x_starts, x_steps, counts = out = outputs(p)
    assert np.array_equal(base, exp.bin_base), what
    for name, got, want in (("starts", starts, exp.starts), ("depth", depth, exp.depth), ("export's starts", x_starts, exp.starts),
                            ("steps", x_steps, exp.steps)):
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "%s: %s[%d]: got %d, the model %d" % (what, name, bad[0], got[bad[0]], want[bad[0]])
    if not np.array_equal(recs.view(np.uint32), exp.records.view(np.uint32)):  # (the padding word included: it is zero)
        for f in PILEUP_DTYPE.names:
            bad = np.flatnonzero(recs[f] != exp.records[f])
            assert bad.size == 0, "%s: organism %d: %s: got %s, the model %s" % (what, bad[0], f, recs[bad[0]], exp.records[bad[0]])
        raise AssertionError(what + ": the padding of a record is not zero")
    assert counts == (exp.n_records, exp.n_placed), what
    return out


def same_bytes(a, b):
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:6], b[:6])) and a[6] == b[6]


def add_all(p, d, rule=pc.RULE, first=0, n=None, stream=0):
    p.add_device(d.at(first), d.n - first if n is None else n, rule[0], rule[1], stream=stream)


def test_the_record_is_the_models():
    assert PILEUP_DTYPE == pm.PILEUP_DTYPE and PILEUP_DTYPE.itemsize == 48 == 12 * 4


@pytest.mark.parametrize("w", pc.BIG_WIDTHS)
def test_the_loci_tests_table(big_db, w):
    loci, exp = pc.big_case(w)
    with big_db.pileup(w) as p, DeviceRecords(loci) as d, DeviceRecords(loci[np.random.default_rng(w).permutation(loci.size)]) as ds:
        assert p.n_orgs == 2 ** 24 and p.n_bins == int(exp.bin_base[-1]) and p.bin_width == w
        add_all(p, d)
        check(p, exp, "W = %d" % w)
        one = p.export()
        p.reset()
        add_all(p, ds)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(one, p.export())), "the list shuffled"


def test_more_than_the_cap_of_bins_is_refused(big_db):
    free0 = big_db_free(big_db)
    assert status(lambda: big_db.pileup(1)) == -1  # KID_ERR_ARG: B > 2^28
    assert status(lambda: big_db.pileup(0)) == -1
    assert big_db_free(big_db) >= free0 - (64 << 20)  # nothing is left allocated


def big_db_free(db):
    free, total = C.c_uint64(0), C.c_uint64(0)
    _lib.check(db._lib.kid_device_mem_info(0, C.byref(free), C.byref(total)))
    return free.value


@pytest.mark.parametrize("w", pc.SMALL_WIDTHS)
def test_the_second_table_in_any_order_and_any_split(small_db, w):
    small_db.set_sites(*pc.small())
    loci, exp = pc.small_case(w)
    rng = np.random.default_rng(w)
    with small_db.pileup(w) as p, DeviceRecords(loci) as d, DeviceRecords(loci[rng.permutation(loci.size)]) as ds:
        assert (p.n_orgs, p.n_bins) == (4, 302 if w == 1 else 45)
        add_all(p, d)
        whole = check(p, exp, "W = %d" % w)
        assert whole[0]["span_bins"].tolist() == [1, 1, 0, 300 if w == 1 else 43]
        same_bytes(outputs(p), whole)  # a summary modifies nothing: a second one gives the same
        with small_db.pileup(w) as q:  # the list shuffled
            add_all(q, ds)
            same_bytes(outputs(q), whole)
        p.reset()
        assert p.counts() == (0, 0) and not any(a.any() for a in p.export()) and not p.bins()[2].any()
        assert p.summary()["n_placed"].sum() == 0 and p.summary()["max_gap"].tolist() == whole[0]["span_bins"].tolist()
        for a, b in ((0, 1), (1, 150), (150, loci.size)):  # three calls over cuts of the list, after a reset: a second run
            add_all(p, d, first=a, n=b - a)
        same_bytes(outputs(p), whole)


@pytest.mark.parametrize("n", pc.COUNTS)
def test_lists_of_few_records(small_db, n):
    small_db.set_sites(*pc.small())
    loci = pc.small_case(7)[0][:n]
    with small_db.pileup(7) as p, DeviceRecords(loci) as d:
        p.time()
        add_all(p, d)
        check(p, pc.Expected(loci, *pc.small(), 7), "%d records" % n)
        ms, calls, records = p.time()
        assert (calls, records) == ((1, n) if n else (0, 0)) and (ms > 0) == (n > 0)
        assert p.time() == (0, 0, 0)


@pytest.mark.parametrize("shape", ["hot_spot", "uniform"])
def test_100000_records(small_db, shape):
    small_db.set_sites(*pc.small())
    loci, exp = pc.shape_case(shape, 7)
    with small_db.pileup(7) as p, DeviceRecords(loci) as d:
        add_all(p, d, (2, 1))
        add_all(p, d, (2, 1), n=0)  # launches nothing, counts nothing
        check(p, exp, shape)
        assert p.time()[1:] == (1, loci.size)


@pytest.mark.parametrize("n_slots", pc.SCAN_SLOTS)
def test_the_edges_of_the_scan(small_db, n_slots):
    x = n_slots - 6
    org, pos = pc.scan_table(n_slots)
    small_db.set_sites(org, pos)
    loci, exp = pc.small_case(1, x, 200)
    with small_db.pileup(1) as p, DeviceRecords(loci) as d:
        assert p.n_bins + p.n_orgs == n_slots
        add_all(p, d)
        recs = check(p, exp, "%d slots" % n_slots)[0]
        assert recs[3]["bins_covered"] == x and recs[3]["max_depth"] >= 2  # a chain over the whole span: the carry crosses every tile


def test_two_streams_and_a_summary_with_nothing_between(small_db):
    import torch
    small_db.set_sites(*pc.small())
    uni, hot = pc.shape_case("uniform", 7)[0], pc.shape_case("hot_spot", 7)[0]
    both = np.concatenate([uni, hot])
    exp = pc.Expected(both, *pc.small(), 7, (2, 1))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with small_db.pileup(7) as p, DeviceRecords(uni) as d1, DeviceRecords(hot) as d2:
        _lib.check(d1.lib.kid_dev_sync(0))
        add_all(p, d1, (2, 1), stream=s1.cuda_stream)
        add_all(p, d2, (2, 1), stream=s2.cuda_stream)
        recs = p.summary()  # nothing here waits for the adds: the library has to
        assert recs.tobytes() == exp.records.tobytes()
        check(p, exp, "two streams")
        assert p.time()[1:] == (2, both.size)


def test_export_of_two_merged_into_a_third(small_db):
    small_db.set_sites(*pc.small())
    loci, exp = pc.small_case(7)
    half = loci.size // 2
    with small_db.pileup(7) as a, small_db.pileup(7) as b, small_db.pileup(7) as c, DeviceRecords(loci) as d:
        add_all(a, d, n=half)
        add_all(b, d, first=half)
        add_all(c, d, n=5)  # the third holds something of its own: merge adds
        for part in (a, b):
            c.merge(*part.export(), *part.counts())
        both = pc.Expected(np.concatenate([loci[:5], loci]), *pc.small(), 7)
        check(c, both, "merged")
        c.reset()
        for part in (a, b):
            c.merge(*part.export(), *part.counts())
        check(c, exp, "merged into an empty one")
        with pytest.raises(ValueError):
            c.merge(np.zeros(3, np.uint32), np.zeros(7, np.uint32), 0, 0)


def test_statuses_of_add_and_bins(small_db):
    small_db.set_sites(*pc.small())
    loci, exp = pc.small_case(7)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    with small_db.pileup(7) as p, DeviceRecords(loci) as d:
        lib, h = p._lib, p._h
        assert status(lambda: p.add_device(d.ptr, d.n, 0, 0)) == -1  # min_chain = 0
        assert status(lambda: p.add(loci, 0, 0)) == -1
        assert status(lambda: p.add_device(0, 5, 2, 1)) == -1        # a null pointer with records
        p.add_device(0, 0, 2, 1)                                     # n = 0: KID_OK, nothing launched
        assert p.counts() == (0, 0) and p.time()[1:] == (0, 0)
        p.add(loci, *pc.RULE)                                        # the host form
        check(p, exp, "host form")
        base, starts, depth = guarded(10), guarded(45), guarded(45)
        assert lib.kid_pileup_bins(h, ptr(base), None, None, 0) == 0  # the sizing call
        assert untouched(base, 10, "bin_base").view(np.uint64).tolist() == exp.bin_base.tolist() and base[8] == 45
        for args in ((ptr(base), ptr(starts), None, 45), (ptr(base), None, ptr(depth), 45), (ptr(base), ptr(starts), ptr(depth), 44),
                     (ptr(base), None, None, 45), (None, ptr(starts), ptr(depth), 45)):
            base[:] = CANARY
            assert lib.kid_pileup_bins(h, *args) == -1
            assert np.all(base == CANARY) and np.all(starts == CANARY) and np.all(depth == CANARY), "nothing is written"
        assert lib.kid_pileup_reset(None) == -1 and lib.kid_pileup_destroy(None) == -1 and lib.kid_pileup_summary(None, ptr(base)) == -1
        assert lib.kid_pileup_summary(h, None) == -1 and lib.kid_pileup_export(h, None, ptr(starts)) == -1
        assert lib.kid_pileup_counts(h, None, None) == 0
