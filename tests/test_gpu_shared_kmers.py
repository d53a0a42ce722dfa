"""K-mers shared between samples (kid_db_shared_kmers / kid_shared_kmers) against the numpy model of
tests/shared_kmers_model.py: exact equality of int64[n, n, ntar] for the entry counts and target layouts at the edges of
the kernel's words, quads, tiles and spans, for bitmaps that are empty, full (padding bits included), sparse and dense,
for 1 .. 64 bitmaps in host and in device memory, through both forms; two real samples; the argument errors."""
import ctypes as C

import numpy as np
import pytest

import shared_kmers_model as sm
from helpers import oracle_db, small_db
from kmer_id_amd import KidError, KmerDB, _lib, shared_kmers, synth
from read_calls import header_constant

pytestmark = pytest.mark.gpu

NTAR = 12
TILE = header_constant("kid_shared.hip.h", "KID_SHARED_TILE")
SPAN = TILE * header_constant("kid_shared.hip.h", "KID_SHARED_MIN_SPAN")  # entries a workgroup takes at least
SIZES = [1, 31, 32, 33, 127, 128, 129, 2047, 2048, 2049, 4097, SPAN - 1, SPAN, SPAN + 1, 70001]


def layout(name, n):
    """the targets of n entries"""
    o = np.arange(n)
    if name == "one":
        return np.full(n, 7, np.uint32)
    if name == "word-and-tile-edges":  # runs whose boundaries fall at the entries 31 / 32 / 33 and 2047 / 2048 / 2049 (and at the span's)
        edges = [31, 32, 33, 2047, 2048, 2049, SPAN - 1, SPAN, SPAN + 1]
        return (2 + np.searchsorted(edges, o, side="right") % 10).astype(np.uint32)
    if name == "no-runs":
        return (2 + o % 5).astype(np.uint32)
    if name == "three-tiles-then-mid-word":  # one run over three tiles and 13 bits of a word, then runs of 700
        return np.where(o < 3 * TILE + 13, 3, 4 + (o // 700) % 8).astype(np.uint32)
    raise KeyError(name)


LAYOUTS = ["one", "word-and-tile-edges", "no-runs", "three-tiles-then-mid-word"]


def bitmaps_for(n_entries, seed):
    """all zero, all ones with the padding bits, random at 0.01 and at 0.5 -- and the last one named twice"""
    rng = np.random.default_rng(seed)
    nbytes = sm.seen_bytes(n_entries)
    sparse = sm.pack(rng.random(n_entries) < 0.01)
    dense = rng.integers(0, 256, nbytes, dtype=np.uint8)  # (random padding bits too)
    return [np.zeros(nbytes, np.uint8), np.full(nbytes, 255, np.uint8), sparse, dense, dense]


def database(targets):
    rng = np.random.default_rng(targets.size)
    keys = rng.permutation(np.arange(1, 4 * targets.size + 1, dtype=np.uint64))[:targets.size] * np.uint64(0x9E3779B1)
    keys &= np.uint64((1 << 60) - 1)
    return KmerDB(keys, targets, np.ones(NTAR, np.int32), k=30, log2_slots=18)


def same(got, exp, what):
    assert got.dtype == np.int64 and got.shape == exp.shape, what
    bad = np.argwhere(got != exp)
    assert bad.size == 0, "%s: [%d, %d, %d]: got %d, the model %d" % ((what,) + tuple(bad[0]) + (int(got[tuple(bad[0])]), int(exp[tuple(bad[0])])))


class Device:
    """arrays in the memory of device 0"""

    def __init__(self):
        self.lib, self.bufs = _lib.load(), []

    def put(self, a):
        p = C.c_void_p()
        _lib.check(self.lib.kid_dev_alloc(0, a.nbytes, C.byref(p)))
        self.bufs.append(p)
        _lib.check(self.lib.kid_dev_upload(0, p, a.ctypes.data_as(C.c_void_p), a.nbytes))
        return p.value

    def close(self):
        for p in self.bufs:
            self.lib.kid_dev_free(0, p)


def raw_call(db, targets, bitmaps, on_device, n=None, shared=None):
    """both forms through the C ABI with the pointers as they are -> (status of the kid_db form, its matrix, status of the
    targets form, its matrix)"""
    lib = _lib.load()
    n = len(bitmaps) if n is None else n
    ptrs = (C.c_void_p * max(len(bitmaps), 1))(*bitmaps)
    out = []
    for form in ("db", "targets"):
        m = np.full((max(n, 0), max(n, 0), NTAR), -7, np.int64) if shared is None else shared
        if form == "db":
            rc = lib.kid_db_shared_kmers(db._h, ptrs, n, on_device, m.ctypes.data_as(C.c_void_p))
        else:
            rc = lib.kid_shared_kmers(0, targets.ctypes.data_as(C.c_void_p), targets.size, NTAR, ptrs, n, on_device, m.ctypes.data_as(C.c_void_p))
        out += [rc, m]
    return out


# ------------------------------------------------------------------ 1. sizes x layouts x bitmap contents, both forms
@pytest.mark.parametrize("name", LAYOUTS)
def test_every_size_and_layout_equals_the_model(name):
    for n_entries in SIZES:
        what = "%s, %d entries" % (name, n_entries)
        targets = layout(name, n_entries)
        maps = bitmaps_for(n_entries, n_entries)
        exp = sm.shared(targets, NTAR, maps)
        assert exp[1, 1].sum() == n_entries and np.array_equal(exp[3], exp[4])  # the full bitmap counts the entries alone
        got = shared_kmers(targets, NTAR, maps)
        same(got, exp, what + ", the targets form")
        assert np.array_equal(got, got.transpose(1, 0, 2)), what
        if n_entries in (33, 2049, 4097, SPAN + 1, 70001):  # (a table per size: a few of them)
            db = database(targets)
            first = db.shared_kmers(maps)
            same(first, exp, what + ", the kid_db form")
            assert db.shared_kmers(maps).tobytes() == first.tobytes() == got.tobytes(), what  # again: the same bytes
            db.close()


# ------------------------------------------------------------------ 2. sample counts, host and device pointers
@pytest.fixture(scope="module")
def cohort():
    """64 bitmaps over 4097 + 700 entries in runs and a database of them"""
    targets = layout("three-tiles-then-mid-word", 3 * TILE + 713)
    rng = np.random.default_rng(64)
    maps = [sm.pack(rng.random(targets.size) < d, pad_ones=bool(i & 1)) for i, d in enumerate(np.linspace(0.0, 1.0, 64))]
    db = database(targets)
    yield targets, maps, sm.shared(targets, NTAR, maps), db
    db.close()


@pytest.mark.parametrize("n", [1, 2, 3, 64])
def test_sample_counts_host_and_device(cohort, n):
    targets, maps, exp, db = cohort
    pick = list(range(64)) if n == 64 else [40, 9, 63][:n]
    want = exp[np.ix_(pick, pick)]
    dev = Device()
    try:
        for on_device in (0, 1):
            ptrs = [dev.put(maps[i]) if on_device else maps[i].ctypes.data for i in pick]
            rc_db, m_db, rc_t, m_t = raw_call(db, targets, ptrs, on_device)
            assert rc_db == 0 and rc_t == 0, _lib.load().kid_last_error()
            same(m_db, want, "n = %d, on_device = %d, the kid_db form" % (n, on_device))
            assert m_t.tobytes() == m_db.tobytes() and np.array_equal(m_db, m_db.transpose(1, 0, 2))
    finally:
        dev.close()


# ------------------------------------------------------------------ 3. two real samples
def test_two_samples_that_classified_different_reads():
    parent, cum, keys, targets = small_db(2e-4)
    db = KmerDB(keys, targets, parent, k=30, log2_slots=18)
    replica = db.replicate(0)
    off = synth.fixed_offsets(600, 150)
    reads = [synth.reads(cum, parent, 600, 150, read_seed=seed) for seed in (11, 12)]
    odb = oracle_db(parent, keys, targets, 18)
    samples, ucounts = [db.sample(), replica.sample()], []
    for s, bases in zip(samples, reads):
        s.classify(bases, off)
        g, u = s.end()
        o = odb_sample_counts(odb, bases, off)
        assert np.array_equal(u, o)
        ucounts.append(u)
    assert np.count_nonzero((ucounts[0] > 0) & (ucounts[1] > 0)) >= 2  # both hit at least two common targets
    maps = [s.seen_export(0, s.seen_bytes()) for s in samples]
    exp = sm.shared(targets, parent.size, maps)
    got = db.shared_kmers(samples + [maps[1]])  # Samples (one on a replica) and an array
    same(got[:2, :2], exp, "two samples")
    assert np.array_equal(got[0, 0], ucounts[0]) and np.array_equal(got[1, 1], ucounts[1]) and np.array_equal(got[2], got[1])
    assert got[0, 1].sum() < min(got[0, 0].sum(), got[1, 1].sum())  # different reads: neither sample holds the other
    same(shared_kmers(targets, parent.size, maps), exp, "two samples, the targets form")
    for s in samples:
        g, u = s.end()  # no sample was touched
        assert np.array_equal(u, ucounts[samples.index(s)])
        s.close()
    replica.close(), db.close()


def odb_sample_counts(odb, bases, off):
    from helpers import ob
    s = ob.OracleSample(odb)
    s.classify(bases, off)
    return s.counts()[1]


# ------------------------------------------------------------------ 4. errors
def test_argument_errors_write_nothing(cohort):
    targets, maps, exp, db = cohort
    ok = [m.ctypes.data for m in maps]
    untouched = np.full((65, 65, NTAR), -7, np.int64)
    for what, ptrs, n in (("n = 0", ok[:1], 0), ("n = 65", ok + ok[:1], 65), ("n = -1", ok[:1], -1), ("a null bitmap", [ok[0], None, ok[2]], 3)):
        m = untouched.copy()
        rc_db, _, rc_t, _ = raw_call(db, targets, ptrs, 0, n=n, shared=m)
        assert rc_db == -1 and rc_t == -1 and np.array_equal(m, untouched), what  # KID_ERR_ARG
    lib = _lib.load()
    m = untouched.copy()
    ptrs = (C.c_void_p * 2)(*ok[:2])
    assert lib.kid_db_shared_kmers(db._h, None, 2, 0, m.ctypes.data_as(C.c_void_p)) == -1
    assert lib.kid_db_shared_kmers(db._h, ptrs, 2, 0, None) == -1 and lib.kid_db_shared_kmers(None, ptrs, 2, 0, m.ctypes.data_as(C.c_void_p)) == -1
    assert lib.kid_shared_kmers(0, None, targets.size, NTAR, ptrs, 2, 0, m.ctypes.data_as(C.c_void_p)) == -1
    bad = targets.copy()
    bad[-1] = NTAR
    assert lib.kid_shared_kmers(0, bad.ctypes.data_as(C.c_void_p), bad.size, NTAR, ptrs, 2, 0, m.ctypes.data_as(C.c_void_p)) == -7  # KID_ERR_TARGET
    assert np.array_equal(m, untouched)
    with pytest.raises(KidError):
        shared_kmers(bad, NTAR, maps[:2])
    with pytest.raises(ValueError):
        db.shared_kmers([maps[0][:-16]])
    same(db.shared_kmers(maps[:2]), exp[:2, :2], "after the errors")
