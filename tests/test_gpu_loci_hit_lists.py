"""kid_db_loci_from_hits_device on the synthetic hit lists of tests/read_loci_cases.py: reads of 0 to 5000 hits at every edge
of the kernels' three regimes and of the 4096 participants; one long chain, two chains of equal size on two orgs, one org
on distinct diagonals, uniform hits over three orgs, forward and reverse chains of equal size; read positions up to
2^32 - 1, sites up to 2^31 - 1, org 2^24 - 1; diagonal bins of width 1, 7 and 2^31 - 1; entries outside the database; every
list once more with every read's hits shuffled.  Every record equals the model's (tests/read_loci_model.py) field by field;
the outputs' guard records stay untouched.  The last test queues two calls on two streams with nothing between them."""
import numpy as np
import pytest

import read_loci_cases as lc
import read_support_cases as sc
from helpers import DeviceCsr, concat_reads, oracle_db
from hit_list_cases import raw_hits
from kmer_id_amd import LOCUS_DTYPE, KmerDB, _lib
from read_calls import same_records
from read_hits_model import HitModel
import read_loci_model as lm

pytestmark = pytest.mark.gpu

CUTS = [0, 21, 50, lc.N_READS]


@pytest.fixture(scope="module")
def db():
    c = lc.case()
    parent = np.ones(8, np.int32)
    d = KmerDB(c.keys, c.targets, parent, k=lc.K, log2_slots=15)
    assert d.info.n_entries == lc.N_ENTRIES
    d.set_sites(c.org, c.pos)
    yield d
    d.close()


def call(db, d, d_out, w, first=0, n=None, stream=0):
    """the device-form call over the reads [first, first + n) of the CSR on the device: offsets stay absolute"""
    n = d.n - first if n is None else n
    db.loci_from_hits_device(d.d_ho.value + 8 * first, d.d_hits.value, d.d_nk.value + 4 * first, n, d_out.value + LOCUS_DTYPE.itemsize * first,
                             diag_bin=w, stream=stream)


def run(db, d, w):
    d_out = d.out(d.n, LOCUS_DTYPE)
    call(db, d, d_out, w)
    _lib.check(d.lib.kid_dev_sync(0))
    return d.records(d_out, d.n, LOCUS_DTYPE)


def test_the_lists_cover_what_they_are_for():
    c = lc.case()
    assert LOCUS_DTYPE == lm.LOCUS_DTYPE
    ms = {m for m, s in c.what}
    for edge in (lc.LANE_HITS, lc.WAVE_HITS, 64, 4096):
        assert {edge - 1, edge, edge + 1} <= ms
    assert {0, 1, 2, 5000} <= ms and int(c.hits.pos.max()) == 2 ** 32 - 1
    exp = c.expected("hits", 1)
    assert {0, 1} == set(exp["strand"].tolist()) and lc.ORG_A in set(exp["org"].tolist())
    assert (exp["n_other"] == exp["n_chain"]).sum() >= 10 and int(exp["n_chain"].max()) == 4096
    assert (c.out_of_range.entry >= lc.N_ENTRIES).sum() > 100


@pytest.mark.parametrize("w", lc.WIDTHS)
@pytest.mark.parametrize("variant", ["hits", "shuffled", "out_of_range"])
def test_every_record_equals_the_models(db, variant, w):
    c = lc.case()
    hits = getattr(c, variant)
    with DeviceCsr(hits.offsets, raw_hits(hits), hits.n_kmers) as d:
        got = run(db, d, w)
    same_records(got, c.expected(variant, w), LOCUS_DTYPE, "%s, W = %d" % (variant, w))
    if variant == "shuffled":  # the multiset alone, as long as all of it takes part
        small = np.array([m <= lc.MAX_HITS for m, s in c.what])
        assert got[small].tobytes() == c.expected("hits", w)[small].tobytes()


def test_three_calls_and_a_second_run_give_the_bytes_of_one(db):
    c, w = lc.case(), 7
    with DeviceCsr(c.hits.offsets, raw_hits(c.hits), c.hits.n_kmers) as d:
        whole = run(db, d, w)
        assert run(db, d, w).tobytes() == whole.tobytes()
        d_out = d.out(d.n, LOCUS_DTYPE)
        for a, b in zip(CUTS[:-1], CUTS[1:]):
            call(db, d, d_out, w, a, b - a)
        _lib.check(d.lib.kid_dev_sync(0))
        assert d.records(d_out, d.n, LOCUS_DTYPE).tobytes() == whole.tobytes()
    same_records(whole, c.expected("hits", w), LOCUS_DTYPE, "one call")


@pytest.mark.parametrize("first", ["A", "B"])
def test_calls_on_two_streams_do_not_share_scratch_in_flight(db, first):
    """loci(first) on one stream, loci(second) on another, a host-form read_loci, and only then a synchronisation: nothing
    here waits for the first call, the library has to (kid_settle(KID_FAM_LOCI)) before it zeroes the counter of the list
    and binds the list again.  A: 600 reads, all for the second kernel."""
    import torch
    c, w = lc.case(), 1
    lists = {"A": c.big, "B": c.hits}
    exp = {"A": c.expected("big", w), "B": c.expected("hits", w)}
    rng = np.random.default_rng(41)
    seqs = [sc.implanted(rng, [sc.cases.key_seq(c.keys[j], lc.K) for j in rng.integers(0, c.keys.size, n)], gap=1) for n in (0, 1, 3, 9, 20, 40)]
    bases, off = concat_reads(seqs)
    hm = HitModel(oracle_db(np.ones(8, np.int32), c.keys, c.targets, 15), c.keys, c.targets, lc.K)
    host_hits = hm.batch(bases, off)
    assert int(np.diff(host_hits.offsets.astype(np.int64)).max()) >= 40
    second = "B" if first == "A" else "A"
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with DeviceCsr(lists["A"].offsets, raw_hits(lists["A"]), lists["A"].n_kmers) as da, \
            DeviceCsr(lists["B"].offsets, raw_hits(lists["B"]), lists["B"].n_kmers) as db_:
        dev = {"A": da, "B": db_}
        out = {name: d.out(d.n, LOCUS_DTYPE) for name, d in dev.items()}
        _lib.check(da.lib.kid_dev_sync(0))
        db.read_loci_time()
        call(db, dev[first], out[first], w, stream=s1.cuda_stream)
        call(db, dev[second], out[second], w, stream=s2.cuda_stream)
        host = db.read_loci(bases, off, diag_bin=w)
        _lib.check(da.lib.kid_dev_sync(0))
        for name in ("A", "B"):
            same_records(dev[name].records(out[name], dev[name].n, LOCUS_DTYPE), exp[name], LOCUS_DTYPE, "%s, %s first" % (name, first))
        same_records(host, lm.batch(host_hits, c.org, c.pos, w), LOCUS_DTYPE, "host form, %s first" % first)
        ms, calls, reads = db.read_loci_time()
        assert (calls, reads) == (3, 600 + lc.N_READS + off.size - 1) and ms > 0
