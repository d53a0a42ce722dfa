"""kid_db_fragment_loci_from_hits_device on the synthetic interleaved hit lists of tests/read_fragment_loci_cases.py: mates
of 0 to 5000 hits at every edge of the kernels' two regimes and of the 4096 participants, absent mates, proper pairs on
either org and in either orientation, equal scores on two orgs, a paired and a solo placement of equal score, D > E, the
partner exactly at max_span and one base beyond for W = 1 and W = 7, max_span = 0, read positions up to 2^32 - 1, sites up
to 2^31 - 1, org 2^24 - 1 (hi saturates), entries outside the database; every list once more with each mate's hits shuffled.
Every record equals the model's (tests/read_fragment_loci_model.py) field by field; the outputs' guard records stay
untouched.  The last test queues two calls on two streams with a host-form call behind them."""
import numpy as np
import pytest

import read_fragment_loci_cases as fc
import read_fragment_loci_model as fm
import read_support_cases as sc
from helpers import DeviceCsr, concat_reads, oracle_db
from hit_list_cases import raw_hits
from kmer_id_amd import FRAGMENT_LOCUS_DTYPE, KmerDB, _lib
from read_calls import same_records
from read_hits_model import HitModel

pytestmark = pytest.mark.gpu

SIZE = FRAGMENT_LOCUS_DTYPE.itemsize


@pytest.fixture(scope="module")
def db():
    c = fc.case()
    d = KmerDB(c.keys, c.targets, np.ones(8, np.int32), k=fc.K, log2_slots=15)
    assert d.info.n_entries == fc.N_ENTRIES
    d.set_sites(c.org, c.pos)
    yield d
    d.close()


def call(db, d, d_out, rule, first=0, n=None, stream=0):
    """the device-form call over the fragments [first, first + n) of the CSR on the device: offsets stay absolute"""
    n = d.n // 2 - first if n is None else n
    db.fragment_loci_from_hits_device(d.d_ho.value + 16 * first, d.d_hits.value, d.d_nk.value + 8 * first, 2 * n, d_out.value + SIZE * first,
                                      diag_bin=rule[0], max_span=rule[1], stream=stream)


def run(db, d, rule):
    d_out = d.out(d.n // 2, FRAGMENT_LOCUS_DTYPE)
    call(db, d, d_out, rule)
    _lib.check(d.lib.kid_dev_sync(0))
    return d.records(d_out, d.n // 2, FRAGMENT_LOCUS_DTYPE)


def test_the_lists_cover_what_they_are_for():
    c = fc.case()
    assert FRAGMENT_LOCUS_DTYPE == fm.FRAGMENT_LOCUS_DTYPE and SIZE == 64
    pairs = {(a, b) for a, b, s in c.what}
    L = fc.LANE_HITS
    for x in (L - 1, L, L + 1):  # the edge of the lane regime in either mate, the other on either side of it
        for y in (0, 1, L, L + 1):
            assert (x, y) in pairs and (y, x) in pairs
    for m in (0, 1, 2, 4095, 4096, 4097):
        assert any(m in p for p in pairs)
    assert (5000, 1) in pairs and (1, 5000) in pairs and int(c.hits.pos.max()) == 2 ** 32 - 1
    assert any(a == 0 and b > 0 for a, b in pairs) and any(b == 0 and a > 0 for a, b in pairs)
    for w, s in fc.RULES[:4]:  # the partner at max_span pairs, one base beyond it does not
        exp = c.expected("hits", (w, s))
        for suffix in ("", "_swapped"):
            assert exp[c.index("at_%d_%d%s" % (w, s, suffix))]["mates"] == 3 and exp[c.index("beyond_%d_%d%s" % (w, s, suffix))]["mates"] != 3
        assert exp[c.index("D_above_E")]["mates"] != 3
    exp = c.expected("hits", (1, 1000))
    assert {0, 1, 2, 3} == set(exp["mates"].tolist()) and {0, 1} == set(exp["orient"][exp["mates"] == 3].tolist())
    assert {fc.ORG_A, fc.ORG_B} <= set(exp["org"].tolist())
    tie = exp[c.index("two_orgs_tie")]
    assert tie["n_other"] == tie["n_chain"] == 2 and tie["org"] == fc.ORG_A
    tie = exp[c.index("pair_and_solo_tie")]
    assert tie["mates"] == 3 and tie["n_chain"] == 2 and c.expected("hits", (1, 0))[c.index("pair_and_solo_tie")]["mates"] == 1
    assert int(c.expected("hits", fc.RULES[4])[c.index("saturate")]["hi"]) == 2 ** 32 - 1
    assert (c.out_of_range.entry >= fc.N_ENTRIES).sum() > 100


@pytest.mark.parametrize("rule", fc.RULES, ids=lambda r: "W%d_S%d" % r)
@pytest.mark.parametrize("variant", ["hits", "shuffled", "out_of_range"])
def test_every_record_equals_the_models(db, variant, rule):
    c = fc.case()
    hits = getattr(c, variant)
    with DeviceCsr(hits.offsets, raw_hits(hits), hits.n_kmers) as d:
        got = run(db, d, rule)
    same_records(got, c.expected(variant, rule), FRAGMENT_LOCUS_DTYPE, "%s, (W, max_span) = %s" % (variant, rule))
    if variant == "shuffled":  # the two multisets alone, as long as all of both take part
        small = np.array([a <= fc.MAX_HITS and b <= fc.MAX_HITS for a, b, s in c.what])
        assert small.sum() >= c.n_fragments - 8
        assert got[small].tobytes() == c.expected("hits", rule)[small].tobytes()


def test_three_calls_and_a_second_run_give_the_bytes_of_one(db):
    c, rule = fc.case(), (7, 1000)
    cuts = [0, 21, 50, c.n_fragments]
    with DeviceCsr(c.hits.offsets, raw_hits(c.hits), c.hits.n_kmers) as d:
        whole = run(db, d, rule)
        assert run(db, d, rule).tobytes() == whole.tobytes()
        d_out = d.out(d.n // 2, FRAGMENT_LOCUS_DTYPE)
        for a, b in zip(cuts[:-1], cuts[1:]):
            call(db, d, d_out, rule, a, b - a)
        _lib.check(d.lib.kid_dev_sync(0))
        assert d.records(d_out, d.n // 2, FRAGMENT_LOCUS_DTYPE).tobytes() == whole.tobytes()
    same_records(whole, c.expected("hits", rule), FRAGMENT_LOCUS_DTYPE, "one call")


@pytest.mark.parametrize("first", ["A", "B"])
def test_calls_on_two_streams_do_not_share_scratch_in_flight(db, first):
    """a call on one stream, a second on another, a host-form read_fragment_loci, and only then a synchronisation: nothing
    here waits for the first call, the library has to (its own family's timer) before it zeroes the counter of the list and
    binds the list again.  A: 300 fragments, all for the second kernel."""
    import torch
    c, rule = fc.case(), (1, 1000)
    lists = {"A": c.big, "B": c.hits}
    exp = {"A": c.expected("big", rule), "B": c.expected("hits", rule)}
    rng = np.random.default_rng(41)
    seqs = [sc.implanted(rng, [sc.cases.key_seq(c.keys[j], fc.K) for j in rng.integers(0, c.keys.size, n)], gap=1) for n in (0, 1, 3, 9, 20, 40)]
    bases, off = concat_reads(seqs)
    hm = HitModel(oracle_db(np.ones(8, np.int32), c.keys, c.targets, 15), c.keys, c.targets, fc.K)
    host_hits = hm.batch(bases, off)
    assert int(np.diff(host_hits.offsets.astype(np.int64)).max()) >= 40
    second = "B" if first == "A" else "A"
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with DeviceCsr(lists["A"].offsets, raw_hits(lists["A"]), lists["A"].n_kmers) as da, \
            DeviceCsr(lists["B"].offsets, raw_hits(lists["B"]), lists["B"].n_kmers) as db_:
        dev = {"A": da, "B": db_}
        out = {name: d.out(d.n // 2, FRAGMENT_LOCUS_DTYPE) for name, d in dev.items()}
        _lib.check(da.lib.kid_dev_sync(0))
        db.read_fragment_loci_time()
        call(db, dev[first], out[first], rule, stream=s1.cuda_stream)
        call(db, dev[second], out[second], rule, stream=s2.cuda_stream)
        host = db.read_fragment_loci(bases, off, diag_bin=rule[0], max_span=rule[1])
        _lib.check(da.lib.kid_dev_sync(0))
        for name in ("A", "B"):
            same_records(dev[name].records(out[name], dev[name].n // 2, FRAGMENT_LOCUS_DTYPE), exp[name], FRAGMENT_LOCUS_DTYPE,
                         "%s, %s first" % (name, first))
        same_records(host, fm.batch(host_hits, c.org, c.pos, fc.K, *rule), FRAGMENT_LOCUS_DTYPE, "host form, %s first" % first)
        ms, calls, fragments = db.read_fragment_loci_time()
        assert (calls, fragments) == (3, 300 + c.n_fragments + (off.size - 1) // 2) and ms > 0
