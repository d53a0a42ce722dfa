"""kid_db_support_from_hits_device, kid_db_fragments_from_hits_device and kid_db_votes_from_hits_device on the synthetic hit
lists of tests/hit_list_cases.py: lists no read against a table gives -- trees of depth 8 (the last the ancestor rows hold)
and 9, a flat tree, 65536 and 65537 nodes; reads of 0 to 5000 hits at every edge of the kernels' work splits; ties below and
at the root by the dozen; n_kmers up to 2^32 - 1, among them the value at which a 32-bit `1000 * n` wraps; targets outside
(0, ntar).  Every comparison with the models (SupportModel, FragmentModel's record, VoteModel) is exact, per record and
field; the outputs' guard records stay untouched.  The last test queues vote calls on two streams with nothing between
them: the second must not bind the list, the counter and the rows of the first while its second kernel still runs."""
import numpy as np
import pytest

import hit_list_cases as hc
import read_support_cases as sc
from helpers import DeviceCsr, concat_reads
from kmer_id_amd import FRAGMENT_DTYPE, VOTE_DTYPE, KmerDB, _lib
from kmer_id_amd.api import SUPPORT_DTYPE
from read_calls import same_records

pytestmark = pytest.mark.gpu

FAMILIES = {"support": (SUPPORT_DTYPE, 1), "fragments": (FRAGMENT_DTYPE, 2), "votes": (VOTE_DTYPE, 1)}  # the record, reads per record
WIDE_RULES = [(0, 0), (0, 1000)]
CUTS = [0, 65, 130, hc.N_READS]


def call(db, family, d, d_out, rule, first=0, n=None, stream=0):
    """the family's device-form call over the reads [first, first + n) of the CSR on the device: offsets stay absolute"""
    dtype, unit = FAMILIES[family]
    n = d.n - first if n is None else n
    getattr(db, family + "_from_hits_device")(d.d_ho.value + 8 * first, d.d_hits.value, d.d_nk.value + 4 * first, n,
                                              d_out.value + dtype.itemsize * (first // unit), min_hits=rule[0], min_permille=rule[1], stream=stream)


def run(db, family, d, rule):
    dtype, unit = FAMILIES[family]
    d_out = d.out(d.n // unit, dtype)
    call(db, family, d, d_out, rule)
    _lib.check(d.lib.kid_dev_sync(0))
    return d.records(d_out, d.n // unit, dtype)


@pytest.fixture(scope="module")
def dbs():
    made = {}

    def get(name):
        if name not in made:
            c = hc.case(name)
            made[name] = KmerDB(c.models.keys, c.models.targets, c.parent, k=hc.K, log2_slots=10)
            assert made[name].info.tree_depth == c.max_depth and made[name].info.ntar == c.ntar
        return made[name]

    yield get
    for d in made.values():
        d.close()


# ------------------------------------------------------------------ 1. every family, every tree, every rule
@pytest.mark.parametrize("variant", ["plain", "out_of_range"])
@pytest.mark.parametrize("name", sorted(hc.TREES))
def test_every_family_equals_its_model(dbs, name, variant):
    c, db = hc.case(name), dbs(name)
    hits, exp = (c.hits, c.plain) if variant == "plain" else c.out_of_range
    rules = WIDE_RULES if name.startswith("wide") else hc.RULES
    with DeviceCsr(hits.offsets, hc.raw_hits(hits), hits.n_kmers) as d:
        for family in FAMILIES:
            for rule in rules:
                same_records(run(db, family, d, rule), getattr(exp, family)(rule), FAMILIES[family][0],
                             "%s, %s, %s, rule %s" % (name, variant, family, rule))


# ------------------------------------------------------------------ 2. splits
@pytest.mark.parametrize("name", sorted(hc.TREES))
def test_three_calls_give_the_bytes_of_one(dbs, name):
    c, db, rule = hc.case(name), dbs(name), (2, 25)
    with DeviceCsr(c.hits.offsets, hc.raw_hits(c.hits), c.hits.n_kmers) as d:
        for family, (dtype, unit) in FAMILIES.items():
            whole = run(db, family, d, rule)
            same_records(whole, getattr(c.plain, family)(rule), FAMILIES[family][0], "%s, %s, one call" % (name, family))
            d_out = d.out(d.n // unit, dtype)
            cuts = [x + x % unit for x in CUTS]  # (a batch of fragments is cut between two pairs: 66 reads, 130 = 65 fragments)
            for a, b in zip(cuts[:-1], cuts[1:]):
                call(db, family, d, d_out, rule, a, b - a)
            _lib.check(d.lib.kid_dev_sync(0))
            assert d.records(d_out, d.n // unit, dtype).tobytes() == whole.tobytes(), (name, family)


# ------------------------------------------------------------------ 3. votes depend on the multiset alone
@pytest.mark.parametrize("name", sorted(hc.TREES))
def test_votes_survive_a_shuffle_of_every_reads_hits_and_finals_do_not(dbs, name):
    c, db = hc.case(name), dbs(name)
    sh, sh_exp = c.shuffled
    for rule in [(0, 0), (2, 25)]:
        with DeviceCsr(c.hits.offsets, hc.raw_hits(c.hits), c.hits.n_kmers) as d:
            votes, support = run(db, "votes", d, rule), run(db, "support", d, rule)
        with DeviceCsr(sh.offsets, hc.raw_hits(sh), sh.n_kmers) as d:
            votes_sh, support_sh = run(db, "votes", d, rule), run(db, "support", d, rule)
        assert votes_sh.tobytes() == votes.tobytes(), (name, rule)
        same_records(votes_sh, c.plain.votes(rule), VOTE_DTYPE, "%s, shuffled, rule %s" % (name, rule))
        same_records(support_sh, sh_exp.support(rule), SUPPORT_DTYPE, "%s, shuffled, support, rule %s" % (name, rule))
        assert (support_sh["final"] != support["final"]).any()  # ... which `final` does not survive


# ------------------------------------------------------------------ 4. two vote calls on two streams
@pytest.fixture(scope="module")
def race():
    c = hc.case("rows8")
    a = hc.big_reads(c)
    assert int(np.diff(a.offsets.astype(np.int64)).min()) == hc.WAVE_HITS + 1 and a.offsets.size - 1 == 2000
    rng = np.random.default_rng(41)
    seqs = []
    for n_implanted in (0, 1, 3, 9, 20, 40):
        pick = rng.integers(0, c.models.keys.size, n_implanted)
        seqs.append(sc.implanted(rng, [sc.cases.key_seq(c.models.keys[j], hc.K) for j in pick], gap=1))
    bases, off = concat_reads(seqs)
    rule = (2, 25)
    host_hits = c.models.hm.batch(bases, off)
    assert int(np.diff(host_hits.offsets.astype(np.int64)).max()) >= 40
    return {"A": a, "B": c.hits, "bases": bases, "off": off, "rule": rule, "exp_A": c.models.votes(a, rule), "exp_B": c.plain.votes(rule),
            "exp_support_B": c.plain.support(rule), "exp_host": c.models.votes(host_hits, rule)}


@pytest.mark.parametrize("first", ["A", "B"])
def test_vote_calls_on_two_streams_do_not_share_scratch_in_flight(dbs, race, first):
    """votes(first) on one stream, votes(second) and support(B) on another, a host-form read_votes, and only then a
    synchronisation: nothing here waits for the first call, the library has to (KID_SETTLE_VOTES).  A: 2000 reads for the
    second kernel, which took the two vote kernels 0.43 ms on an MI355X against a launch of microseconds, so a call that
    did not wait would zero the counter and bind the rows under it -- most of the time, not every time."""
    import torch
    db, rule = dbs("rows8"), race["rule"]
    second = "B" if first == "A" else "A"
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    n_host = race["off"].size - 1
    with DeviceCsr(race["A"].offsets, hc.raw_hits(race["A"]), race["A"].n_kmers) as da, \
            DeviceCsr(race["B"].offsets, hc.raw_hits(race["B"]), race["B"].n_kmers) as db_:
        dev = {"A": da, "B": db_}
        if first == "A":  # what the second kernel costs on list A alone: for the log, outside the race
            db.read_votes_time()
            same_records(run(db, "votes", da, rule), race["exp_A"], VOTE_DTYPE, "A alone")
            print("votes(A) alone: read_votes_time = %s" % (db.read_votes_time(),))
        out = {name: d.out(d.n, VOTE_DTYPE) for name, d in dev.items()}
        out_support = db_.out(db_.n, SUPPORT_DTYPE)
        _lib.check(da.lib.kid_dev_sync(0))
        db.read_votes_time()
        call(db, "votes", dev[first], out[first], rule, stream=s1.cuda_stream)
        call(db, "votes", dev[second], out[second], rule, stream=s2.cuda_stream)
        call(db, "support", db_, out_support, rule, stream=s2.cuda_stream)
        host = db.read_votes(race["bases"], race["off"], min_hits=rule[0], min_permille=rule[1])
        _lib.check(da.lib.kid_dev_sync(0))
        same_records(da.records(out["A"], da.n, VOTE_DTYPE), race["exp_A"], VOTE_DTYPE, "A, %s first" % first)
        same_records(db_.records(out["B"], db_.n, VOTE_DTYPE), race["exp_B"], VOTE_DTYPE, "B, %s first" % first)
        same_records(db_.records(out_support, db_.n, SUPPORT_DTYPE), race["exp_support_B"], SUPPORT_DTYPE, "support(B), %s first" % first)
        same_records(host, race["exp_host"], VOTE_DTYPE, "host form, %s first" % first)
        ms, calls, reads = db.read_votes_time()
        assert (calls, reads) == (3, 2000 + hc.N_READS + n_host) and ms > 0
