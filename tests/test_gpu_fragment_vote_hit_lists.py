"""kid_db_fragment_votes_from_hits_device on the synthetic hit lists of tests/hit_list_cases.py (reads 2i and 2i + 1 are
the mates of fragment i: p, q and p + q stand on both sides of every edge of the three work splits, n_1 + n_2 wraps) and
on a hand-laid CSR whose fragments put the three regimes into one wave.  Every comparison with the model
(tests/read_fragment_votes_model.py) is exact, per record and field; the per-mate calls are also held to what
kid_db_votes_from_hits_device returns for the same CSR; the outputs' guard records stay untouched.  Shuffles inside the
mates, exchanges of the mates, splits of the batch, more big fragments than workgroups followed by a call on other
hits (rows left dirty would show), and a vote call beside a fragment-vote call on two streams."""
import numpy as np
import pytest

import hit_list_cases as hc
from helpers import DeviceCsr
from kmer_id_amd import FRAGMENT_VOTE_DTYPE, VOTE_DTYPE, KidError, KmerDB, _lib
from read_calls import same_records
from read_fragment_votes_model import FragmentVoteModel, exchanged, exchanged_records
from read_hits_model import Hits

pytestmark = pytest.mark.gpu

WIDE_RULES = [(0, 0), (0, 1000)]
PQ = [(0, 0), (8, 0), (0, 8), (4, 4), (5, 4), (8, 1), (64, 0), (63, 2), (256, 256), (512, 0), (0, 512), (257, 256), (512, 1), (1, 600), (600, 1),
      (600, 600)]


def call(db, d, d_out, rule, first=0, n=None, stream=0):
    """the device-form call over the reads [first, first + n) of the CSR on the device: offsets stay absolute"""
    n = d.n - first if n is None else n
    db.fragment_votes_from_hits_device(d.d_ho.value + 8 * first, d.d_hits.value, d.d_nk.value + 4 * first, n, d_out.value + 40 * (first // 2),
                                       min_hits=rule[0], min_permille=rule[1], stream=stream)


def run(db, d, rule):
    d_out = d.out(d.n // 2, FRAGMENT_VOTE_DTYPE)
    call(db, d, d_out, rule)
    _lib.check(d.lib.kid_dev_sync(0))
    return d.records(d_out, d.n // 2, FRAGMENT_VOTE_DTYPE)


def run_votes(db, d, rule, stream=0):
    d_out = d.out(d.n, VOTE_DTYPE)
    db.votes_from_hits_device(d.d_ho.value, d.d_hits.value, d.d_nk.value, d.n, d_out.value, min_hits=rule[0], min_permille=rule[1], stream=stream)
    _lib.check(d.lib.kid_dev_sync(0))
    return d.records(d_out, d.n, VOTE_DTYPE)


def csr(hits):
    return DeviceCsr(hits.offsets, hc.raw_hits(hits), hits.n_kmers)


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


def model(name):
    return FragmentVoteModel(hc.case(name).models.vm)


# ------------------------------------------------------------------ 1. all ten fields, every tree, every rule
@pytest.mark.parametrize("name", sorted(hc.TREES))
def test_all_ten_fields_equal_the_model(dbs, name):
    c, db, fvm = hc.case(name), dbs(name), model(name)
    with csr(c.hits) as d:
        for rule in (WIDE_RULES if name.startswith("wide") else hc.RULES):
            got = run(db, d, rule)
            same_records(got, fvm.batch_anc(c.hits, rule, c.plain.calls), FRAGMENT_VOTE_DTYPE, "%s, rule %s" % (name, rule))
            votes = run_votes(db, d, rule)  # GPU against GPU: the per-mate calls are the reads' vote calls
            assert np.array_equal(got["call_1"], votes["call"][0::2]) and np.array_equal(got["call_2"], votes["call"][1::2]), (name, rule)


def test_targets_outside_the_tree_are_read_as_the_root(dbs):
    c, db, fvm = hc.case("rows8"), dbs("rows8"), model("rows8")
    raw, exp = c.out_of_range
    with csr(raw) as d:
        same_records(run(db, d, (2, 25)), fvm.batch_anc(exp.hits, (2, 25), exp.calls), FRAGMENT_VOTE_DTYPE, "out of range")


# ------------------------------------------------------------------ 2. work-split edges: the three regimes in one wave
def edge_list(name, n_fragments):
    """fragments with (p, q) running through PQ, n_fragments of them; n_1 = p or 2^32 - 1, n_2 = q + 91"""
    c = hc.case(name)
    rng = np.random.default_rng([c.seed, n_fragments, 23])
    deepest = np.flatnonzero(c.depth == c.depth.max())
    per, tg = [], []
    for f in range(n_fragments):
        for mate, m in enumerate(PQ[f % len(PQ)]):
            shape = hc.SHAPES[(f // len(PQ) + f + mate) % len(hc.SHAPES)]
            per.append(m)
            tg.append(hc._targets(rng, shape, m, c.parent, c.depth, deepest))
    per = np.array(per, np.int64)
    off = np.zeros(per.size + 1, np.uint64)
    off[1:] = np.cumsum(per)
    nk = per.copy()
    nk[1::2] += 91
    nk[0::6] = 2 ** 32 - 1
    target = np.concatenate(tg + [np.empty(0, np.uint32)]).astype(np.uint32)
    count = np.arange(target.size, dtype=np.uint32)
    return Hits(off, nk.astype(np.uint32), count, target, count.copy())


@pytest.mark.parametrize("name", ["rows8", "climb9"])
def test_work_split_edges(dbs, name):
    db, fvm = dbs(name), model(name)
    assert hc.LANE_HITS == 8 and hc.WAVE_HITS == 512  # what PQ was laid out for
    for nf in (63, 64, 65):
        hits = edge_list(name, nf)
        with csr(hits) as d:
            for rule in [(0, 0), (2, 25)]:
                same_records(run(db, d, rule), fvm.batch_anc(hits, rule), FRAGMENT_VOTE_DTYPE, "%s, %d fragments, rule %s" % (name, nf, rule))
    whole = edge_list(name, 16)
    for f in (3, 7, 15):  # F = 1: a lane's, a wave's and a workgroup's fragment, each a batch of its own
        lo, hi = int(whole.offsets[2 * f]), int(whole.offsets[2 * f + 2])
        one = Hits(whole.offsets[2 * f:2 * f + 3] - whole.offsets[2 * f], whole.n_kmers[2 * f:2 * f + 2], whole.pos[lo:hi], whole.target[lo:hi],
                   whole.entry[lo:hi])
        with csr(one) as d:
            for rule in [(0, 0), (2, 25)]:
                same_records(run(db, d, rule), fvm.batch_anc(one, rule), FRAGMENT_VOTE_DTYPE, "%s, fragment %d alone, rule %s" % (name, f, rule))


# ------------------------------------------------------------------ 3. shuffles and exchanges
@pytest.mark.parametrize("name", sorted(hc.TREES))
def test_shuffles_change_nothing_and_exchanges_the_last_two_columns(dbs, name):
    c, db, fvm = hc.case(name), dbs(name), model(name)
    sh, _ = c.shuffled
    ex = exchanged(c.hits)
    for rule in [(0, 0), (2, 25)]:
        with csr(c.hits) as d:
            plain = run(db, d, rule)
        with csr(sh) as d:
            assert run(db, d, rule).tobytes() == plain.tobytes(), (name, rule)
        with csr(ex) as d:
            got = run(db, d, rule)
        assert got.tobytes() == exchanged_records(plain).tobytes(), (name, rule)
        assert (plain["call_1"] != plain["call_2"]).any()
        same_records(got, fvm.batch_anc(ex, rule), FRAGMENT_VOTE_DTYPE, "%s, exchanged, rule %s" % (name, rule))


# ------------------------------------------------------------------ 4. splits
@pytest.mark.parametrize("name", sorted(hc.TREES))
def test_three_calls_give_the_bytes_of_one(dbs, name):
    c, db, rule = hc.case(name), dbs(name), (2, 25)
    with csr(c.hits) as d:
        whole = run(db, d, rule)
        d_out = d.out(d.n // 2, FRAGMENT_VOTE_DTYPE)
        cuts = [0, 66, 130, hc.N_READS]  # even read indexes: 33, 32 and 37 fragments
        for a, b in zip(cuts[:-1], cuts[1:]):
            call(db, d, d_out, rule, a, b - a)
        _lib.check(d.lib.kid_dev_sync(0))
        assert d.records(d_out, d.n // 2, FRAGMENT_VOTE_DTYPE).tobytes() == whole.tobytes(), name


# ------------------------------------------------------------------ 5. the big regime
def big_fragments(c, n, seed):
    """n fragments of 600 + 600 hits, uniform over the tree's nodes"""
    rng = np.random.default_rng([seed, n])
    off = np.arange(2 * n + 1, dtype=np.uint64) * 600
    target = rng.integers(1, c.ntar, int(off[-1])).astype(np.uint32)
    count = np.arange(target.size, dtype=np.uint32)
    return Hits(off, np.full(2 * n, 700, np.uint32), count, target, count.copy())


def test_more_big_fragments_than_workgroups_and_clean_rows_behind_them(dbs):
    c, db, fvm = hc.case("flat"), dbs("flat"), model("flat")
    a, b = big_fragments(c, 300, 5), big_fragments(c, 40, 6)
    import torch
    assert torch.cuda.get_device_properties(0).multi_processor_count < 300  # one workgroup per compute unit takes the list
    for hits, what in ((a, "300 big fragments"), (b, "a second call on other hits"), (c.hits, "a third on the lists")):
        with csr(hits) as d:
            same_records(run(db, d, (2, 25)), fvm.batch_anc(hits, (2, 25)), FRAGMENT_VOTE_DTYPE, what)


# ------------------------------------------------------------------ 6. a vote call and a fragment-vote call on two streams
@pytest.mark.parametrize("first", ["votes", "fragment_votes"])
def test_a_vote_call_and_a_fragment_vote_call_on_two_streams(dbs, first):
    """nothing between the two calls waits: each must find a list, a counter and rows that the other does not touch.
    Both CSRs send hundreds of units to the second kernels."""
    import torch
    c, db, fvm, rule = hc.case("rows8"), dbs("rows8"), model("rows8"), (2, 25)
    a, b = hc.big_reads(c, 600), big_fragments(c, 300, 9)
    exp_votes, exp_frag = c.models.votes(a, rule), fvm.batch_anc(b, rule)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with csr(a) as da, csr(b) as db_:
        out_v, out_f = da.out(da.n, VOTE_DTYPE), db_.out(db_.n // 2, FRAGMENT_VOTE_DTYPE)
        _lib.check(da.lib.kid_dev_sync(0))
        db.read_fragment_votes_time()

        def votes(stream):
            db.votes_from_hits_device(da.d_ho.value, da.d_hits.value, da.d_nk.value, da.n, out_v.value, min_hits=rule[0], min_permille=rule[1],
                                      stream=stream.cuda_stream)

        if first == "votes":
            votes(s1)
            call(db, db_, out_f, rule, stream=s2.cuda_stream)
        else:
            call(db, db_, out_f, rule, stream=s1.cuda_stream)
            votes(s2)
        _lib.check(da.lib.kid_dev_sync(0))
        got_v, got_f = da.records(out_v, da.n, VOTE_DTYPE), db_.records(out_f, db_.n // 2, FRAGMENT_VOTE_DTYPE)
        for f in exp_votes.dtype.names:
            assert np.array_equal(got_v[f], exp_votes[f]), (first, f)
        same_records(got_f, exp_frag, FRAGMENT_VOTE_DTYPE, "%s first" % first)
        ms, calls, frags = db.read_fragment_votes_time()
        assert (calls, frags) == (1, 300) and ms > 0


# ------------------------------------------------------------------ 7. odd and empty batches
def test_an_odd_batch_is_refused_and_an_empty_one_writes_nothing(dbs):
    c, db = hc.case("rows8"), dbs("rows8")
    with csr(c.hits) as d:
        d_out = d.out(d.n // 2, FRAGMENT_VOTE_DTYPE)
        with pytest.raises(KidError) as e:
            call(db, d, d_out, (0, 0), 0, 5)
        assert e.value.status == -1
        call(db, d, d_out, (0, 0), 0, 0)
        _lib.check(d.lib.kid_dev_sync(0))
        assert np.all(d.down(d_out, np.uint32, 10 * (d.n // 2)) == d.CANARY)
    lib = _lib.load()
    assert lib.kid_db_fragment_votes_from_hits_device(db._h, None, None, None, 0, 0, 0, None, None) == 0
    assert lib.kid_db_fragment_votes_from_hits_device(db._h, None, None, None, 6, 0, 0, None, None) == -1
    assert lib.kid_db_fragment_votes_from_hits_device(db._h, None, None, None, 0, 0, 1001, None, None) == -1
