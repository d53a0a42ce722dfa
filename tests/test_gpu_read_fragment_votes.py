"""kid_db_read_fragment_votes* (mate pairs called by root-path votes) through the hit pass, on the small synthetic world
of tests/test_gpu_read_fragments.py: against the independent model of tests/read_fragment_votes_model.py applied to
HitModel.batch, against the vote calls of the same library, and against its own contract (tally, depth, the counted
fragments of the FASTQ form, error statuses, the device form, the timer).  Every comparison is exact."""
import numpy as np
import pytest

import read_depth_model as dm
import read_fragments_cases as fc
import read_calls
import read_support_cases as sc
from helpers import DeviceBatch, fastq_block
from kmer_id_amd import FRAGMENT_VOTE_DTYPE, KID_DB_OPT_MIN_BASE_QUALITY, KID_FLAG_REF_GEOMETRY, KID_OPT_ENTRY_DEPTH, KmerDB, _lib
from read_calls import ends_equal, fastq_model, fastq_world, same_records, status
from read_fragment_votes_model import FragmentVoteModel
from read_fragments_model import fragment_csr
from read_votes_model import VoteModel

pytestmark = pytest.mark.gpu

RULES = [(0, 0), (2, 25), (3, 0)]


@pytest.fixture(scope="module")
def world():
    """the fragments of tests/read_fragments_cases.py: a few hundred ragged mates, some empty, the hand-built pairs"""
    parent, cum, keys, targets = sc.database()
    bases, off, where = fc.fragments(parent, cum, keys, targets)
    w = read_calls.World(parent, keys, targets, bases, off, 20)
    w.where, w.cum, w.hits, w.nf = where, cum, w.hm.batch(bases, off), (off.size - 1) // 2
    w.fvm = FragmentVoteModel(VoteModel(w.sm))
    w.vexp = {rule: w.fvm.batch_anc(w.hits, rule) for rule in RULES}
    return w


@pytest.fixture(scope="module")
def db(world):
    d = world.db()
    yield d
    d.close()


# ------------------------------------------------------------------ 1. the model, both table kinds
@pytest.mark.parametrize("flags", [0, KID_FLAG_REF_GEOMETRY])
def test_all_ten_fields_equal_the_model(world, flags):
    a = world.vexp[(0, 0)][world.where["8|X_6"]]  # the fold says 6 here; the vote 8, whichever mate comes first
    b = world.vexp[(0, 0)][world.where["X_6|8"]]
    assert (int(a["call"]), int(a["call_1"]), int(a["call_2"])) == (8, 8, 1) and (int(b["call"]), int(b["call_1"]), int(b["call_2"])) == (8, 1, 8)
    per = np.diff(world.hits.offsets.astype(np.int64))
    assert ((per[0::2] == 0) & (per[1::2] > 0)).any() and ((per[0::2] > 0) & (per[1::2] == 0)).any() and ((per[0::2] + per[1::2]) == 0).any()
    d = world.db(flags)
    for rule, exp in world.vexp.items():
        same_records(d.read_fragment_votes(world.bases, world.off, min_hits=rule[0], min_permille=rule[1]), exp, FRAGMENT_VOTE_DTYPE,
                     "flags %d rule %s" % (flags, rule))
    d.close()


def test_per_mate_calls_are_what_read_votes_returns(world, db):
    got = db.read_fragment_votes(world.bases, world.off, min_hits=2, min_permille=25)
    votes = db.read_votes(world.bases, world.off, min_hits=2, min_permille=25)
    assert np.array_equal(got["call_1"], votes["call"][0::2]) and np.array_equal(got["call_2"], votes["call"][1::2])
    frag = db.read_fragments(world.bases, world.off, min_hits=2, min_permille=25)
    assert np.array_equal(got["n_kmers"], frag["n_kmers"]) and np.array_equal(got["n_hits"], frag["n_hits"])


def test_records_do_not_depend_on_the_split_into_calls(world, db):
    a = db.read_fragment_votes(world.bases, world.off, min_hits=2, min_permille=25)
    for cut in (1, 64):
        parts = [db.read_fragment_votes(world.bases, world.off[:2 * cut + 1], min_hits=2, min_permille=25),
                 db.read_fragment_votes(world.bases, world.off[2 * cut:], min_hits=2, min_permille=25)]
        assert np.concatenate(parts).tobytes() == a.tobytes(), cut


# ------------------------------------------------------------------ 2. the FASTQ form: dropped records, absent mates
@pytest.mark.parametrize("q", [0, 20])
def test_fastq_form(world, db, q):
    n, (s1, q1, t1, r1), (s2, q2, t2, r2) = fastq_world(world)
    hits, keep1, keep2 = fastq_model(world, (s1, q1), (s2, q2), q)
    assert (keep1 & ~keep2).sum() >= 20 and (~keep1 & keep2).sum() >= 20 and (~keep1 & ~keep2).sum() >= 20
    assert tuple(r2[9 + 200, [1, 3]]) == (0, 0)  # an absent mate
    counted = keep1 | keep2
    db.set_option(KID_DB_OPT_MIN_BASE_QUALITY, q)
    try:
        for rule in [(0, 0), (2, 25)]:
            exp = world.fvm.batch_anc(hits, rule)
            t = db.sample()
            got = db.read_fragment_votes_fastq(t1, r1[5:5 + n], t2, r2[9:9 + n], min_hits=rule[0], min_permille=rule[1], tally=t)
            same_records(got, exp, FRAGMENT_VOTE_DTYPE, "q %d rule %s" % (q, rule))
            g, u = t.end()
            assert ends_equal((g, u), world.fvm.tally(hits, exp, counted, world.targets)), (q, rule)
            assert int(g.sum()) == int(counted.sum()) < n  # a fragment with both mates dropped is counted nowhere
            t.close()
    finally:
        db.set_option(KID_DB_OPT_MIN_BASE_QUALITY, 0)


# ------------------------------------------------------------------ 3. tally
def test_tally_equals_the_model_and_adds_to_a_classified_sample(world, db):
    counted = np.ones(world.nf, bool)
    t = db.sample()
    rec = db.read_fragment_votes(world.bases, world.off, min_hits=2, min_permille=25, tally=t)
    exp = world.vexp[(2, 25)]
    same_records(rec, exp, FRAGMENT_VOTE_DTYPE)
    g, u = world.fvm.tally(world.hits, exp, counted, world.targets)
    assert int(g.sum()) == world.nf and int(g[0]) > int((exp["call"] == 0).sum())  # once per fragment; the rule un-calls some
    before = t.stats()
    assert ends_equal(t.end(), (g, u))
    assert before == {"reads": 0, "lookups": 0, "probes": 0, "hits": 0}  # kid_sample_stats is not updated
    t.reset()
    db.read_fragment_votes(world.bases, world.off, tally=t, min_hits=3)  # out is what the Python form always asks for; a reset sample counts from nothing
    assert ends_equal(t.end(), world.fvm.tally(world.hits, world.vexp[(3, 0)], counted, world.targets))
    # classify and this tally in one sample: the reads and the fragments add up, and under (0, 0) both see the same k-mers
    t.reset()
    t.classify(world.bases, world.off)
    db.read_fragment_votes(world.bases, world.off, tally=t)
    both = t.end()
    t.reset()
    t.classify(world.bases, world.off)
    alone = t.end()
    g0, u0 = world.fvm.tally(world.hits, world.vexp[(0, 0)], counted, world.targets)
    assert np.array_equal(both[0], alone[0] + g0) and np.array_equal(both[1], alone[1]) and np.array_equal(u0, alone[1])
    t.close()


def test_depth_counts_every_hit_of_both_mates(world, db):
    s = db.sample()
    s.set_option(KID_OPT_ENTRY_DEPTH, 1)
    for rule in [(0, 0), (2, 25)]:
        s.reset()
        db.read_fragment_votes(world.bases, world.off, min_hits=rule[0], min_permille=rule[1], tally=s)
        exp = dm.depth_of(fragment_csr(world.hits), world.vexp[rule], np.ones(world.nf, bool), world.keys.size)
        got = s.entry_depth()
        bad = np.flatnonzero(got != exp)
        assert bad.size == 0, "rule %s: entry %d: got %d, the model %d" % (rule, bad[0], got[bad[0]], exp[bad[0]])
    s.close()


# ------------------------------------------------------------------ 4. the device form and the timer
def test_device_form_on_what_read_hits_device_left(world, db):
    bases, off = world.bases, world.off
    n, nf = off.size - 1, world.nf
    total = int(world.hits.offsets[-1])
    db.read_fragment_votes_time()
    host = db.read_fragment_votes(bases, off, min_hits=2, min_permille=25)
    with DeviceBatch(bases, off, total) as d:
        d.run(db, total)
        d_out = d.dev(nf * 40, np.full(nf * 10, 0xA5A5A5A5, np.uint32))
        db.fragment_votes_from_hits_device(d.d_ho.value, d.d_hits.value, d.d_nk.value, n, d_out.value, min_hits=2, min_permille=25)
        _lib.check(d.lib.kid_dev_sync(0))
        got = d.down(d_out, np.uint32, nf * 10).view(FRAGMENT_VOTE_DTYPE)
        same_records(got, host, FRAGMENT_VOTE_DTYPE, "device form")
        same_records(got, world.vexp[(2, 25)], FRAGMENT_VOTE_DTYPE, "device form vs model")
    ms, calls, frags = db.read_fragment_votes_time()
    assert calls == 2 and frags == 2 * nf and ms > 0
    assert db.read_fragment_votes_time() == (0.0, 0, 0)


# ------------------------------------------------------------------ 5. errors, as kid_db_read_fragments* refuses them
def test_error_statuses(world, db):
    bases, off = world.bases, world.off[:201]
    assert status(lambda: db.read_fragment_votes(bases, off[:200])) == -1  # an odd number of reads
    assert status(lambda: db.read_fragment_votes(bases, off, min_permille=1001)) == -1
    assert db.read_fragment_votes(bases, off, min_permille=1000).size == 100
    assert db.read_fragment_votes(np.zeros(0, np.uint8), np.zeros(1, np.uint64)).size == 0  # no read at all
    other = KmerDB(world.keys[:1000], world.targets[:1000], world.parent, k=30, log2_slots=14)
    t_other, t = other.sample(), db.sample()
    assert status(lambda: db.read_fragment_votes(bases, off, tally=t_other)) == -1  # a sample of another kid_db
    db.read_fragment_votes(bases, off, tally=t)
    assert int(t.end()[0].sum()) == 100
    assert status(lambda: db.read_fragment_votes(bases, off, tally=t)) == -10  # after kid_sample_end without reset
    # the order: the rule is refused before the tally, the tally before the batch
    lib = _lib.load()
    lib.kid_db_read_fragment_votes(db._h, None, None, None, None, 3, 0, 1001, None, t._h)
    assert b"min_permille" in lib.kid_last_error()
    lib.kid_db_read_fragment_votes(db._h, None, None, None, None, 3, 0, 0, None, t._h)
    assert b"kid_sample_end" in lib.kid_last_error()
    t.reset()
    # a short quality line in block 2: refused, and nothing of the batch is counted
    f = world.where["6_8|"]
    seq = world.bases[int(world.off[2 * f]):int(world.off[2 * f + 1])].tobytes()
    t1, r1 = fastq_block([seq] * 4, [b"I" * len(seq)] * 4, eol=b"\r\n", blank_every=5)
    t2, r2 = fastq_block([seq] * 4, [b"I" * len(seq)] * 4)
    assert db.read_fragment_votes_fastq(t1, r1, t2, r2, tally=t).size == 4
    t.reset()
    bad = r2.copy()
    bad[2, 3] -= 1
    assert status(lambda: db.read_fragment_votes_fastq(t1, r1, t2, bad, tally=t)) == -9
    assert int(t.end()[0].sum()) == 0
    t.reset()
    # two blocks of 4 GiB together, and more fragments than a batch holds: refused before a byte is read
    out = np.zeros(4, FRAGMENT_VOTE_DTYPE)
    p = lambda a: a.ctypes.data  # noqa: E731
    assert lib.kid_db_read_fragment_votes_fastq(db._h, p(t1), 2 ** 31, p(r1), p(t2), 2 ** 31, p(r2), 4, 0, 0, p(out), None) == -1
    assert b"4 GiB" in lib.kid_last_error()
    assert lib.kid_db_read_fragment_votes_fastq(db._h, p(t1), t1.size, p(r1), p(t2), t2.size, p(r2), 2 ** 30, 0, 0, p(out), None) == -1
    assert lib.kid_db_read_fragment_votes(None, None, None, None, None, 0, 0, 0, None, None) == -1
    assert lib.kid_db_read_fragment_votes(db._h, None, None, None, None, 2, 0, 0, None, None) == -1  # null pointers
    assert lib.kid_db_read_fragment_votes_fastq(db._h, p(t1), t1.size, None, p(t2), t2.size, p(r2), 4, 0, 0, p(out), None) == -1
    assert lib.kid_db_read_fragment_votes_fastq(db._h, None, 0, None, None, 0, None, 0, 0, 0, None, None) == 0  # no fragment: nothing is launched
    assert lib.kid_db_fragment_votes_from_hits_device(db._h, None, None, None, 6, 0, 0, None, None) == -1
    assert lib.kid_db_read_fragment_votes_time(None, None, None, None) == -1
    for s in (t, t_other):
        s.close()
    other.close()


# ------------------------------------------------------------------ 6. the tally in every regime, the second kernel's included
@pytest.mark.parametrize("depth", [0, 1])
def test_tally_of_fragments_settled_by_every_regime(world, depth):
    """a genome-shaped database (every window of a random genome a key): a mate cut from it has a hit in every window, so
    fragments of a lane's, a wave's and a workgroup's size stand in one batch, and the sample counts all of them"""
    from read_fragments_model import interleave
    from read_hits_model import HitModel, windows
    from read_support_model import SupportModel
    from helpers import concat_reads, oracle_db
    combos = [(0, 0), (3, 4), (8, 0), (40, 30), (300, 300), (600, 0), (0, 600), (512, 1), (2, 2), (257, 256)]
    rng = np.random.default_rng(2020)
    parent = world.parent
    x = next(int(t) for t in world.targets if t > 1 and sc.top_level(parent, int(t)) != 5)
    g = rng.choice(sc.ACGT, 4000).tobytes()
    keys, _ = windows(g, 0, len(g) - 1, 30)
    tg = np.array([8, 6, 5, 36, 35, 8, 1, x], np.uint32)[rng.integers(0, 8, keys.size)]

    def dense(h):
        if h == 0:
            return b""
        p = int(rng.integers(0, len(g) - (h + 29)))
        return g[p:p + h + 29]

    m1, m2 = [dense(p) for p, _ in combos], [dense(q) for _, q in combos]
    bases, off = concat_reads(interleave(m1, m2))
    hm = HitModel(oracle_db(parent, keys, tg, 16), keys, tg, 30)
    fvm = FragmentVoteModel(VoteModel(SupportModel(hm, parent)))
    hits = hm.batch(bases, off)
    per = np.diff(hits.offsets.astype(np.int64))
    assert [(int(per[2 * j]), int(per[2 * j + 1])) for j in range(len(combos))] == combos  # from the model, before the library is asked
    counted = np.ones(len(combos), bool)
    d = KmerDB(keys, tg, parent, k=30, log2_slots=16)
    t = d.sample()
    t.set_option(KID_OPT_ENTRY_DEPTH, depth)
    for rule in [(0, 0), (200, 0), (2, 900)]:
        exp = fvm.batch_anc(hits, rule)
        t.reset()
        same_records(d.read_fragment_votes(bases, off, min_hits=rule[0], min_permille=rule[1], tally=t), exp, FRAGMENT_VOTE_DTYPE,
                     "depth %d rule %s" % (depth, rule))
        if depth:
            want = dm.depth_of(fragment_csr(hits), exp, counted, keys.size)
            got = t.entry_depth()
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, "rule %s: entry %d: got %d, the model %d" % (rule, bad[0], got[bad[0]], want[bad[0]])
        g_u = fvm.tally(hits, exp, counted, tg)
        assert int(g_u[0].sum()) == len(combos)
        assert ends_equal(t.end(), g_u), (depth, rule)
    assert len({int(c) for c in fvm.batch_anc(hits, (200, 0))["confident"]}) > 1  # the rule un-calls the small fragments alone
    t.close()
    d.close()
