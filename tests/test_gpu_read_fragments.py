"""kid_db_read_fragments* (mate pairs called as one fragment) against the independent model of
tests/read_fragments_model.py, against the classify and read-support paths of the same library, and against its own
contract.  Every comparison is exact: integers and bytes."""

import numpy as np
import pytest

import read_calls
import read_depth_model as dm
import read_fragments_cases as fc
import read_support_cases as sc
from helpers import DeviceBatch, concat_reads, fastq_block, oracle_db
from kmer_id_amd import (FRAGMENT_DTYPE, KID_DB_OPT_MIN_BASE_QUALITY, KID_FLAG_REF_GEOMETRY, KID_OPT_ENTRY_DEPTH, KID_OPT_MIN_BASE_QUALITY, KmerDB,
                         _lib)
from read_calls import KINDS, ends_equal, fastq_model, fastq_world, header_constant, same_records, status
from read_fragments_model import FragmentModel, fragment_csr, interleave
from read_hits_model import HitModel, windows
from read_support_model import SupportModel

pytestmark = pytest.mark.gpu

FIELDS = FRAGMENT_DTYPE.names
SUPPORT_FIELDS = FIELDS[:6]
LANE_HITS = header_constant("kid_support.hip.h", "KID_SUPPORT_LANE_HITS")


class World(read_calls.World):
    """a database, its models, a batch of 2 F interleaved reads and the model's records for every rule: computed once"""

    def __init__(self, parent, keys, targets, bases, off, log2_slots, rules=fc.RULES):
        super().__init__(parent, keys, targets, bases, off, log2_slots)
        self.fm = FragmentModel(self.sm)
        self.hits = self.hm.batch(bases, off)
        self.exp = {rule: self.fm.batch(self.hits, rule) for rule in rules}
        self.nf = (off.size - 1) // 2

    def check(self, db, what=""):
        for rule, exp in self.exp.items():
            same_records(db.read_fragments(self.bases, self.off, min_hits=rule[0], min_permille=rule[1]), exp, FRAGMENT_DTYPE,
                         "%s rule %s" % (what, rule))


@pytest.fixture(scope="module")
def world():
    parent, cum, keys, targets = sc.database()
    bases, off, where = fc.fragments(parent, cum, keys, targets)
    w = World(parent, keys, targets, bases, off, 20)
    w.where, w.cum = where, cum
    return w


@pytest.fixture(scope="module")
def db(world):
    return world.db()


# ------------------------------------------------------------------ 1. the model, three table kinds
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_all_eight_fields_equal_the_model(world, kind):
    e0 = world.exp[(0, 0)]
    a = e0[world.where["8|X_6"]]  # the non-associative case is among the fragments (tests/test_read_fragments_model.py: the rest)
    assert (int(a["final"]), int(a["final_1"]), int(a["final_2"])) == (6, 8, 1) and world.odb.msca(8, 1) == 8
    d = world.db(KINDS[kind])
    world.check(d, kind)
    d.close()


# ------------------------------------------------------------------ 2. work-split edges
def test_work_split_edges(world):
    L = LANE_HITS
    combos = [(0, 0), (0, 1), (1, 0), (L, 0), (0, L), (L - 1, 1), (1, L - 1), (L, 1), (1, L), (63, 1), (1, 63), (64, 0), (0, 64), (64, 1),
              (1, 64), (64, 64), (65, 63), (63, 65), (7, 200), (200, 7)]
    rng = np.random.default_rng(6464)
    parent = world.parent
    x = next(int(t) for t in world.targets if t > 1 and sc.top_level(parent, int(t)) != 5)
    g = rng.choice(sc.ACGT, 4000).tobytes()  # a genome-shaped database: every window of a random genome
    keys, _ = windows(g, 0, len(g) - 1, 30)
    tg = np.array([8, 6, 5, 36, 35, 8, 6, x], np.uint32)[rng.integers(0, 8, keys.size)]

    def dense(h):  # a stretch of the genome with h windows; none: no read at all
        if h == 0:
            return b""
        p = int(rng.integers(0, len(g) - (h + 29)))
        return g[p:p + h + 29]

    filler = lambda i: b"" if i % 3 == 0 else rng.choice(sc.ACGT, 100).tobytes()  # noqa: E731
    at = (0, 63, 64, 100)
    d = KmerDB(keys, tg, parent, k=30, log2_slots=16)
    hm = HitModel(oracle_db(parent, keys, tg, 16), keys, tg, 30)
    fm = FragmentModel(SupportModel(hm, parent))
    for i in range(0, len(combos), 4):  # batches of 130 fragments; fragments 0, 63, 64 and 100 of each are dense
        m1, m2 = [filler(2 * j) for j in range(130)], [filler(2 * j + 1) for j in range(130)]
        for j, (p, q) in zip(at, combos[i:i + 4]):
            m1[j], m2[j] = dense(p), dense(q)
        bases, off = concat_reads(interleave(m1, m2))
        hits = hm.batch(bases, off)
        per = np.diff(hits.offsets.astype(np.int64))
        assert [(int(per[2 * j]), int(per[2 * j + 1])) for j in at] == combos[i:i + 4]  # from the model, before the library is asked
        assert int(per.sum()) == sum(p + q for p, q in combos[i:i + 4])  # the fragments between have no hit
        for rule in fc.RULES:
            same_records(d.read_fragments(bases, off, min_hits=rule[0], min_permille=rule[1]), fm.batch(hits, rule), FRAGMENT_DTYPE,
                         "batch %d rule %s" % (i // 4, rule))
    d.close()


# ------------------------------------------------------------------ 3. trees without rows
@pytest.mark.parametrize("depth", [8, 12])
def test_hand_built_trees(depth):
    """depth 8: the deepest tree the ancestor rows hold; depth 12: the parent[] / depth[] path.  Mate 1 ends, and mate 2
    begins, at each depth of one lineage, with few hits (one lane) and with many (the whole wave)."""
    parent, spine, sibs = sc.chain_taxonomy(depth)
    rng = np.random.default_rng(100 + depth)
    nodes = spine + sibs
    tg = np.repeat(np.array(nodes, np.uint32), 4)
    keys = sc.random_keys(rng, tg.size)
    kseq = lambda node: sc.cases.key_seq(keys[nodes.index(node) * 4 + int(rng.integers(0, 4))], 30)  # noqa: E731
    rand = lambda n: [sc.cases.key_seq(keys[j], 30) for j in rng.integers(0, keys.size, n)]  # noqa: E731
    m1, m2 = [], []
    for a in spine:
        for b in spine:
            for extra in (1, LANE_HITS):
                m1.append(sc.implanted(rng, rand(extra) + [kseq(a)]))
                m2.append(sc.implanted(rng, [kseq(b)] + rand(extra)))
    bases, off = concat_reads(interleave(m1, m2))
    w = World(parent, keys, tg, bases, off, 12)
    per = np.diff(w.hits.offsets.astype(np.int64))
    assert int((per[0::2] + per[1::2]).max()) > LANE_HITS >= int((per[0::2] + per[1::2]).min())
    for flags in (0, KID_FLAG_REF_GEOMETRY):
        d = w.db(flags)
        assert d.info.tree_depth == depth
        w.check(d, "depth %d flags %d" % (depth, flags))
        d.close()


# ------------------------------------------------------------------ 4. cross-checks within the library
def test_per_mate_folds_are_what_classify_returns(world, db):
    got = db.read_fragments(world.bases, world.off)
    s = db.sample()
    finals = s.classify(world.bases, world.off)
    s.close()
    assert np.array_equal(got["final_1"], finals[0::2]) and np.array_equal(got["final_2"], finals[1::2])


def test_an_absent_mate_leaves_the_support_record_of_the_other(world, db):
    raw = bytes(world.bases)
    reads = [raw[int(world.off[i]):int(world.off[i + 1])] for i in range(world.off.size - 1)]
    alone = concat_reads(reads)
    first = concat_reads(interleave(reads, [b""] * len(reads)))
    second = concat_reads(interleave([b""] * len(reads), reads))
    for rule in [(0, 0), (2, 25)]:
        sup = db.read_support(*alone, min_hits=rule[0], min_permille=rule[1])
        a = db.read_fragments(*first, min_hits=rule[0], min_permille=rule[1])
        b = db.read_fragments(*second, min_hits=rule[0], min_permille=rule[1])
        for f in SUPPORT_FIELDS:
            assert np.array_equal(a[f], sup[f]) and np.array_equal(b[f], sup[f]), (rule, f)
        assert np.array_equal(a["final_1"], sup["final"]) and not a["final_2"].any()
        assert np.array_equal(b["final_2"], sup["final"]) and not b["final_1"].any()


# ------------------------------------------------------------------ 5. determinism
def test_records_repeat_and_do_not_depend_on_the_split_into_calls(world, db):
    a = db.read_fragments(world.bases, world.off, min_hits=2, min_permille=25)
    b = db.read_fragments(world.bases, world.off, min_hits=2, min_permille=25)
    assert a.tobytes() == b.tobytes()
    for cut in (1, 63, 64, 65):
        parts = [db.read_fragments(world.bases, world.off[:2 * cut + 1], min_hits=2, min_permille=25),
                 db.read_fragments(world.bases, world.off[2 * cut:], min_hits=2, min_permille=25)]
        assert np.concatenate(parts).tobytes() == a.tobytes(), cut


# ------------------------------------------------------------------ 6. the FASTQ form
@pytest.mark.parametrize("q", [0, 20])
def test_fastq_form(world, db, q):
    n, (s1, q1, t1, r1), (s2, q2, t2, r2) = fastq_world(world)
    hits, keep1, keep2 = fastq_model(world, (s1, q1), (s2, q2), q)
    assert (keep1 & ~keep2).sum() >= 20 and (~keep1 & keep2).sum() >= 20 and (~keep1 & ~keep2).sum() >= 20
    assert tuple(r2[9 + 200, [1, 3]]) == (0, 0)
    counted = keep1 | keep2
    if q:  # the mask changes what is found
        plain = fastq_model(world, (s1, q1), (s2, q2), 0)[0]
        assert int(plain.offsets[-1]) > int(hits.offsets[-1]) and int(plain.n_kmers.sum()) > int(hits.n_kmers.sum())
    db.set_option(KID_DB_OPT_MIN_BASE_QUALITY, q)
    try:
        for rule in [(0, 0), (2, 25)]:
            exp = world.fm.batch(hits, rule)
            t = db.sample()
            got = db.read_fragments_fastq(t1, r1[5:5 + n], t2, r2[9:9 + n], min_hits=rule[0], min_permille=rule[1], tally=t)
            same_records(got, exp, FRAGMENT_DTYPE, "q %d rule %s" % (q, rule))
            g, u = t.end()
            assert ends_equal((g, u), world.fm.tally(hits, exp, counted, world.targets)), (q, rule)
            assert int(g.sum()) == int(counted.sum()) < n
            t.close()
            if rule == (0, 0):  # ... and the unique k-mers are those of a sample that classified both blocks
                s = db.sample()
                s.set_option(KID_OPT_MIN_BASE_QUALITY, q)
                s.classify_fastq(t1, r1[5:5 + n])
                s.classify_fastq(t2, r2[9:9 + n])
                assert np.array_equal(s.end()[1], u)
                s.close()
    finally:
        db.set_option(KID_DB_OPT_MIN_BASE_QUALITY, 0)


# ------------------------------------------------------------------ 7. tally
def test_tally_under_rule_2_25_equals_the_model(world, db):
    t = db.sample()
    rec = db.read_fragments(world.bases, world.off, min_hits=2, min_permille=25, tally=t)
    exp = world.exp[(2, 25)]
    same_records(rec, exp, FRAGMENT_DTYPE)
    counted = np.ones(world.nf, bool)
    g, u = world.fm.tally(world.hits, exp, counted, world.targets)
    assert int(g.sum()) == world.nf and int(g[0]) > int((exp["final"] == 0).sum())  # once per fragment; the rule un-calls some
    before = t.stats()
    assert ends_equal(t.end(), (g, u))
    assert before == {"reads": 0, "lookups": 0, "probes": 0, "hits": 0}  # kid_sample_stats is not updated
    t.reset()
    assert db.read_fragments(world.bases, world.off, tally=t).size == world.nf  # after a reset the sample counts from nothing
    assert ends_equal(t.end(), world.fm.tally(world.hits, world.exp[(0, 0)], counted, world.targets))
    t.close()


def test_depth_counts_every_hit_of_both_mates(world, db):
    s = db.sample()
    s.set_option(KID_OPT_ENTRY_DEPTH, 1)
    for rule in [(0, 0), (2, 25)]:
        s.reset()
        db.read_fragments(world.bases, world.off, min_hits=rule[0], min_permille=rule[1], tally=s)
        exp = dm.depth_of(fragment_csr(world.hits), world.exp[rule], np.ones(world.nf, bool), world.keys.size)
        got = s.entry_depth()
        bad = np.flatnonzero(got != exp)
        assert bad.size == 0, "rule %s: entry %d: got %d, the model %d" % (rule, bad[0], got[bad[0]], exp[bad[0]])
    # a k-mer present in both mates counts 2: a batch of that one fragment alone
    f = world.where["same_kmer"]
    off = world.off[2 * f:2 * f + 3]
    s.reset()
    db.read_fragments(world.bases, off, tally=s)
    got = s.entry_depth()
    ent = np.concatenate([world.hits.of(2 * f)[2], world.hits.of(2 * f + 1)[2]])
    twice = [int(e) for e in np.unique(ent) if (ent == e).sum() == 2]
    assert len(twice) == 1 and int(got[twice[0]]) == 2 and int(got.sum()) == ent.size
    s.close()


# ------------------------------------------------------------------ 8. the device form
def test_device_form_equals_host_form(world, db):
    bases, off = world.bases, world.off
    n, nf = off.size - 1, world.nf
    total = int(world.hits.offsets[-1])
    host = db.read_fragments(bases, off, min_hits=2, min_permille=25)
    db.read_fragments_time()
    with DeviceBatch(bases, off, total) as d:
        d.run(db, total)
        d_out = d.dev(nf * 32, np.full(nf * 8, 0xA5A5A5A5, np.uint32))
        db.fragments_from_hits_device(d.d_ho.value, d.d_hits.value, d.d_nk.value, n, d_out.value, min_hits=2, min_permille=25)
        _lib.check(d.lib.kid_dev_sync(0))
        got = d.down(d_out, np.uint32, nf * 8).view(FRAGMENT_DTYPE)
        same_records(got, host, FRAGMENT_DTYPE, "device form")
        same_records(got, world.exp[(2, 25)], FRAGMENT_DTYPE, "device form vs model")
        # the same batch in three calls (offsets stay absolute: the hits pointer is the same)
        d_out3 = d.dev(nf * 32, np.full(nf * 8, 0xA5A5A5A5, np.uint32))
        cuts = [0, nf // 3, nf // 3 + 65, nf]
        for a, b in zip(cuts[:-1], cuts[1:]):
            db.fragments_from_hits_device(d.d_ho.value + 16 * a, d.d_hits.value, d.d_nk.value + 8 * a, 2 * (b - a), d_out3.value + 32 * a,
                                          min_hits=2, min_permille=25)
        _lib.check(d.lib.kid_dev_sync(0))
        assert d.down(d_out3, np.uint32, nf * 8).tobytes() == got.tobytes()
        ms, calls, frags = db.read_fragments_time()
        assert calls == 4 and frags == 2 * nf and ms > 0
        assert db.read_fragments_time() == (0.0, 0, 0)


# ------------------------------------------------------------------ 9. errors
def test_error_statuses(world, db):
    bases, off = world.bases, world.off[:201]
    assert status(lambda: db.read_fragments(bases, off[:200])) == -1  # an odd number of reads
    assert status(lambda: db.read_fragments(bases, off, min_permille=1001)) == -1
    assert db.read_fragments(bases, off, min_permille=1000).size == 100
    assert db.read_fragments(np.zeros(0, np.uint8), np.zeros(1, np.uint64)).size == 0  # no read at all
    other = KmerDB(world.keys[:1000], world.targets[:1000], world.parent, k=30, log2_slots=14)
    t_other, t = other.sample(), db.sample()
    assert status(lambda: db.read_fragments(bases, off, tally=t_other)) == -1  # a sample of another kid_db
    db.read_fragments(bases, off, tally=t)
    first = t.end()
    assert int(first[0].sum()) == 100
    assert status(lambda: db.read_fragments(bases, off, tally=t)) == -10  # after kid_sample_end without reset
    t.reset()
    # a short quality line in block 2: refused, and nothing of the batch is counted
    f = world.where["6_8|"]
    seq = world.bases[int(world.off[2 * f]):int(world.off[2 * f + 1])].tobytes()
    t1, r1 = fastq_block([seq] * 4, [b"I" * len(seq)] * 4, eol=b"\r\n", blank_every=5)
    t2, r2 = fastq_block([seq] * 4, [b"I" * len(seq)] * 4)
    assert db.read_fragments_fastq(t1, r1, t2, r2, tally=t).size == 4
    t.reset()
    r2[2, 3] -= 1
    assert status(lambda: db.read_fragments_fastq(t1, r1, t2, r2, tally=t)) == -9
    assert int(t.end()[0].sum()) == 0
    lib = _lib.load()
    assert lib.kid_db_read_fragments(None, None, None, None, None, 0, 0, 0, None, None) == -1
    assert lib.kid_db_read_fragments(db._h, None, None, None, None, 2, 0, 0, None, None) == -1  # null pointers
    assert lib.kid_db_read_fragments_fastq(db._h, None, 0, None, None, 0, None, 0, 0, 0, None, None) == 0  # no fragment: nothing is launched
    assert lib.kid_db_fragments_from_hits_device(db._h, None, None, None, 6, 0, 0, None, None) == -1
    assert lib.kid_db_fragments_from_hits_device(db._h, None, None, None, 5, 0, 0, None, None) == -1
    assert lib.kid_db_fragments_from_hits_device(db._h, None, None, None, 0, 0, 1001, None, None) == -1
    for s in (t, t_other):
        s.close()
    other.close()
