"""kid_db_read_support* (reads called by k-mer support) against the independent model of tests/read_support_model.py,
against the classify path of the same library, and against its own contract.  Every comparison is exact: integers."""

import numpy as np
import pytest

import read_calls
import read_support_cases as sc
from helpers import DeviceBatch, concat_reads, fastq_block, oracle_db
from kmer_id_amd import KID_FLAG_REF_GEOMETRY, KmerDB, _lib, end_merged
from kmer_id_amd.api import SUPPORT_DTYPE
from read_calls import KINDS, ends_equal, genome_world, header_constant, same_records, status
from read_hits_model import HitModel, trim_ranges
from read_support_model import RULES, SupportModel

pytestmark = pytest.mark.gpu

FIELDS = SUPPORT_DTYPE.names
LANE_HITS = header_constant("kid_support.hip.h", "KID_SUPPORT_LANE_HITS")


class World(read_calls.World):
    """a database, its model, a batch of reads and the model's records for every rule of the grid: computed once"""

    def __init__(self, parent, keys, targets, bases, off, log2_slots, rules=RULES):
        super().__init__(parent, keys, targets, bases, off, log2_slots)
        self.model = self.sm
        self.hits = self.hm.batch(bases, off)
        self.finals = self.model.finals(self.hits)
        self.exp = {rule: self.model.batch_identity(self.hits, rule, self.finals) for rule in rules}

    def check(self, db, what=""):
        """every rule's records equal the model's, and `final` equals kid_classify_batch's per-read output"""
        for rule, exp in self.exp.items():
            same_records(db.read_support(self.bases, self.off, min_hits=rule[0], min_permille=rule[1]), exp, SUPPORT_DTYPE,
                         "%s rule %s" % (what, rule))
        s = db.sample()
        assert np.array_equal(s.classify(self.bases, self.off), self.finals), what
        s.close()


@pytest.fixture(scope="module")
def world():
    parent, cum, keys, targets = sc.database()
    bases, off, where = sc.reads(parent, cum, keys, targets)
    w = World(parent, keys, targets, bases, off, 20)
    w.where, w.cum = where, cum
    return w


@pytest.fixture(scope="module")
def db(world):
    return world.db()


# ------------------------------------------------------------------ 1. (and 4.) the model, three table kinds
def test_no_outcome_is_missing_from_the_cases(world):
    seen = set()
    for rule, e in world.exp.items():
        f, c = e["final"].astype(np.int64), e["confident"].astype(np.int64)
        anc = np.array([c[r] > 1 and c[r] != f[r] and world.model.under(f[r], c[r]) for r in range(f.size)])
        seen |= {name for name, m in (("same", (c == f) & (f > 1)), ("ancestor", anc), ("root", (f > 1) & (c == 1)),
                                      ("none", (f > 0) & (c == 0))) if m.any()}
    assert seen == {"same", "ancestor", "root", "none"}
    e3 = world.exp[(3, 0)]
    assert (int(e3[world.where["6_36_8"]]["final"]), int(e3[world.where["6_36_8"]]["confident"])) == (8, 5)
    assert (int(e3[world.where["X_8_6"]]["final"]), int(e3[world.where["X_8_6"]]["confident"])) == (6, 1)
    r = world.hits.of(world.where["root_only"])[1]
    assert r.size == 3 and np.all(r == 1)
    assert np.array_equal(world.exp[(0, 0)]["confident"], world.finals)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_all_six_fields_equal_the_model(world, kind):
    d = world.db(KINDS[kind])
    world.check(d, kind)
    d.close()


def test_records_repeat_byte_for_byte(world, db):
    a = db.read_support(world.bases, world.off, min_hits=2, min_permille=25)
    b = db.read_support(world.bases, world.off, min_hits=2, min_permille=25)
    assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ 2. work-split edges
def test_work_split_edges(world):
    rng = np.random.default_rng(64)
    parent = world.parent
    x = next(int(t) for t in world.targets if t > 1 and sc.top_level(parent, int(t)) != 5)
    g, keys, tg = genome_world(rng, [8, 6, 5, 36, 35, 8, 6, x], 4000, 1)
    counts = [LANE_HITS - 1, LANE_HITS, LANE_HITS + 1, 63, 64, 65, 200]
    rules = [(0, 0), (3, 0), (2, 25), (0, 1000)]

    def dense(h):
        p = int(rng.integers(0, len(g) - (h + 29)))
        return g[p:p + h + 29]

    filler = lambda i: b"" if i % 2 else rng.choice(sc.ACGT, 100).tobytes()  # noqa: E731
    seqs = []
    for i in range(len(counts)):  # batches of 130 reads back to back; reads 0, 63, 64 of each are dense
        batch = [filler(j) for j in range(130)]
        batch[0], batch[63], batch[64] = dense(counts[i]), dense(counts[(i + 1) % 7]), dense(counts[(i + 2) % 7])
        batch[100] = dense(counts[(i + 3) % 7])
        seqs.append(batch)
    d = KmerDB(keys, tg, parent, k=30, log2_slots=16)
    odb = oracle_db(parent, keys, tg, 16)
    hm = HitModel(odb, keys, tg, 30)
    model = SupportModel(hm, parent)
    for i, batch in enumerate(seqs):
        bases, off = concat_reads(batch)
        hits = hm.batch(bases, off)
        per = np.diff(hits.offsets.astype(np.int64))
        assert [int(per[j]) for j in (0, 63, 64)] == [counts[i], counts[(i + 1) % 7], counts[(i + 2) % 7]] and int(per[1]) == 0
        finals = model.finals(hits)
        for rule in rules:
            same_records(d.read_support(bases, off, min_hits=rule[0], min_permille=rule[1]), model.batch_identity(hits, rule, finals), SUPPORT_DTYPE,
                         "batch %d rule %s" % (i, rule))
        s = d.sample()
        assert np.array_equal(s.classify(bases, off), finals)
        s.close()
    # no read at all; 65 reads without a hit
    assert d.read_support(np.zeros(0, np.uint8), np.zeros(1, np.uint64)).size == 0
    bases, off = concat_reads([filler(j) for j in range(65)])
    got = d.read_support(bases, off, min_hits=1)
    assert not got["final"].any() and not got["confident"].any() and not got["n_hits"].any() and int(got["n_kmers"].sum()) == 33 * 71
    d.close()


def test_a_record_of_70000_windows(world):
    rng = np.random.default_rng(70000)
    parent = world.parent
    g, keys, tg = genome_world(rng, [8, 6, 5, 36, 35, 5, 5, 1], 70029, 20)
    short = [rng.choice(sc.ACGT, 150).tobytes() for _ in range(5)]
    bases, off = concat_reads(short[:2] + [g] + short[2:] + [g[1000:1000 + 29 + 40]])
    w = World(parent, keys, tg, bases, off, 16, rules=[(0, 0), (3000, 0), (0, 50), (0, 60), (2, 25)])
    assert int(w.hits.n_kmers[2]) == 70000 and 3000 <= int(np.diff(w.hits.offsets.astype(np.int64))[2]) <= 4000
    assert len({int(e["confident"][2]) for e in w.exp.values()}) >= 2  # the rules tell the record's lineage apart
    d = w.db()
    w.check(d, "long record")
    d.close()


# ------------------------------------------------------------------ 3. trees
@pytest.mark.parametrize("depth", [8, 12])
def test_hand_built_trees(depth):
    """depth 8: the deepest tree the ancestor rows hold (depth-8 nodes are not stored in their own row); depth 12: the
    parent[] / depth[] path.  Reads of 1 .. 14 implanted k-mers: both work splits."""
    parent, spine, sibs = sc.chain_taxonomy(depth)
    rng = np.random.default_rng(depth)
    nodes = spine + sibs
    tg = np.repeat(np.array(nodes, np.uint32), 4)
    keys = sc.random_keys(rng, tg.size)
    kseq = lambda node, j=0: sc.cases.key_seq(keys[nodes.index(node) * 4 + j], 30)  # noqa: E731
    deep, deep_sib, above = spine[-1], sibs[-1], spine[-2]
    seqs = [sc.implanted(rng, [kseq(deep)]),                                    # a node at the deepest level is final
            sc.implanted(rng, [kseq(deep), kseq(deep, 1), kseq(above)]),
            sc.implanted(rng, [kseq(deep), kseq(deep_sib)]),                      # ... is a hit under a final one level up
            sc.implanted(rng, [kseq(deep_sib), kseq(deep)] * 6)]                  # the same with the whole wave
    for _ in range(200):
        pick = rng.integers(0, keys.size, int(rng.integers(1, 15)))
        seqs.append(sc.implanted(rng, [sc.cases.key_seq(keys[j], 30) for j in pick]))
    bases, off = concat_reads(seqs)
    w = World(parent, keys, tg, bases, off, 12)
    assert int(w.finals[0]) == deep and int(w.finals[2]) == above and int(w.finals[3]) == above
    assert int(w.exp[(2, 0)][2]["s_final"]) == 2 and int(w.exp[(2, 0)][2]["confident"]) == above
    assert int(np.diff(w.hits.offsets.astype(np.int64)).max()) > LANE_HITS
    for flags in (0, KID_FLAG_REF_GEOMETRY):
        d = w.db(flags)
        assert d.info.tree_depth == depth
        w.check(d, "depth %d flags %d" % (depth, flags))
        d.close()


# ------------------------------------------------------------------ 5. tally
def adversarial(world):
    n = 600  # the first 600 reads of the world are the adversarial ones: 0 .. 300 bytes, whole-read ranges
    return world.bases[:int(world.off[n])], world.off[:n + 1]


def test_tally_under_rule_00_equals_classifying(world, db):
    bases, off = adversarial(world)
    assert int((np.diff(off.astype(np.int64)) < 30).sum()) > 20  # reads shorter than k: counted under target 0
    s, t = db.sample(), db.sample()
    s.classify(bases, off)
    rec = db.read_support(bases, off, tally=t)
    same_records(rec, world.exp[(0, 0)][:600], SUPPORT_DTYPE)
    g, u = t.end()
    assert ends_equal((g, u), s.end()) and int(g.sum()) == 600 and int(u.sum()) > 100
    s.close(), t.close()


def test_tally_of_a_fastq_block_counts_what_classifying_counts(world, db):
    from kmer_id_amd import synth
    n, length = 1200, 150
    bases, off = sc.cases.synth_reads(world.cum, world.parent, n, length)
    quals = [q.tobytes() for q in synth.qualities(n, length)]
    seqs = [bases[i * length:(i + 1) * length].tobytes() for i in range(n)]
    seqs += [b"ACGT" * 5, b"", seqs[3][:31]]  # records too short for a k-mer
    quals += [b"I" * 20, b"", b"I" * 31]
    start, stop, keep = trim_ranges(quals, [len(s) for s in seqs], 30)
    assert 0 < int((~keep).sum()) and int(keep.sum()) > 800
    text, recs = fastq_block(seqs, quals, eol=b"\r\n", blank_every=5)  # CRLF line ends, blank lines between records
    s, t = db.sample(), db.sample()
    final, st, sp = s.classify_fastq(text, recs)
    rec = db.read_support_fastq(text, recs, tally=t)
    assert np.array_equal(rec["final"], final) and np.array_equal(rec["confident"], final)
    assert np.array_equal(st, start) and np.all(rec["n_kmers"][~keep] == 0)
    g, u = t.end()
    assert ends_equal((g, u), s.end()) and int(g.sum()) == int(keep.sum())  # a dropped record is counted nowhere
    s.close(), t.close()


def test_classify_and_tally_mix_in_one_sample_and_merge(world, db):
    bases, off = world.bases, world.off
    n = off.size - 1
    cut = n // 3
    whole = db.sample()
    whole.classify(bases, off)
    ref = whole.end()
    mixed = db.sample()
    mixed.classify(bases, off[:cut + 1])
    db.read_support(bases, off[cut:], tally=mixed)
    assert ends_equal(mixed.end(), ref)
    # two tallied samples closed together equal one
    a, b = db.sample(), db.sample()
    db.read_support(bases, off[:cut + 1], tally=a)
    db.read_support(bases, off[cut:], tally=b)
    assert ends_equal(end_merged([a, b]), ref)
    for s in (whole, mixed, a, b):
        s.close()


def test_tally_under_rule_2_25_equals_the_model(world, db):
    t = db.sample()
    rec = db.read_support(world.bases, world.off, min_hits=2, min_permille=25, tally=t)
    exp = world.exp[(2, 25)]
    same_records(rec, exp, SUPPORT_DTYPE)
    g, u = world.model.tally(world.hits, exp, np.ones(exp.size, bool), world.targets)
    assert int(g[0]) > int((world.finals == 0).sum())  # the rule un-calls reads
    before = t.stats()
    assert ends_equal(t.end(), (g, u))
    assert before == {"reads": 0, "lookups": 0, "probes": 0, "hits": 0}  # kid_sample_stats is not updated by a tally
    t.reset()
    db.read_support(world.bases, world.off, tally=t)  # after a reset the sample counts from nothing
    g0, u0 = world.model.tally(world.hits, world.exp[(0, 0)], np.ones(exp.size, bool), world.targets)
    assert ends_equal(t.end(), (g0, u0))
    t.close()


# ------------------------------------------------------------------ 6. the device form
def test_device_form_equals_host_form(world, db):
    bases, off = world.bases, world.off
    n = off.size - 1
    total = int(world.hits.offsets[-1])
    host = db.read_support(bases, off, min_hits=2, min_permille=25)
    db.read_support_time()
    with DeviceBatch(bases, off, total) as d:
        d.run(db, total)
        d_out = d.dev(n * 24, np.full(n * 6, 0xA5A5A5A5, np.uint32))
        db.support_from_hits_device(d.d_ho.value, d.d_hits.value, d.d_nk.value, n, d_out.value, min_hits=2, min_permille=25)
        _lib.check(d.lib.kid_dev_sync(0))
        got = d.down(d_out, np.uint32, n * 6).view(SUPPORT_DTYPE)
        same_records(got, host, SUPPORT_DTYPE, "device form")
        same_records(got, world.exp[(2, 25)], SUPPORT_DTYPE, "device form vs model")
        # the same batch in three calls (offsets stay absolute: the hits pointer is the same)
        d_out3 = d.dev(n * 24, np.full(n * 6, 0xA5A5A5A5, np.uint32))
        cuts = [0, n // 3, n // 3 + 65, n]
        for a, b in zip(cuts[:-1], cuts[1:]):
            db.support_from_hits_device(d.d_ho.value + 8 * a, d.d_hits.value, d.d_nk.value + 4 * a, b - a, d_out3.value + 24 * a,
                                        min_hits=2, min_permille=25)
        _lib.check(d.lib.kid_dev_sync(0))
        assert d.down(d_out3, np.uint32, n * 6).tobytes() == got.tobytes()
        ms, calls, reads = db.read_support_time()
        assert calls == 4 and reads == 2 * n and ms > 0
        assert db.read_support_time() == (0.0, 0, 0)


# ------------------------------------------------------------------ 7. errors
def test_error_statuses(world, db):
    bases, off = adversarial(world)

    assert status(lambda: db.read_support(bases, off, min_permille=1001)) == -1
    assert db.read_support(bases, off, min_permille=1000).size == 600
    other = KmerDB(world.keys[:1000], world.targets[:1000], world.parent, k=30, log2_slots=14)
    t_other, t = other.sample(), db.sample()
    assert status(lambda: db.read_support(bases, off, tally=t_other)) == -1  # a sample of another kid_db
    db.read_support(bases, off, tally=t)
    first = t.end()
    assert status(lambda: db.read_support(bases, off, tally=t)) == -10  # after kid_sample_end without reset
    t.reset()
    db.read_support(bases, off, tally=t)
    assert ends_equal(t.end(), first)
    # what kid_db_read_hits reports, reported the same way -- and nothing of a refused batch is counted
    t.reset()
    bad = off[:10].copy()
    bad[4] = bad[3] - np.uint64(1)
    assert status(lambda: db.read_support(bases, bad, tally=t)) == -1
    n = 9
    start, stop = np.zeros(n, np.int32), (np.diff(off[:n + 1].astype(np.int64)) - 1).astype(np.int32)
    stop[2] += 1  # one past the read
    assert status(lambda: db.read_support(bases, off[:n + 1], start, stop, tally=t)) == -1
    text, recs = fastq_block([bases[int(off[3]):int(off[4])].tobytes()] * 4, [b"I" * int(off[4] - off[3])] * 4, eol=b"\r\n", blank_every=5)
    recs[2, 3] -= 1  # a quality line shorter than its sequence
    assert status(lambda: db.read_support_fastq(text, recs, tally=t)) == -9
    assert int(t.end()[0].sum()) == 0
    lib = _lib.load()
    assert lib.kid_db_read_support(db._h, None, None, None, None, 1 << 31, 0, 0, None, None) == -1  # more than 2^31-1 reads
    assert lib.kid_db_read_support(None, None, None, None, None, 0, 0, 0, None, None) == -1
    assert lib.kid_db_support_from_hits_device(db._h, None, None, None, 5, 0, 0, None, None) == -1
    assert lib.kid_db_support_from_hits_device(db._h, None, None, None, 0, 0, 1001, None, None) == -1
    for s in (t, t_other):
        s.close()
    other.close()
