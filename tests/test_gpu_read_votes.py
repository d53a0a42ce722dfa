"""kid_db_read_votes* (reads called by root-path votes) against the independent model of tests/read_votes_model.py and
against its own contract: a record that does not depend on the order of a read's hits.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import read_calls
import read_depth_model as dm
import read_support_cases as sc
import read_votes_cases as vc
from helpers import DeviceBatch, concat_reads, fastq_block, oracle_db
from kmer_id_amd import KID_FLAG_REF_GEOMETRY, KID_OPT_ENTRY_DEPTH, VOTE_DTYPE, KmerDB, _lib
from read_calls import KINDS, ends_equal, header_constant, same_records, seen_bits, status
from read_hits_model import HitModel, Hits, trim_ranges, windows
from read_support_model import RULES, SupportModel
from read_votes_model import VoteModel

pytestmark = pytest.mark.gpu

FIELDS = VOTE_DTYPE.names
LANE_HITS = header_constant("kid_votes.hip.h", "KID_VOTE_LANE_HITS")
WAVE_HITS = header_constant("kid_votes.hip.h", "KID_VOTE_WAVE_HITS")
EDGE_RULES = [(0, 0), (3, 0), (2, 25), (0, 1000)]


class World(read_calls.World):
    """a database, its models, a batch of reads and the model's records for every rule of the grid: computed once"""

    def __init__(self, parent, keys, targets, bases, off, log2_slots, rules=RULES):
        super().__init__(parent, keys, targets, bases, off, log2_slots)
        self.vm = VoteModel(self.sm)
        self.hits = self.hm.batch(bases, off)
        calls = self.vm.calls_anc(self.hits)
        self.exp = {rule: self.vm.batch_anc(self.hits, rule, calls) for rule in rules}

    def check(self, db, what=""):
        for rule, exp in self.exp.items():
            same_records(db.read_votes(self.bases, self.off, min_hits=rule[0], min_permille=rule[1]), exp, VOTE_DTYPE, "%s rule %s" % (what, rule))


@pytest.fixture(scope="module")
def world():
    parent, cum, keys, targets = sc.database()
    bases, off, where, x = vc.reads(parent, cum, keys, targets)
    w = World(parent, keys, targets, bases, off, 20)
    w.where, w.cum, w.x = where, cum, x
    return w


@pytest.fixture(scope="module")
def db(world):
    return world.db()


# ------------------------------------------------------------------ 1. the model, three table kinds, two tree forms
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_all_eight_fields_equal_the_model(world, kind):
    d = world.db(KINDS[kind])
    world.check(d, kind)
    d.close()


def test_the_worked_cases(world, db):
    got = db.read_votes(world.bases, world.off)
    call = lambda name: (int(got[world.where[name]]["call"]), int(got[world.where[name]]["p_best"]), int(got[world.where[name]]["n_best"]))  # noqa: E731
    assert call("6_8") == (8, 2, 1) and call("X_8_6") == (8, 2, 1) and call("v_8_36") == (5, 1, 2) and call("v_X_8") == (1, 1, 2)
    assert call("v_1_X") == (world.x, 2, 1) and call("v_8_8_36_36_X") == (5, 2, 2)
    assert np.array_equal(got["confident"], got["call"])


def test_a_tree_of_depth_12_takes_the_parent_climb():
    parent, spine, sibs = sc.chain_taxonomy(12)
    rng = np.random.default_rng(12)
    nodes = spine + sibs
    tg = np.repeat(np.array(nodes, np.uint32), 4)
    keys = sc.random_keys(rng, tg.size)
    seqs = []
    for n_implanted in list(range(1, 15)) * 12 + [70, 90]:  # both work splits of the first kernel
        pick = rng.integers(0, keys.size, n_implanted)
        seqs.append(sc.implanted(rng, [sc.cases.key_seq(keys[j], 30) for j in pick], gap=1))
    bases, off = concat_reads(seqs)
    w = World(parent, keys, tg, bases, off, 12)
    per = np.diff(w.hits.offsets.astype(np.int64))
    assert int(per.max()) > 64 and int((per <= LANE_HITS).sum()) > 50
    e = w.exp[(0, 0)]
    assert ((e["n_best"] > 1) & (e["call"] > 1)).any() and ((e["n_best"] > 1) & (e["call"] == 1)).any() and (e["n_best"] == 1).any()
    for flags in (0, KID_FLAG_REF_GEOMETRY):
        d = w.db(flags)
        assert d.info.tree_depth == 12
        w.check(d, "depth 12 flags %d" % flags)
        d.close()


def test_records_repeat_byte_for_byte(world, db):
    a = db.read_votes(world.bases, world.off, min_hits=2, min_permille=25)
    b = db.read_votes(world.bases, world.off, min_hits=2, min_permille=25)
    assert a.tobytes() == b.tobytes()


def test_the_reverse_complement_of_every_read_has_the_same_record(world, db):
    """a property that needs no model: the lookup is canonical, so the hits are the same in opposite order"""
    rc = vc.reverse_complement(world.bases, world.off)
    assert not np.array_equal(rc, world.bases)
    for rule in [(0, 0), (2, 25)]:
        fwd = db.read_votes(world.bases, world.off, min_hits=rule[0], min_permille=rule[1])
        rev = db.read_votes(rc, world.off, min_hits=rule[0], min_permille=rule[1])
        assert fwd.tobytes() == rev.tobytes(), rule
    s = db.read_support(world.bases, world.off)["final"]
    assert (s != db.read_support(rc, world.off)["final"]).any()  # ... which `final` does not survive


# ------------------------------------------------------------------ 2. work-split edges
class Dense:
    """a database of every window of a random genome under targets drawn from a lineage list: a stretch of h + 29 bases
    of the genome is a read with exactly h hits.  The list: the nodes of 5 -> 6 -> 8, 5 -> 35 -> 36 and X `core` times
    each, and 80 other nodes once each.  core = 10: a read's votes gather on one lineage, as a real read's do; core = 1:
    flat, so that a read of hundreds of hits often has several best nodes, under the root and under inner nodes."""

    def __init__(self, world, seed=64, genome_len=9000, core=10):
        self.rng = rng = np.random.default_rng(seed)
        self.parent = world.parent
        others = [int(t) for t in np.unique(world.targets) if t > 1 and int(t) not in (5, 6, 8, 35, 36, world.x)][:80]
        assert len(others) == 80
        lineage = np.array([8, 6, 5, 36, 35, 8, 6, world.x] * core + others, np.uint32)
        self.g = rng.choice(sc.ACGT, genome_len).tobytes()
        self.keys, _ = windows(self.g, 0, genome_len - 1, 30)
        self.tg = lineage[rng.integers(0, lineage.size, self.keys.size)]
        self.hm = HitModel(oracle_db(self.parent, self.keys, self.tg, 16), self.keys, self.tg, 30)
        self.sm = SupportModel(self.hm, self.parent)
        self.vm = VoteModel(self.sm)
        self.db = KmerDB(self.keys, self.tg, self.parent, k=30, log2_slots=16)

    def read(self, h):
        p = int(self.rng.integers(0, len(self.g) - (h + 29)))
        return self.g[p:p + h + 29]

    def filler(self, i):
        return b"" if i % 2 else self.rng.choice(sc.ACGT, 100).tobytes()

    def model(self, bases, off, rules=EDGE_RULES):
        hits = self.hm.batch(bases, off)
        calls = self.vm.calls_anc(hits)
        return hits, {rule: self.vm.batch_anc(hits, rule, calls) for rule in rules}

    def check(self, bases, off, exp, what):
        for rule, e in exp.items():
            same_records(self.db.read_votes(bases, off, min_hits=rule[0], min_permille=rule[1]), e, VOTE_DTYPE, "%s rule %s" % (what, rule))


@pytest.fixture(scope="module")
def dense(world):
    d = Dense(world)
    yield d
    d.db.close()


@pytest.fixture(scope="module")
def flat(world):
    d = Dense(world, seed=65, core=1)
    yield d
    d.db.close()


@pytest.fixture(scope="module")
def big_batch(flat):
    dense = flat
    """more reads for the second kernel than it has workgroups (one per compute unit: 256 on an MI355X, 304 on an
    MI300X): 320 reads of WAVE + 1 .. WAVE + 90 hits, nothing else -- the first and the last index of the batch included"""
    bases, off = concat_reads([dense.read(WAVE_HITS + 1 + i % 90) for i in range(320)])
    hits, exp = dense.model(bases, off, [(0, 0), (2, 25)])
    assert int(np.diff(hits.offsets.astype(np.int64)).min()) == WAVE_HITS + 1
    e = exp[(0, 0)]
    assert int(((e["n_best"] > 1) & (e["call"] > 1)).sum()) >= 5 and int(((e["n_best"] > 1) & (e["call"] == 1)).sum()) >= 5
    assert int((e["n_best"] == 1).sum()) >= 100
    return bases, off, hits, exp


def test_work_split_edges(dense):
    counts = [LANE_HITS - 1, LANE_HITS, LANE_HITS + 1, 63, 64, 65, WAVE_HITS - 1, WAVE_HITS, WAVE_HITS + 1]
    nc = len(counts)
    for i in range(nc):  # batches of 130 reads; reads 0, 63, 64, 100 and 129 of each are dense
        batch = [dense.filler(j) for j in range(130)]
        for slot, c in zip((0, 63, 64, 100, 129), range(i, i + 5)):
            batch[slot] = dense.read(counts[c % nc])
        bases, off = concat_reads(batch)
        hits, exp = dense.model(bases, off)
        per = np.diff(hits.offsets.astype(np.int64))
        assert [int(per[j]) for j in (0, 63, 64)] == [counts[i], counts[(i + 1) % nc], counts[(i + 2) % nc]] and int(per[1]) == 0
        dense.check(bases, off, exp, "batch %d" % i)
    # no read at all; 65 reads without a hit (a batch with nothing for either regime above the lane's)
    assert dense.db.read_votes(np.zeros(0, np.uint8), np.zeros(1, np.uint64)).size == 0
    bases, off = concat_reads([dense.filler(j) for j in range(65)])
    got = dense.db.read_votes(bases, off, min_hits=1)
    assert not got["call"].any() and not got["confident"].any() and not got["n_hits"].any() and not got["p_best"].any()
    assert int(got["n_kmers"].sum()) == 33 * 71


@pytest.mark.parametrize("which", ["dense", "flat"])
def test_one_read_of_4000_hits_over_many_targets(dense, flat, which):
    dense = {"dense": dense, "flat": flat}[which]
    seqs = [dense.filler(0), dense.read(4000), dense.read(3), dense.read(700)]
    bases, off = concat_reads(seqs)
    hits, exp = dense.model(bases, off)
    assert int(np.diff(hits.offsets.astype(np.int64))[1]) == 4000 and np.unique(hits.of(1)[1]).size > 64
    assert which == "flat" or len({int(e["confident"][1]) for e in exp.values()}) >= 2
    dense.check(bases, off, exp, "4000 hits")


def test_more_big_reads_than_workgroups_and_clean_rows_between_calls(flat, big_batch):
    dense = flat
    bases, off, hits, exp = big_batch
    dense.check(bases, off, exp, "big only")
    dense.check(bases, off, exp, "big only, again")  # the rows are zero again behind every read
    other, ooff = concat_reads([dense.read(WAVE_HITS + 200 + 7 * i) for i in range(40)] + [dense.read(5), dense.read(100)])
    _, oexp = dense.model(other, ooff)
    dense.check(other, ooff, oexp, "other big reads behind them")


def test_splits_of_a_batch_into_calls_give_the_same_bytes(dense):
    batch = [dense.filler(j) for j in range(130)]
    for slot, h in ((0, WAVE_HITS + 5), (1, 64), (62, LANE_HITS + 1), (63, WAVE_HITS + 1), (64, WAVE_HITS), (65, 9), (129, 2 * WAVE_HITS)):
        batch[slot] = dense.read(h)
    bases, off = concat_reads(batch)
    whole = dense.db.read_votes(bases, off, min_hits=2, min_permille=25)
    same_records(whole, dense.model(bases, off, [(2, 25)])[1][(2, 25)], VOTE_DTYPE, "whole")
    for step in (1, 63, 65):
        parts = [dense.db.read_votes(bases, off[a:a + step + 1], min_hits=2, min_permille=25) for a in range(0, 130, step)]
        assert np.concatenate(parts).tobytes() == whole.tobytes(), step


# ------------------------------------------------------------------ 3. tally
def depth_sample(db):
    s = db.sample()
    s.set_option(KID_OPT_ENTRY_DEPTH, 1)
    return s


def check_tally(s, model_sm, hits, rec, counted, entry_targets, n_entries, what):
    g, u = model_sm.tally(hits, rec, counted, entry_targets)
    depth = s.entry_depth()
    assert np.array_equal(depth, dm.depth_of(hits, rec, counted, n_entries)), what
    assert np.array_equal(depth > 0, seen_bits(s, n_entries)), what
    assert ends_equal(s.end(), (g, u)), what
    return g, u


def test_tally_equals_the_model_applied_to_the_vote_records(world, db, dense):
    for rule in [(0, 0), (2, 25)]:
        s = depth_sample(db)
        rec = db.read_votes(world.bases, world.off, min_hits=rule[0], min_permille=rule[1], tally=s)
        same_records(rec, world.exp[rule], VOTE_DTYPE)
        g, _ = check_tally(s, world.sm, world.hits, world.exp[rule], np.ones(rec.size, bool), world.targets, world.keys.size, "rule %s" % (rule,))
        assert int(g.sum()) == rec.size
        s.close()
    # all three regimes in one tallied batch, the second kernel's reads among them
    batch = [dense.filler(j) for j in range(70)]
    for slot, h in ((0, WAVE_HITS + 3), (5, 70), (6, 3), (63, 2 * WAVE_HITS), (64, WAVE_HITS), (69, WAVE_HITS + 40)):
        batch[slot] = dense.read(h)
    bases, off = concat_reads(batch)
    hits, exp = dense.model(bases, off, [(0, 0), (3, 0), (0, 1000)])
    assert len({int(e["confident"][63]) for e in exp.values()}) >= 2
    for rule, e in exp.items():
        s = depth_sample(dense.db)
        same_records(dense.db.read_votes(bases, off, min_hits=rule[0], min_permille=rule[1], tally=s), e, VOTE_DTYPE)
        check_tally(s, dense.sm, hits, e, np.ones(e.size, bool), dense.tg, dense.keys.size, "dense rule %s" % (rule,))
        s.close()


def test_tally_of_a_fastq_block_with_dropped_records(world, db):
    from kmer_id_amd import synth
    n, length = 600, 150
    bases, _ = sc.cases.synth_reads(world.cum, world.parent, n, length)
    quals = [q.tobytes() for q in synth.qualities(n, length)]
    seqs = [bases[i * length:(i + 1) * length].tobytes() for i in range(n)]
    seqs += [b"ACGT" * 5, b"", seqs[3][:31]]  # records too short for a k-mer
    quals += [b"I" * 20, b"", b"I" * 31]
    start, stop, keep = trim_ranges(quals, [len(x) for x in seqs], 30)
    assert 0 < int((~keep).sum()) and int(keep.sum()) > 400
    start[~keep], stop[~keep] = 1, 0  # a record process_qual drops has no window
    text, recs = fastq_block(seqs, quals, eol=b"\r\n", blank_every=5)
    mb, moff = concat_reads(seqs)
    hits = world.hm.batch(mb, moff, start, stop)
    exp = world.vm.batch_anc(hits, (2, 0))
    s = depth_sample(db)
    got = db.read_votes_fastq(text, recs, min_hits=2, tally=s)
    same_records(got, exp, VOTE_DTYPE, "fastq")
    assert np.all(got["n_kmers"][~keep] == 0)
    g, _ = check_tally(s, world.sm, hits, exp, keep, world.targets, world.keys.size, "fastq")
    assert int(g.sum()) == int(keep.sum())  # a dropped record is counted nowhere
    s.close()


def test_classify_and_vote_tallies_mix_in_one_sample(world, db):
    bases, off = world.bases, world.off
    n = off.size - 1
    cut = n // 3
    finals = world.sm.finals(world.hits)
    assert (finals[cut:] != world.exp[(0, 0)]["call"][cut:]).any() and world.where["X_8_6"] >= cut
    rec = np.zeros(n, VOTE_DTYPE)  # what each read is counted under: its fold where it is classified, its call where it is voted on
    rec["confident"][:cut], rec["confident"][cut:] = finals[:cut], world.exp[(0, 0)]["confident"][cut:]
    g, u = world.sm.tally(world.hits, rec, np.ones(n, bool), world.targets)
    mixed = db.sample()
    mixed.classify(bases, off[:cut + 1])
    db.read_votes(bases, off[cut:], tally=mixed)
    assert ends_equal(mixed.end(), (g, u))
    mixed.close()


def test_error_statuses(world, db):
    n = 600
    bases, off = world.bases[:int(world.off[n])], world.off[:n + 1]

    assert status(lambda: db.read_votes(bases, off, min_permille=1001)) == -1
    assert db.read_votes(bases, off, min_permille=1000).size == n
    other = KmerDB(world.keys[:1000], world.targets[:1000], world.parent, k=30, log2_slots=14)
    t_other, t = other.sample(), db.sample()
    assert status(lambda: db.read_votes(bases, off, tally=t_other)) == -1  # a sample of another kid_db
    db.read_votes(bases, off, tally=t)
    first = t.end()
    assert status(lambda: db.read_votes(bases, off, tally=t)) == -10  # after kid_sample_end without reset
    t.reset()
    db.read_votes(bases, off, tally=t)
    assert ends_equal(t.end(), first)
    # n_reads = 0 launches nothing
    db.read_votes_time()
    assert db.read_votes(np.zeros(0, np.uint8), np.zeros(1, np.uint64)).size == 0
    assert db.read_votes_time() == (0.0, 0, 0)
    lib = _lib.load()
    assert lib.kid_db_read_votes(db._h, None, None, None, None, 1 << 31, 0, 0, None, None) == -1  # more than 2^31-1 reads
    assert lib.kid_db_read_votes(None, None, None, None, None, 0, 0, 0, None, None) == -1
    assert lib.kid_db_votes_from_hits_device(db._h, None, None, None, 5, 0, 0, None, None) == -1
    assert lib.kid_db_votes_from_hits_device(db._h, None, None, None, 0, 0, 1001, None, None) == -1
    for s in (t, t_other):
        s.close()
    other.close()


# ------------------------------------------------------------------ 4. the device form and the timer
def test_device_form_on_what_read_hits_device_left(world, db):
    bases, off = world.bases, world.off
    n = off.size - 1
    total = int(world.hits.offsets[-1])
    host = db.read_votes(bases, off, min_hits=2, min_permille=25)
    db.read_votes_time()
    with DeviceBatch(bases, off, total) as d:
        d.run(db, total)
        d_out = d.dev(n * 32, np.full(n * 8, 0xA5A5A5A5, np.uint32))
        db.votes_from_hits_device(d.d_ho.value, d.d_hits.value, d.d_nk.value, n, d_out.value, min_hits=2, min_permille=25)
        _lib.check(d.lib.kid_dev_sync(0))
        got = d.down(d_out, np.uint32, n * 8).view(VOTE_DTYPE)
        same_records(got, host, VOTE_DTYPE, "device form")
        same_records(got, world.exp[(2, 25)], VOTE_DTYPE, "device form vs model")
        # the same batch in three calls (offsets stay absolute: the hits pointer is the same)
        d_out3 = d.dev(n * 32, np.full(n * 8, 0xA5A5A5A5, np.uint32))
        cuts = [0, n // 3, n // 3 + 65, n]
        for a, b in zip(cuts[:-1], cuts[1:]):
            db.votes_from_hits_device(d.d_ho.value + 8 * a, d.d_hits.value, d.d_nk.value + 4 * a, b - a, d_out3.value + 32 * a,
                                      min_hits=2, min_permille=25)
        _lib.check(d.lib.kid_dev_sync(0))
        assert d.down(d_out3, np.uint32, n * 8).tobytes() == got.tobytes()
        ms, calls, reads = db.read_votes_time()
        assert calls == 4 and reads == 2 * n and ms > 0
        assert db.read_votes_time() == (0.0, 0, 0)
        # a target outside (0, ntar) is read as the root
        raw = d.down(d.d_hits, np.uint32, total * 3).reshape(total, 3)
        r = world.where["X_8_6"]
        h0 = int(world.hits.offsets[r])
        raw[h0, 1], raw[h0 + 1, 1] = world.parent.size + 5, 0  # [X, 8, 6] -> [root, root, 6]
        _lib.check(d.lib.kid_dev_upload(0, d.d_hits, raw.ctypes.data_as(C.c_void_p), raw.nbytes))
        db.votes_from_hits_device(d.d_ho.value, d.d_hits.value, d.d_nk.value, n, d_out.value)
        _lib.check(d.lib.kid_dev_sync(0))
        got = d.down(d_out, np.uint32, n * 8).view(VOTE_DTYPE)
        tg = world.hits.target.copy()
        tg[h0], tg[h0 + 1] = 1, 1
        patched = Hits(world.hits.offsets, world.hits.n_kmers, world.hits.pos, tg, world.hits.entry)
        same_records(got, world.vm.batch_anc(patched, (0, 0)), VOTE_DTYPE, "targets out of range")
        assert (int(got[r]["call"]), int(got[r]["p_best"]), int(got[r]["n_best"])) == (6, 3, 1)
