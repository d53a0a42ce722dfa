"""k-mer depth per database entry (KID_OPT_ENTRY_DEPTH): the counters a tally leaves, their spectrum, the export / add
pair and the merged form, against the independent model of tests/read_depth_model.py and against the sample's own seen
bitmap and ucount.  Every comparison is exact: integers."""

import numpy as np
import pytest

import read_calls
import read_depth_model as dm
import read_support_cases as sc
from helpers import concat_reads, fastq_block
from kmer_id_amd import KID_DB_OPT_MIN_BASE_QUALITY, KID_OPT_ENTRY_DEPTH, KmerDB, depth_spectrum_merged, end_merged
from read_calls import KINDS, header_constant, seen_bits, status
from read_hits_model import trim_ranges, windows
from read_support_model import RULES

pytestmark = pytest.mark.gpu

LANE_HITS = header_constant("kid_support.hip.h", "KID_SUPPORT_LANE_HITS")
MAXD = dm.DEPTH_MAX


class World(read_calls.World):
    """a database, its model, a batch of reads and, per rule, the model's records and depth: computed once"""

    def __init__(self, parent, keys, targets, bases, off, log2_slots, rules):
        super().__init__(parent, keys, targets, bases, off, log2_slots)
        self.model = self.sm
        self.hits = self.hm.batch(bases, off)
        self.finals = self.model.finals(self.hits)
        self.counted = np.ones(self.finals.size, bool)
        self.rec = {rule: self.model.batch_identity(self.hits, rule, self.finals) for rule in rules}
        self.depth = {rule: dm.depth_of(self.hits, self.rec[rule], self.counted, keys.size) for rule in rules}

    def spectrum(self, depth, bins):
        return dm.spectrum_of(depth, self.targets, self.parent.size, bins)


def depth_sample(db):
    s = db.sample()
    s.set_option(KID_OPT_ENTRY_DEPTH, 1)
    return s


def same_spectrum(got, exp, what=""):
    for g, e, name in zip(got, exp, ("spectrum", "ksum", "dmax")):
        assert g.dtype == e.dtype and g.shape == e.shape, "%s: %s" % (what, name)
        bad = np.argwhere(g != e)
        assert bad.size == 0, "%s: %s%s: got %d, the model %d" % (what, name, tuple(bad[0]), int(g[tuple(bad[0])]), int(e[tuple(bad[0])]))


@pytest.fixture(scope="module")
def world():
    parent, cum, keys, targets = sc.database()
    bases, off, _ = sc.reads(parent, cum, keys, targets)
    w = World(parent, keys, targets, bases, off, 20, RULES)
    w.cum = cum
    return w


@pytest.fixture(scope="module")
def db(world):
    return world.db()


# ------------------------------------------------------------------ 1. the model, every rule, three table kinds
def test_the_cases_have_depths_above_one_and_rules_that_uncall(world):
    assert int(world.depth[(0, 0)].max()) > 1
    assert 0 < int(world.depth[(3, 0)].sum()) < int(world.depth[(0, 0)].sum()) and not world.depth[(10 ** 6, 0)].any()
    assert np.unique(world.keys).size < world.keys.size  # duplicate keys: their later entries are never hit


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_depth_and_spectrum_equal_the_model(world, kind):
    d = world.db(KINDS[kind])
    n_entries = world.keys.size
    s, plain = depth_sample(d), d.sample()
    for rule in RULES:
        what = "%s rule %s" % (kind, rule)
        s.reset(), plain.reset()
        d.read_support(world.bases, world.off, min_hits=rule[0], min_permille=rule[1], tally=s)
        d.read_support(world.bases, world.off, min_hits=rule[0], min_permille=rule[1], tally=plain)
        got = s.entry_depth()
        bad = np.flatnonzero(got != world.depth[rule])
        assert got.dtype == np.uint32 and bad.size == 0, "%s: entry %d: got %d, the model %d" % (what, bad[0], got[bad[0]], world.depth[rule][bad[0]])
        spectra = {bins: s.depth_spectrum(bins) for bins in (2, 3, 256)}  # (before kid_sample_end ...)
        assert np.array_equal(got > 0, seen_bits(s, n_entries)), what
        g, u = s.end()
        gp, up = plain.end()
        assert np.array_equal(g, gp) and np.array_equal(u, up), what
        for bins, sp in spectra.items():
            same_spectrum(sp, world.spectrum(world.depth[rule], bins), "%s bins %d" % (what, bins))
            assert np.array_equal(sp[0][:, 1:].sum(axis=1).astype(np.int64), u), what  # distinct = ucount
            assert np.array_equal(sp[0].sum(axis=1), np.bincount(world.targets, minlength=world.parent.size)), what
        same_spectrum(s.depth_spectrum(256), spectra[256], what + " (... and after it, repeated)")
    s.close(), plain.close(), d.close()


# ------------------------------------------------------------------ 2. work-split edges
def test_work_split_edges(world):
    """reads of LANE_HITS - 1 .. 200 hits at the reads 0, 63 and 64 of a group of 64, cut from the first 900 bases of one
    genome so that they overlap; two reads hold one stretch twice (lane path: 2 x 3 hits, wave path: 2 x 11 hits)"""
    rng = np.random.default_rng(640)
    parent = world.parent
    x = next(int(t) for t in world.targets if t > 1 and sc.top_level(parent, int(t)) != 5)
    g = rng.choice(sc.ACGT, 4000).tobytes()
    keys = windows(g, 0, len(g) - 1, 30)[0]
    tg = np.array([8, 6, 5, 36, 35, 8, 6, x], np.uint32)[rng.integers(0, 8, keys.size)]
    counts = [LANE_HITS - 1, LANE_HITS, LANE_HITS + 1, 63, 64, 65, 200]
    rules = [(0, 0), (3, 0), (2, 25), (0, 1000)]

    def dense(h, lo=0, hi=600):
        p = int(rng.integers(lo, hi))
        return g[p:p + h + 29]

    filler = lambda i: b"" if i % 2 else rng.choice(sc.ACGT, 100).tobytes()  # noqa: E731
    seqs = []
    for i in range(len(counts)):
        batch = [filler(j) for j in range(130)]
        batch[0], batch[63], batch[64] = dense(counts[i]), dense(counts[(i + 1) % 7]), dense(counts[(i + 2) % 7])
        batch[100] = dense(counts[(i + 3) % 7])
        batch[10], batch[70] = g[300:332] + b"N" + g[300:332], g[420:460] + b"N" + g[420:460]
        batch[20], batch[21], batch[22] = dense(1, 2000, 3000), dense(2, 2000, 3000), dense(2, 2000, 3000)  # too few hits for (3, 0)
        seqs += batch
    bases, off = concat_reads(seqs)
    w = World(parent, keys, tg, bases, off, 16, rules)
    per = np.diff(w.hits.offsets.astype(np.int64))
    assert [int(per[j]) for j in (0, 63, 64, 10, 70)] == [counts[0], counts[1], counts[2], 6, 22] and int(per[1]) == 0
    c3 = w.rec[(3, 0)]["confident"]
    assert ((per > 0) & (c3 == 0)).any() and ((per > LANE_HITS) & (c3 > 0)).any()
    assert int(w.depth[(0, 0)].max()) > 5 and int((w.depth[(0, 0)] != w.depth[(3, 0)]).sum()) > 0
    d = w.db()
    s = depth_sample(d)
    for rule in rules:
        s.reset()
        for a in range(0, off.size - 1, 130):  # the batches one call each: the reads 0, 63, 64 keep their lanes
            d.read_support(bases, off[a:a + 131], min_hits=rule[0], min_permille=rule[1], tally=s)
        got = s.entry_depth()
        bad = np.flatnonzero(got != w.depth[rule])
        assert bad.size == 0, "rule %s: entry %d: got %d, the model %d" % (rule, bad[0], got[bad[0]], w.depth[rule][bad[0]])
        same_spectrum(s.depth_spectrum(256), w.spectrum(w.depth[rule], 256), "rule %s" % (rule,))
        assert np.array_equal(got > 0, seen_bits(s, keys.size))
    s.close(), d.close()


# ------------------------------------------------------------------ 3. contention
def test_one_kmer_in_5000_reads_of_one_batch(world, db):
    rng = np.random.default_rng(5000)
    first = np.unique(world.keys, return_index=True)[1]
    e = int(next(o for o in np.sort(first) if world.targets[o] > 1))
    kmer = sc.cases.key_seq(world.keys[e], 30)
    bases, off = concat_reads([rng.choice(sc.ACGT, 5).tobytes() + kmer + rng.choice(sc.ACGT, 5).tobytes() for _ in range(5000)])
    hits = world.hm.batch(bases, off)
    finals = world.model.finals(hits)
    exp = dm.depth_of(hits, world.model.batch_identity(hits, (0, 0), finals), np.ones(5000, bool), world.keys.size)
    assert int(exp[e]) == 5000
    s = depth_sample(db)
    db.read_support(bases, off, tally=s)
    got = s.entry_depth()
    assert int(got[e]) == 5000 and np.array_equal(got, exp)
    sp, ksum, dmax = s.depth_spectrum(256)
    t = int(world.targets[e])
    assert int(dmax[t]) == 5000 and int(sp[t, 255]) == 1 and int(ksum.sum()) == int(exp.sum())
    s.close()


# ------------------------------------------------------------------ 4. saturation
def test_counters_saturate(world, db):
    first = np.unique(world.keys, return_index=True)[1]
    e = int(next(o for o in np.sort(first) if world.targets[o] > 1))
    t = int(world.targets[e])
    kmer = sc.cases.key_seq(world.keys[e], 30)
    bases, off = concat_reads([b"N".join([kmer] * 5)])
    s = depth_sample(db)
    s.depth_add(e, np.array([0xFFFFFFFE], np.uint32))
    rec = db.read_support(bases, off, tally=s)
    assert int(rec["n_hits"][0]) == 5 and int(rec["confident"][0]) == t
    assert int(s.entry_depth(e, e + 1)[0]) == MAXD
    db.read_support(bases, off, tally=s)  # adds onto the maximum leave the maximum
    assert int(s.entry_depth(e, e + 1)[0]) == MAXD
    # the array add saturates too; ksum and dmax report the saturated value
    s.reset()
    s.depth_add(e, np.array([0x20], np.uint32))
    s.depth_add(e, np.array([0xFFFFFFF0], np.uint32))
    got = s.entry_depth()
    assert int(got[e]) == MAXD and int(got.astype(np.uint64).sum()) == MAXD
    sp, ksum, dmax = s.depth_spectrum(256)
    assert int(ksum[t]) == MAXD and int(dmax[t]) == MAXD and int(sp[t, 255]) == 1 and int(sp[:, 1:].sum()) == 1
    s.close()


# ------------------------------------------------------------------ 5. spectrum geometry
@pytest.mark.parametrize("n", [1, 127, 128, 129, 513, 4097])
def test_spectrum_of_interleaved_targets_and_the_padding(n):
    """targets interleaved, not in runs; counters set through depth_add, the bin edges among them (a tree of 18 nodes,
    so that 4096 bins are a small table)"""
    rng = np.random.default_rng(n)
    parent = sc.chain_taxonomy(8)[0]
    keys = np.unique(rng.integers(0, 1 << 60, 2 * n, dtype=np.uint64))[:n]
    rng.shuffle(keys)
    tg = (2 + (np.arange(n) * 5 + rng.integers(0, 2, n)) % (parent.size - 2)).astype(np.uint32)
    d = KmerDB(keys, tg, parent, k=30, log2_slots=16)
    assert d.info.n_entries == n
    s = depth_sample(d)
    for bins in (2, 3, 16, 256, 4096):
        depth = np.where(rng.random(n) < 0.5, 0, rng.integers(0, 2 * bins, n)).astype(np.uint32)
        depth[rng.integers(0, n, 3)] = [bins - 2, bins - 1, bins]
        depth[-1] = bins - 1  # the last entry, next to the padding
        s.reset()
        s.depth_add(0, depth)
        assert np.array_equal(s.entry_depth(), depth)
        got = s.depth_spectrum(bins)
        same_spectrum(got, dm.spectrum_of(depth, tg, parent.size, bins), "n %d bins %d" % (n, bins))
        assert np.array_equal(got[0].sum(axis=1), np.bincount(tg, minlength=parent.size))
    # a part of the array, added twice
    s.reset()
    part = rng.integers(1, 9, n - n // 2).astype(np.uint32)
    s.depth_add(n // 2, part), s.depth_add(n // 2, part)
    assert np.array_equal(s.entry_depth(n // 2), 2 * part) and not s.entry_depth(0, n // 2).any()
    s.close(), d.close()


def test_duplicate_keys_and_target_0_entries_sit_in_column_0(world):
    rng = np.random.default_rng(40)
    parent = world.parent
    keys = sc.random_keys(rng, 40)
    tg = np.array([5, 6, 8, 35, 36], np.uint32)[np.arange(40) % 5]
    keys[10], keys[31] = keys[3], keys[3]  # entries 10 and 31 repeat entry 3 (under other targets)
    tg[20] = 0
    bases, off = concat_reads([sc.cases.key_seq(k, 30) for k in keys] * 2)
    w = World(parent, keys, tg, bases, off, 16, [(0, 0)])
    exp = w.depth[(0, 0)]
    assert int(exp[3]) == 6 and int(exp[10]) == 0 and int(exp[31]) == 0 and int(exp[20]) == 0 and int(exp[4]) == 2
    d = w.db()
    s = depth_sample(d)
    d.read_support(bases, off, tally=s)
    assert np.array_equal(s.entry_depth(), exp)
    got = s.depth_spectrum(4)
    same_spectrum(got, w.spectrum(exp, 4), "duplicates")
    assert int(got[0][0, 0]) == 1 and np.array_equal(got[0].sum(axis=1), np.bincount(tg, minlength=parent.size))
    s.close(), d.close()


# ------------------------------------------------------------------ 6. the FASTQ form
def test_fastq_records_and_masked_bases(world, db):
    from kmer_id_amd import synth
    from base_quality_cases import mask_block
    n, length = 600, 150
    bases, _ = sc.cases.synth_reads(world.cum, world.parent, n, length)
    quals = synth.qualities(n, length)
    quals[::2, 75] = ord("2")  # Q17 in the middle of every other read: masked at Q = 20, not trimmed
    seqs = [bases[i * length:(i + 1) * length].tobytes() for i in range(n)] + [b"ACGT" * 5, b"", bytes(bases[450:481])]
    qs = [q.tobytes() for q in quals] + [b"I" * 20, b"", b"I" * 31]
    start, stop, keep = trim_ranges(qs, [len(x) for x in seqs], 30)
    assert 0 < int((~keep).sum()) and int(keep.sum()) > 400
    start[~keep], stop[~keep] = 1, 0  # a record process_qual drops has no window
    text, recs = fastq_block(seqs, qs, eol=b"\r\n", blank_every=5)
    s = depth_sample(db)
    exp = {}
    for q in (0, 20):
        mtext = mask_block(text, recs, q)[0] if q else text
        mb, moff = concat_reads([bytes(mtext[so:so + sl]) for so, sl, _, _ in recs.tolist()])
        hits = world.hm.batch(mb, moff, start, stop)
        rec = world.model.batch_identity(hits, (2, 0), world.model.finals(hits))
        exp[q] = dm.depth_of(hits, rec, keep, world.keys.size)
        db.set_option(KID_DB_OPT_MIN_BASE_QUALITY, q)
        s.reset()
        got_rec = db.read_support_fastq(text, recs, min_hits=2, tally=s)
        assert np.array_equal(got_rec["confident"], rec["confident"]) and np.all(got_rec["n_kmers"][~keep] == 0)
        assert np.array_equal(s.entry_depth(), exp[q]), "Q = %d" % q
        assert int(s.end()[0].sum()) == int(keep.sum())  # a dropped record is counted nowhere
    db.set_option(KID_DB_OPT_MIN_BASE_QUALITY, 0)
    assert 0 < int(exp[20].sum()) < int(exp[0].sum())
    s.close()


# ------------------------------------------------------------------ 7. state
def test_option_states_and_argument_errors(world, db):
    bases, off = world.bases, world.off[:601]
    s = db.sample()
    for call in (lambda: s.entry_depth(), lambda: s.depth_add(0, np.ones(4, np.uint32)), lambda: s.depth_spectrum(),
                 lambda: depth_spectrum_merged([s]), lambda: depth_spectrum_merged([s, depth_sample(db)])):
        assert status(call) == -10  # the option is off
    assert status(lambda: s.set_option(KID_OPT_ENTRY_DEPTH, 2)) == -1 and status(lambda: s.set_option(KID_OPT_ENTRY_DEPTH, -1)) == -1
    db.read_support(bases, off, tally=s)  # (a tally without the option counts as ever)
    s.set_option(KID_OPT_ENTRY_DEPTH, 1)
    assert not s.entry_depth().any()  # allocated zeroed: what was tallied before is not in it
    db.read_support(bases, off, tally=s)
    first = s.entry_depth()
    assert first.any()
    s.set_option(KID_OPT_ENTRY_DEPTH, 1)  # on while on: a no-op
    assert np.array_equal(s.entry_depth(), first)
    # a classify call into the sample leaves every counter as it is
    s.classify(world.bases, world.off)
    assert np.array_equal(s.entry_depth(), first)
    n = world.keys.size
    assert status(lambda: s.depth_spectrum(1)) == -1 and status(lambda: s.depth_spectrum(4097)) == -1
    assert status(lambda: depth_spectrum_merged([s, depth_sample(db)], 1)) == -1
    assert status(lambda: s.entry_depth(0, n + 1)) == -1 and status(lambda: s.entry_depth(n + 1, n + 1)) == -1
    assert status(lambda: s.depth_add(n - 1, np.ones(2, np.uint32))) == -1
    assert s.entry_depth(n, n).size == 0
    assert status(lambda: depth_spectrum_merged([s, s])) == -1  # a sample named twice
    s.reset()
    assert not s.entry_depth().any() and int(s.depth_spectrum(2)[0][:, 1].sum()) == 0
    s.set_option(KID_OPT_ENTRY_DEPTH, 0)  # off: the counters are gone
    assert status(lambda: s.entry_depth()) == -10
    s.set_option(KID_OPT_ENTRY_DEPTH, 0)
    s.close()


def test_any_split_of_the_batch_and_a_second_sample_give_the_same_bytes(world, db):
    a0, a1 = 500, 800  # 100 adversarial and 200 synthetic reads
    exp = None
    for step in (a1 - a0, 64, 7, 1):
        s = depth_sample(db)
        for a in range(a0, a1, step):
            db.read_support(world.bases, world.off[a:min(a + step, a1) + 1], min_hits=2, min_permille=25, tally=s)
        got = s.entry_depth().tobytes()
        exp = exp or got
        assert got == exp and any(got), "calls of %d reads" % step
        s.close()
    s, t = depth_sample(db), depth_sample(db)
    db.read_support(world.bases, world.off, tally=s), db.read_support(world.bases, world.off, tally=t)
    assert s.entry_depth().tobytes() == t.entry_depth().tobytes() == world.depth[(0, 0)].tobytes()
    s.close(), t.close()


# ------------------------------------------------------------------ 8. merged
def test_merged_spectrum_equals_the_one_sample_answer(world):
    d0 = world.db()
    d1 = d0.replicate(0)  # a replica on device 0, as the merge tests of the suite have it
    n = world.off.size - 1
    cut = n // 3
    whole, a, b = depth_sample(d0), depth_sample(d0), depth_sample(d1)
    d0.read_support(world.bases, world.off, min_hits=2, min_permille=25, tally=whole)
    d0.read_support(world.bases, world.off[:cut + 1], min_hits=2, min_permille=25, tally=a)
    d1.read_support(world.bases, world.off[cut:], min_hits=2, min_permille=25, tally=b)
    da, db_ = a.entry_depth(), b.entry_depth()
    assert da.any() and db_.any() and np.array_equal(dm.saturating_add(da, db_), world.depth[(2, 25)])
    for bins in (2, 256):
        one = whole.depth_spectrum(bins)
        same_spectrum(one, world.spectrum(world.depth[(2, 25)], bins), "one sample, bins %d" % bins)
        m1 = depth_spectrum_merged([a, b], bins)
        m2 = depth_spectrum_merged([b, a], bins)
        same_spectrum(m1, one, "merged, bins %d" % bins)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(m1, m2))
    assert np.array_equal(a.entry_depth(), da) and np.array_equal(b.entry_depth(), db_)  # no sample's counters changed
    # the sum saturates: preload both halves of one entry
    e = int(np.flatnonzero(world.depth[(2, 25)])[0])
    a.depth_add(e, np.array([0xFFFFFFF0], np.uint32)), b.depth_add(e, np.array([0x7FFFFFFF], np.uint32))
    sp, ksum, dmax = depth_spectrum_merged([a, b], 256)
    t = int(world.targets[e])
    assert int(dmax[t]) == MAXD and int(ksum.sum()) == int(world.depth[(2, 25)].astype(np.uint64).sum()) - int(world.depth[(2, 25)][e]) + MAXD
    # gcount / ucount of the merged samples are what they are without the option
    g, u = end_merged([a, b])
    gw, uw = whole.end()
    assert np.array_equal(g, gw) and np.array_equal(u, uw)
    for s in (whole, a, b):
        s.close()
    d1.close(), d0.close()
