"""kid_db_read_segment_votes* (segments called by root-path votes) against the independent model of
tests/read_segment_votes_model.py (its direct form), against kid_db_read_segments and kid_db_read_votes of the same
library, and against its own contract.  Every comparison is exact: integers."""
import ctypes as C

import numpy as np
import pytest

import read_calls
import read_support_cases as sc
from base_quality_cases import hit_reads, mask_block
from helpers import DeviceBatch, concat_reads, fastq_block, oracle_db
from kmer_id_amd import (FRAGMENT_VOTE_DTYPE, KID_DB_OPT_LOW_COMPLEXITY, KID_DB_OPT_MIN_BASE_QUALITY, KID_FLAG_REF_GEOMETRY, SEGMENT_VOTE_DTYPE,
                         VOTE_DTYPE, KmerDB, _lib)
from low_complexity_model import mask_block as lowc_mask_block
from read_calls import KINDS, RC_SETTINGS, genome_world, header_constant, mirrored, same_segments, status, strand_world
from read_fragment_votes_model import FragmentVoteModel
from read_hits_model import HitModel, trim_ranges
from read_segment_votes_model import VOTE_FIELDS, SegmentVoteModel
from read_support_model import SupportModel

pytestmark = pytest.mark.gpu

SETTINGS = [(1, 1), (63, 63), (64, 64), (65, 13), (100, 50), (121, 121), (10 ** 6, 10 ** 6)]
RULES = [(0, 0), (2, 25)]
GEOMETRY = ("pos", "n_pos", "n_kmers", "n_hits")
LANE = header_constant("kid_votes.hip.h", "KID_VOTE_LANE_HITS")
WAVE = header_constant("kid_votes.hip.h", "KID_VOTE_WAVE_HITS")
CANARY = 0xA5A5A5A5


def call(db, bases, off, seg, rule, start=None, stop=None):
    return db.read_segment_votes(bases, off, start, stop, seg_len=seg[0], seg_step=seg[1], min_hits=rule[0], min_permille=rule[1])


def regimes(rec):
    """-> how many of the model's segments each of the three regimes takes"""
    m = rec["n_hits"]
    return int(((m > 0) & (m <= LANE)).sum()), int(((m > LANE) & (m <= WAVE)).sum()), int((m > WAVE).sum())


class World(read_calls.World):
    """a database, its models and a batch of reads; the model's segments per (setting, rule) are computed once"""

    def __init__(self, parent, keys, targets, bases, off, log2_slots, start=None, stop=None):
        super().__init__(parent, keys, targets, bases, off, log2_slots)
        self.seg = SegmentVoteModel(self.sm, bases, off, start, stop)
        self.start, self.stop = start, stop
        self._exp = {}

    def exp(self, seg, rule):
        if (seg, rule) not in self._exp:
            self._exp[(seg, rule)] = self.seg.direct(seg[0], seg[1], rule)
        return self._exp[(seg, rule)]

    def check(self, db, settings, rules, what=""):
        for seg in settings:
            for rule in rules:
                same_segments(call(db, self.bases, self.off, seg, rule, self.start, self.stop), self.exp(seg, rule), SEGMENT_VOTE_DTYPE,
                              "%s %s rule %s" % (what, seg, rule))


@pytest.fixture(scope="module")
def world():
    parent, cum, keys, targets = sc.database()
    bases, off, where = sc.reads(parent, cum, keys, targets)
    w = World(parent, keys, targets, bases, off, 20)
    w.cum = cum
    return w


@pytest.fixture(scope="module")
def db(world):
    return world.db()


def other_lineage(world):
    return next(int(t) for t in world.targets if t > 1 and sc.top_level(world.parent, int(t)) != 5)


# ------------------------------------------------------------------ 1. the model, three table kinds
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_segment_votes_equal_the_model(world, kind):
    assert world.off.size - 1 == 2605
    d = world.db(KINDS[kind])
    world.check(d, SETTINGS, RULES, kind)
    for rule in RULES:
        # one segment per read: the eight vote fields are kid_db_read_votes' of the same library
        got = call(d, world.bases, world.off, (10 ** 6, 10 ** 6), rule)
        votes = d.read_votes(world.bases, world.off, min_hits=rule[0], min_permille=rule[1])
        per = np.diff(got.offsets.astype(np.int64))
        assert np.all(per <= 1) and np.all(per[votes["n_kmers"] > 0] == 1) and not votes["n_hits"][per == 0].any()
        for f in VOTE_FIELDS:
            assert np.array_equal(got.records[f], votes[f][per == 1]), (rule, f)
        assert not got.records["pos"].any() and np.array_equal(got.records["n_pos"], world.seg.P[per == 1])
        # at every setting the geometry is kid_db_read_segments' of the same library
        for seg in SETTINGS:
            got = call(d, world.bases, world.off, seg, rule)
            fold = d.read_segments(world.bases, world.off, seg_len=seg[0], seg_step=seg[1], min_hits=rule[0], min_permille=rule[1])
            assert np.array_equal(got.offsets, fold.offsets), (seg, rule)
            for f in GEOMETRY:
                assert np.array_equal(got.records[f], fold.records[f]), (seg, rule, f)
    e = world.exp((100, 50), (2, 25))[1]
    assert int((e["confident"] != e["call"]).sum()) > 0 and int((e["n_hits"] == 0).sum()) > 1000  # the rule bites; the list is dense
    d.close()


# ------------------------------------------------------------------ 2. tile edges
def test_tile_edges(world):
    rng = np.random.default_rng(6464)
    parent = world.parent
    g, keys, tg = genome_world(rng, [8, 6, 5, 36, 35, 8, 6, 1], 4000, 1)
    d = KmerDB(keys, tg, parent, k=30, log2_slots=16)
    sm = SupportModel(HitModel(oracle_db(parent, keys, tg, 16), keys, tg, 30), parent)
    for P in (1, 63, 64, 65, 127, 128, 129, 192):
        p0 = int(rng.integers(0, len(g) - (P + 29)))
        stretch = g[p0:p0 + P + 29]
        with_n = bytearray(stretch)
        for m in range(64, len(stretch), 64):  # an N exactly at, and one base before, every multiple of 64 from the read's start
            with_n[m] = with_n[m - 1] = ord("N")
        for copy, seq in (("plain", stretch), ("N", bytes(with_n))):
            # twice, a read of fewer than k bases and an empty one in between; the second is the batch's last read
            bases, off = concat_reads([seq, b"ACGTACGTAC", b"", seq])
            model = SegmentVoteModel(sm, bases, off)
            for seg_len in (1, 32, 64, 65, 128):
                for seg_step in sorted({1, seg_len} | ({64} if 64 <= seg_len else set())):
                    for rule in [(0, 0), (2, 25)]:
                        exp = model.direct(seg_len, seg_step, rule)
                        what = "P %d %s %d:%d %s" % (P, copy, seg_len, seg_step, rule)
                        same_segments(call(d, bases, off, (seg_len, seg_step), rule), exp, SEGMENT_VOTE_DTYPE, what)
                        rec = exp[1]
                        assert int(exp[0][1]) * 2 == rec.size == int(exp[0][4]) and exp[0][1] == exp[0][2] == exp[0][3], what
                        if copy == "plain":
                            assert np.array_equal(rec["n_kmers"], rec["n_pos"]) and np.array_equal(rec["n_hits"], rec["n_pos"]), what
    d.close()


# ------------------------------------------------------------------ 3. regime edges
def test_regime_edges(world):
    rng = np.random.default_rng(512)
    parent = world.parent
    g, keys, tg = genome_world(rng, [8, 6, 5, 36, 35, 8, 6, other_lineage(world)], 4029, 1)  # 4000 positions, every one a hit
    counts = [LANE - 1, LANE, LANE + 1, 63, 64, 65, WAVE - 1, WAVE, WAVE + 1, 1500]
    nc = len(counts)
    rules = [(0, 0), (2, 25), (0, 1000)]

    def dense(h):
        p = int(rng.integers(0, len(g) - (h + 29)))
        return g[p:p + h + 29]

    def spacer(n):
        return rng.choice(sc.ACGT, n).tobytes()

    d = KmerDB(keys, tg, parent, k=30, log2_slots=16)
    sm = SupportModel(HitModel(oracle_db(parent, keys, tg, 16), keys, tg, 30), parent)
    # (a) single-segment reads at lanes 0, 63, 64 and 198 of a batch of 260, hit-free fillers around them
    seen = set()
    for i in range(0, nc, 2):
        batch = [spacer(100) if j <= 64 or j % 3 == 0 else (b"", b"ACGT")[j % 2] for j in range(260)]
        at = {0: counts[i], 63: counts[(i + 1) % nc], 64: counts[(i + 2) % nc], 198: counts[(i + 5) % nc]}
        for j, h in at.items():
            batch[j] = dense(h)
        bases, off = concat_reads(batch)
        model = SegmentVoteModel(sm, bases, off)
        for rule in rules:
            exp = model.direct(2000, 2000, rule)
            assert exp[1].size >= 130 and [int(exp[0][j]) for j in (0, 63, 64)] == [0, 63, 64]
            assert [int(exp[1]["n_hits"][int(exp[0][j])]) for j in sorted(at)] == [at[j] for j in sorted(at)]
            assert int(exp[1]["n_hits"][1:63].sum()) == 0
            same_segments(call(d, bases, off, (2000, 2000), rule), exp, SEGMENT_VOTE_DTYPE, "batch %d rule %s" % (i, rule))
        seen |= set(at.values())
    assert seen == set(counts)
    # (b) the same counts as segments INSIDE one record: a stretch of h hits and a hit-free spacer fill 1600 bases each,
    # so that segment j of 1600:1600 holds exactly counts[j] hits (an N at either end of a spacer: its first or last base
    # must not continue the genome by chance)
    parts = [dense(h) + b"N" + spacer(1600 - (h + 29) - 2) + b"N" for h in counts]
    bases, off = concat_reads([spacer(100), b"".join(parts) + spacer(29), spacer(100)])
    model = SegmentVoteModel(sm, bases, off)
    for rule in rules:
        exp = model.direct(1600, 1600, rule)
        rec = exp[1][int(exp[0][1]):int(exp[0][2])]
        assert rec["n_hits"].tolist() == counts and regimes(rec) == (2, 6, 2)
        same_segments(call(d, bases, off, (1600, 1600), rule), exp, SEGMENT_VOTE_DTYPE, "one record rule %s" % (rule,))
    # (c) overlap: about a hundred segments of more than WAVE hits that share hits, all the workgroup kernel's
    bases, off = concat_reads([spacer(100), spacer(700) + dense(700) + spacer(700), spacer(100)])
    model = SegmentVoteModel(sm, bases, off)
    seg = (WAVE + 88, 1)
    for rule in rules:
        exp = model.direct(seg[0], seg[1], rule)
        lane, wave, big = regimes(exp[1])
        assert big >= 100 and wave >= 100 and lane >= 8, (lane, wave, big)
        same_segments(call(d, bases, off, seg, rule), exp, SEGMENT_VOTE_DTYPE, "overlap rule %s" % (rule,))
    # no read at all; reads without a window only
    empty = d.read_segment_votes(np.zeros(0, np.uint8), np.zeros(1, np.uint64), seg_len=5)
    assert empty.records.size == 0 and empty.records.dtype == SEGMENT_VOTE_DTYPE and empty.offsets.tolist() == [0]
    bases, off = concat_reads([b"", b"ACGT", b""])
    none = d.read_segment_votes(bases, off, seg_len=5)
    assert none.records.size == 0 and none.offsets.tolist() == [0, 0, 0, 0]
    d.close()


# ------------------------------------------------------------------ 4. one long record
def test_a_record_of_70000_positions(world):
    rng = np.random.default_rng(70000)
    parent = world.parent
    g, keys, tg = genome_world(rng, [8, 6, 5, 36, 35, 5, 5, 1], 70029, 20)
    short = [rng.choice(sc.ACGT, 150).tobytes() for _ in range(5)]
    bases, off = concat_reads(short[:2] + [g] + short[2:] + [g[1000:1000 + 29 + 40]])
    w = World(parent, keys, tg, bases, off, 16)
    assert int(w.seg.P[2]) == 70000
    settings, rules = [(4096, 1024), (1000, 1000)], [(0, 0), (0, 60), (150, 0)]
    for seg in settings:
        conf = np.stack([w.exp(seg, rule)[1]["confident"] for rule in rules])
        assert int((conf != conf[0]).any(axis=0).sum()) > 0  # somewhere the rules give different answers
        assert int(w.exp(seg, (0, 0))[0][3] - w.exp(seg, (0, 0))[0][2]) == (66 if seg[0] == 4096 else 70)
    d = w.db()
    w.check(d, settings, rules, "long record")
    d.close()


# ------------------------------------------------------------------ 5. a record and its reverse complement
def test_reverse_complement(world):
    keys, tg, bases, off = strand_world(world.parent, world.targets)
    w = World(world.parent, keys, tg, bases, off, 16)
    d = w.db()
    differ = 0
    for seg in RC_SETTINGS:
        for rule in RULES:
            got = call(d, bases, off, seg, rule)
            same_segments(got, w.exp(seg, rule), SEGMENT_VOTE_DTYPE, "strands %s %s" % (seg, rule))
            a, b = mirrored(got.offsets, got.records, (seg, rule))
            for f in VOTE_FIELDS:
                assert np.array_equal(a[f], b[f]), (seg, rule, f)
        fold = d.read_segments(bases, off, seg_len=seg[0], seg_step=seg[1])
        fa, fb = mirrored(fold.offsets, fold.records, seg)
        differ += int((fa["final"] != fb["final"]).sum())
    assert differ > 0  # the fold of the same library depends on the strand
    d.close()


# ------------------------------------------------------------------ 6. trees: the ROWS and the parent[] form
@pytest.mark.parametrize("depth", [8, 12])
def test_hand_built_trees(depth):
    parent, spine, sibs = sc.chain_taxonomy(depth)
    rng = np.random.default_rng(depth)
    nodes = spine + sibs
    tg = np.repeat(np.array(nodes, np.uint32), 4)
    keys = sc.random_keys(rng, tg.size)
    kseq = lambda node, j=0: sc.cases.key_seq(keys[nodes.index(node) * 4 + j], 30)  # noqa: E731
    deep, deep_sib, above = spine[-1], sibs[-1], spine[-2]
    seqs = [sc.implanted(rng, [kseq(deep)]),
            sc.implanted(rng, [kseq(deep), kseq(deep, 1), kseq(above)]),
            sc.implanted(rng, [kseq(deep), kseq(deep_sib)]),
            sc.implanted(rng, [kseq(deep_sib), kseq(deep)] * 6)]
    for _ in range(120):
        pick = rng.integers(0, keys.size, int(rng.integers(1, 15)))
        seqs.append(sc.implanted(rng, [sc.cases.key_seq(keys[j], 30) for j in pick]))
    # a record whose every window is a hit somewhere on the tree: 700 hits, the workgroup kernel's as one segment
    g, gkeys, gtg = genome_world(rng, nodes, 729, 1)
    seqs.insert(7, g)
    keys, tg = np.concatenate([keys, gkeys]), np.concatenate([tg, gtg])
    bases, off = concat_reads(seqs)
    w = World(parent, keys, tg, bases, off, 12)
    settings = [(40, 20), (600, 100), (10 ** 6, 10 ** 6)]
    e = w.exp((40, 20), (2, 0))[1]
    assert int((e["n_hits"] > 1).sum()) > 50 and int(((e["confident"] != e["call"]) & (e["confident"] > 0)).sum()) > 0
    assert regimes(e)[1] > 0 and regimes(w.exp((600, 100), (0, 0))[1])[2] >= 2 and regimes(w.exp((10 ** 6, 10 ** 6), (0, 0))[1])[2] == 1
    for flags in (0, KID_FLAG_REF_GEOMETRY):
        d = w.db(flags)
        assert d.info.tree_depth == depth
        w.check(d, settings, [(0, 0), (2, 0), (2, 25)], "depth %d flags %d" % (depth, flags))
        d.close()


# ------------------------------------------------------------------ 7. the FASTQ form
def test_fastq_form(world, db):
    from kmer_id_amd import synth
    n, length = 1200, 150
    bases, off = sc.cases.synth_reads(world.cum, world.parent, n, length)
    quals = [q.tobytes() for q in synth.qualities(n, length)]
    seqs = [bases[i * length:(i + 1) * length].tobytes() for i in range(n)]
    seqs += [b"ACGT" * 5, b"", seqs[3][:31]]  # records too short for a k-mer
    quals += [b"I" * 20, b"", b"I" * 31]
    # reads with a low-quality base inside their hit windows (not trimmed, masked at Q = 20)
    extra = hit_reads(world.odb, world.keys, world.targets, world.parent, world.cum, 40, r0=90000)
    seqs += [s for s, _ in extra]
    quals += [q for _, q in extra]
    # reads with a database k-mer beside a homopolymer run (masked at T = 20)
    for j in range(20):
        s = sc.cases.key_seq(world.keys[j * 7], 30) + b"A" * 70
        seqs.append(s)
        quals.append(b"I" * len(s))
    start, stop, keep = trim_ranges(quals, [len(s) for s in seqs], 30)
    assert 0 < int((~keep).sum()) and int(keep.sum()) > 800
    text, recs = fastq_block(seqs, quals, eol=b"\r\n", blank_every=5)  # CRLF line ends, blank lines between records

    def expect(the_seqs, seg, rule):
        b, o = concat_reads(the_seqs)
        return SegmentVoteModel(world.sm, b, o, start, stop, keep).direct(seg[0], seg[1], rule)

    def fq(t, seg, rule):
        return db.read_segment_votes_fastq(t, recs, seg_len=seg[0], seg_step=seg[1], min_hits=rule[0], min_permille=rule[1])

    for seg, rule in [((40, 20), (0, 0)), ((64, 64), (2, 25)), ((10 ** 6, 10 ** 6), (2, 25))]:
        got = fq(text, seg, rule)
        same_segments(got, expect(seqs, seg, rule), SEGMENT_VOTE_DTYPE, "fastq %s %s" % (seg, rule))
        per = np.diff(got.offsets.astype(np.int64))
        assert not per[~keep].any() and np.all(per[keep] >= 1)  # a dropped record has no segment
        assert np.array_equal(got.records["pos"][got.offsets[:-1][keep].astype(np.int64)], start[keep])
    # the two mask options: the records are those on the text with the masked bases replaced by N
    seg, rule = (40, 20), (2, 25)
    plain = fq(text, seg, rule)
    for option, level, mask in [(KID_DB_OPT_MIN_BASE_QUALITY, 20, mask_block), (KID_DB_OPT_LOW_COMPLEXITY, 20, lowc_mask_block)]:
        masked, n_masked = mask(text, recs, level)
        assert n_masked > 0
        db.set_option(option, level)
        try:
            on = fq(text, seg, rule)
        finally:
            db.set_option(option, 0)
        mseqs = [masked[int(r[0]):int(r[0] + r[1])].tobytes() for r in recs]
        same_segments(on, expect(mseqs, seg, rule), SEGMENT_VOTE_DTYPE, "masked %d" % option)
        off_masked = fq(masked, seg, rule)
        assert on.records.tobytes() == off_masked.records.tobytes() and on.records.tobytes() != plain.records.tobytes(), option
        assert np.array_equal(on.offsets, plain.offsets)  # (the ranges come from the quality line alone)
    assert fq(text, seg, rule).records.tobytes() == plain.records.tobytes()


# ------------------------------------------------------------------ 8. the device form
def test_device_form(world, db):
    bases, off = world.bases, world.off
    n = off.size - 1
    seg, rule = (100, 50), (2, 25)
    exp = world.exp(seg, rule)
    n_seg = int(exp[0][-1])
    n_hits = int(world.seg._whole()[0].offsets[-1])
    host = call(db, bases, off, seg, rule)
    db.read_segment_votes_time(), db.read_hits_time()
    words = SEGMENT_VOTE_DTYPE.itemsize // 4
    with DeviceBatch(bases, off, n_hits) as d:
        d_so, d_ns = d.dev((n + 1) * 8), d.dev(8)
        canary = np.full((n_seg + 2) * words, CANARY, np.uint32)

        def run(hits_cap, seg_cap):
            d_seg = d.dev(canary.nbytes, canary)
            db.read_segment_votes_device(d.d_bases.value, d.nbytes, d.d_off.value, n, seg[0], seg[1], d_so.value, d.d_tot.value, d_ns.value,
                                         min_hits=rule[0], min_permille=rule[1], d_hits=d.d_hits.value if hits_cap else 0, hits_cap=hits_cap,
                                         d_segments=d_seg.value if seg_cap else 0, seg_cap=seg_cap)
            _lib.check(d.lib.kid_dev_sync(0))
            return (d.down(d_seg, np.uint32, canary.size), d.down(d_so, np.uint64, n + 1), int(d.down(d.d_tot, np.uint64, 1)[0]),
                    int(d.down(d_ns, np.uint64, 1)[0]))

        out, so, nh, ns = run(n_hits, n_seg)
        assert (nh, ns) == (n_hits, n_seg) and np.array_equal(so, exp[0])
        assert out[:n_seg * words].tobytes() == host.records.tobytes() == exp[1].tobytes() and np.all(out[n_seg * words:] == CANARY)
        assert np.all(d.down(d.d_hits, np.uint32, d.canary.size)[n_hits * 3:] == CANARY)
        # one short of either total: both counts are reported and no segment is written; the sizing call
        for hits_cap, seg_cap in [(n_hits - 1, n_seg), (n_hits, n_seg - 1), (0, n_seg), (n_hits, 0)]:
            out, so, nh, ns = run(hits_cap, seg_cap)
            assert (nh, ns) == (n_hits, n_seg) and np.array_equal(so, exp[0]), (hits_cap, seg_cap)
            assert np.all(out == CANARY), (hits_cap, seg_cap)
        ms, calls, reads = db.read_segment_votes_time()
        assert calls == 5 and reads == 5 * n and ms > 0
        assert db.read_hits_time()[1:] == (5, 5 * n)  # the hit pass stays in its own timer
        assert db.read_segments_time()[1] == 0 and db.read_votes_time()[1] == 0


def test_two_streams_share_the_rows_with_the_vote_families(world):
    """segment votes (stream 1) -> votes_from_hits -> fragment_votes_from_hits -> segment votes (stream 2) on one KmerDB,
    nothing waited for in between: every call sends units to its second kernel, the first three of them over rows of the
    same scratch.  All four equal their models."""
    import torch
    rng = np.random.default_rng(88)
    parent = world.parent
    g, keys, tg = genome_world(rng, [8, 6, 5, 36, 35, 8, 6, other_lineage(world)], 6029, 1)
    reads = [g[p:p + h + 29] for p, h in ((0, 700), (800, 600), (1500, 20), (1600, 900), (2600, 5), (2700, 1300))] + [g]
    reads += [rng.choice(sc.ACGT, 100).tobytes()]
    bases, off = concat_reads(reads)
    n = off.size - 1
    w = World(parent, keys, tg, bases, off, 16)
    d = w.db()
    hits = w.hm.batch(bases, off)
    vm = w.seg.vm
    n_hits = int(hits.offsets[-1])
    rule = (2, 25)
    segs = [(WAVE + 88, 64), (1000, 1000)]
    exp = [w.exp(s, rule) for s in segs]
    assert all(regimes(e[1])[2] >= 5 for e in exp)
    exp_votes, exp_frag = vm.batch_anc(hits, rule), FragmentVoteModel(vm).batch_anc(hits, rule)
    assert int((exp_votes["n_hits"] > WAVE).sum()) >= 5 and int((exp_frag["n_hits"] > WAVE).sum()) == 4
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    words = SEGMENT_VOTE_DTYPE.itemsize // 4
    with DeviceBatch(bases, off, n_hits) as a, DeviceBatch(bases, off, n_hits) as b:
        a.run(d, n_hits)  # the hit CSR the two *_from_hits calls read (a's d_ho, d_hits, d_nk)
        outs = []
        for e in exp:
            size = (int(e[0][-1]) + 2) * words
            outs.append((b.dev(size * 4, np.full(size, CANARY, np.uint32)), b.dev((n + 1) * 8), b.dev(8), b.dev(8),
                         b.dev(b.canary.nbytes, b.canary)))
        d_votes = b.dev((n + 2) * 32, np.full((n + 2) * 8, CANARY, np.uint32))
        d_frag = b.dev((n // 2 + 2) * 40, np.full((n // 2 + 2) * 10, CANARY, np.uint32))
        _lib.check(a.lib.kid_dev_sync(0))

        def segment_votes(i, stream):
            d_seg, d_so, d_nh, d_ns, d_hits = outs[i]
            d.read_segment_votes_device(b.d_bases.value, b.nbytes, b.d_off.value, n, segs[i][0], segs[i][1], d_so.value, d_nh.value, d_ns.value,
                                        min_hits=rule[0], min_permille=rule[1], d_hits=d_hits.value, hits_cap=n_hits, d_segments=d_seg.value,
                                        seg_cap=int(exp[i][0][-1]), stream=stream.cuda_stream)

        segment_votes(0, s1)
        d.votes_from_hits_device(a.d_ho.value, a.d_hits.value, a.d_nk.value, n, d_votes.value, min_hits=rule[0], min_permille=rule[1],
                                 stream=s2.cuda_stream)
        d.fragment_votes_from_hits_device(a.d_ho.value, a.d_hits.value, a.d_nk.value, n, d_frag.value, min_hits=rule[0], min_permille=rule[1],
                                          stream=s1.cuda_stream)
        segment_votes(1, s2)
        _lib.check(a.lib.kid_dev_sync(0))
        for i, e in enumerate(exp):
            total = int(e[0][-1])
            got = b.down(outs[i][0], np.uint32, (total + 2) * words)
            assert got[:total * words].tobytes() == e[1].tobytes() and np.all(got[total * words:] == CANARY), segs[i]
            assert np.array_equal(b.down(outs[i][1], np.uint64, n + 1), e[0])
            assert int(b.down(outs[i][2], np.uint64, 1)[0]) == n_hits and int(b.down(outs[i][3], np.uint64, 1)[0]) == total
        got_v = b.down(d_votes, np.uint32, (n + 2) * 8)
        assert got_v[:n * 8].tobytes() == exp_votes.tobytes() and np.all(got_v[n * 8:] == CANARY)
        got_f = b.down(d_frag, np.uint32, (n // 2 + 2) * 10)
        assert got_f[:(n // 2) * 10].view(FRAGMENT_VOTE_DTYPE).tobytes() == exp_frag.tobytes() and np.all(got_f[(n // 2) * 10:] == CANARY)
    # and the host form behind them, on rows that must be zero again
    same_segments(call(d, bases, off, segs[0], rule), exp[0], SEGMENT_VOTE_DTYPE, "host form behind the streams")
    assert VOTE_DTYPE.itemsize == 32
    d.close()


# ------------------------------------------------------------------ 9. errors
def test_error_statuses(world, db):
    bases, off = world.bases[:int(world.off[600])], world.off[:601]

    for seg_len, seg_step in [(0, 1), (10, 0), (10, 11), (2048, 1), (0, 0)]:
        assert status(lambda: db.read_segment_votes(bases, off, seg_len=seg_len, seg_step=seg_step)) == -1, (seg_len, seg_step)
    assert status(lambda: db.read_segment_votes(bases, off, seg_len=10, min_permille=1001)) == -1
    assert len(db.read_segment_votes(bases, off, seg_len=1024, seg_step=1, min_permille=1000)) == 600
    bad = off[:10].copy()
    bad[4] = bad[3] - np.uint64(1)
    assert status(lambda: db.read_segment_votes(bases, bad, seg_len=10)) == -1  # offsets that are not monotone
    n = 9
    start, stop = np.zeros(n, np.int32), (np.diff(off[:n + 1].astype(np.int64)) - 1).astype(np.int32)
    stop[2] += 1  # one past the read
    assert status(lambda: db.read_segment_votes(bases, off[:n + 1], start, stop, seg_len=10)) == -1
    text, recs = fastq_block([bases[int(off[3]):int(off[4])].tobytes()] * 4, [b"I" * int(off[4] - off[3])] * 4, eol=b"\r\n", blank_every=5)
    assert len(db.read_segment_votes_fastq(text, recs, seg_len=10)) == 4
    for seg_len, seg_step in [(0, 1), (10, 0), (10, 11), (2048, 1)]:
        assert status(lambda: db.read_segment_votes_fastq(text, recs, seg_len=seg_len, seg_step=seg_step)) == -1
    recs[2, 3] -= 1  # a quality line shorter than its sequence
    assert status(lambda: db.read_segment_votes_fastq(text, recs, seg_len=10)) == -9
    lib = _lib.load()
    so, tot = np.full(2, 7, np.uint64), C.c_uint64(7)
    assert lib.kid_db_read_segment_votes(db._h, None, None, None, None, 1 << 31, 10, 10, 0, 0, so.ctypes.data, None, 0, C.byref(tot)) == -1
    assert lib.kid_db_read_segment_votes(None, None, None, None, None, 0, 10, 10, 0, 0, so.ctypes.data, None, 0, C.byref(tot)) == -1
    assert lib.kid_db_read_segment_votes(db._h, None, None, None, None, 0, 10, 10, 0, 0, so.ctypes.data, None, 5, C.byref(tot)) == -1  # cap without a buffer
    assert lib.kid_db_read_segment_votes(db._h, None, None, None, None, 0, 10, 11, 0, 0, so.ctypes.data, None, 0, C.byref(tot)) == -1
    assert lib.kid_db_read_segment_votes_fastq(None, None, 0, None, 0, 10, 10, 0, 0, so.ctypes.data, None, 0, C.byref(tot)) == -1
    assert lib.kid_db_read_segment_votes_fastq(db._h, None, 0, None, 1 << 31, 10, 10, 0, 0, so.ctypes.data, None, 0, C.byref(tot)) == -1
    assert so.tolist() == [7, 7] and tot.value == 7  # nothing written
    assert lib.kid_db_read_segment_votes(db._h, None, None, None, None, 0, 10, 10, 0, 0, so.ctypes.data, None, 0, C.byref(tot)) == 0
    assert so.tolist() == [0, 7] and tot.value == 0  # n_reads = 0
    assert lib.kid_db_read_segment_votes_device(None, None, 0, None, None, None, 0, 10, 10, 0, 0, None, 0, None, None, 0, None, None, None) == -1
    assert lib.kid_db_read_segment_votes_time(None, None, None, None) == -1
    with DeviceBatch(bases, off, 4) as d:
        d_so, d_ns = d.dev(601 * 8), d.dev(8)
        dev = lambda *geo: lib.kid_db_read_segment_votes_device(db._h, d.d_bases, d.nbytes, d.d_off, None, None, 600, *geo, None, 0, d_so, None,  # noqa: E731
                                                                0, d.d_tot, d_ns, None)
        for geo in [(0, 1, 0, 0), (10, 0, 0, 0), (10, 11, 0, 0), (2048, 1, 0, 0), (10, 10, 0, 1001)]:
            assert dev(*geo) == -1, geo
        assert lib.kid_db_read_segment_votes_device(db._h, d.d_bases, d.nbytes, d.d_off, None, None, 1 << 31, 10, 10, 0, 0, None, 0, d_so, None, 0,
                                                    d.d_tot, d_ns, None) == -1
        assert lib.kid_db_read_segment_votes_device(db._h, d.d_bases, d.nbytes, d.d_off, None, None, 600, 10, 10, 0, 0, None, 4, d_so, None, 0,
                                                    d.d_tot, d_ns, None) == -1  # hits_cap without a buffer
        assert lib.kid_db_read_segment_votes_device(db._h, d.d_bases, d.nbytes, d.d_off, None, None, 600, 10, 10, 0, 0, None, 0, d_so, None, 4,
                                                    d.d_tot, d_ns, None) == -1  # seg_cap without a buffer
        assert dev(10, 10, 0, 0) == 0  # (the sizing call of the device form)
        _lib.check(d.lib.kid_dev_sync(0))
        assert int(d.down(d_ns, np.uint64, 1)[0]) == int(db.read_segment_votes(bases, off, seg_len=10).offsets[-1])


# ------------------------------------------------------------------ 10. the sizing convention, splits, repeats
def test_sizing_splits_and_repeats(world, db):
    lib = _lib.load()
    bases, off = world.bases, world.off
    n = off.size - 1
    exp = world.exp((65, 13), (2, 25))
    total = int(exp[0][-1])
    words = SEGMENT_VOTE_DTYPE.itemsize // 4
    so = np.full(n + 1, 7, np.uint64)
    tot = C.c_uint64(0)
    small = np.full((total - 1) * words, CANARY, np.uint32)
    args = (db._h, bases.ctypes.data, off.ctypes.data, None, None, n, 65, 13, 2, 25, so.ctypes.data)
    assert lib.kid_db_read_segment_votes(*args, small.ctypes.data, total - 1, C.byref(tot)) == 0
    assert tot.value == total and np.array_equal(so, exp[0]) and np.all(small == CANARY)  # nothing written, the count is right
    assert lib.kid_db_read_segment_votes(*args, None, 0, C.byref(tot)) == 0 and tot.value == total
    full = np.zeros(total + 2, SEGMENT_VOTE_DTYPE)
    full[-2:] = 0xA5
    assert lib.kid_db_read_segment_votes(*args, full.ctypes.data, total, C.byref(tot)) == 0
    assert full[:total].tobytes() == exp[1].tobytes() and np.all(full[-2:].view(np.uint32) == 0xA5)
    # three calls give the concatenation; a repeat gives identical bytes
    cuts = [0, n // 3, n // 3 + 65, n]
    parts = [call(db, bases, off[a:b + 1], (65, 13), (2, 25)) for a, b in zip(cuts[:-1], cuts[1:])]
    assert b"".join(p.records.tobytes() for p in parts) == exp[1].tobytes()
    assert np.array_equal(np.concatenate([np.diff(p.offsets.astype(np.int64)) for p in parts]), np.diff(exp[0].astype(np.int64)))
    again = call(db, bases, off, (65, 13), (2, 25))
    assert again.records.tobytes() == exp[1].tobytes() and again.offsets.tobytes() == exp[0].tobytes()
    # trimmed ranges: pos is counted from the first byte of the read
    lens = np.diff(off.astype(np.int64))
    start = np.minimum(5, np.maximum(lens - 1, 0)).astype(np.int32)
    stop = np.maximum(lens - 3, start).astype(np.int32)
    stop[lens == 0] = 0
    start[lens == 0] = 0
    ok = lens > 0
    b2, o2 = concat_reads([bases[int(off[r]):int(off[r + 1])].tobytes() for r in np.flatnonzero(ok)])
    model = SegmentVoteModel(world.sm, b2, o2, start[ok], stop[ok])
    same_segments(call(db, b2, o2, (40, 20), (2, 25), start[ok], stop[ok]), model.direct(40, 20, (2, 25)), SEGMENT_VOTE_DTYPE, "trimmed")


# ------------------------------------------------------------------ 11. the timer
def test_time_counts_calls_and_reads(world, db):
    bases, off = world.bases, world.off
    n = off.size - 1
    db.read_segment_votes_time(), db.read_segments_time(), db.read_votes_time(), db.read_support_time()
    call(db, bases, off, (100, 50), (2, 25))
    call(db, bases, off[:101], (100, 50), (2, 25))
    ms, calls, reads = db.read_segment_votes_time()
    assert calls == 4 and reads == 2 * (n + 100) and ms > 0  # (read_segment_votes is the sizing call and the filling call)
    assert db.read_segment_votes_time() == (0.0, 0, 0)
    assert db.read_segments_time()[1] == 0 and db.read_votes_time()[1] == 0 and db.read_support_time()[1] == 0
