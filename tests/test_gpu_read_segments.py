"""kid_db_read_segments* (records called in segments) against the independent model of tests/read_segments_model.py
(its direct form), against kid_db_read_support of the same library, and against its own contract.  Every comparison is
exact: integers."""
import ctypes as C

import numpy as np
import pytest

import read_calls
import read_support_cases as sc
from base_quality_cases import hit_reads, mask_block
from helpers import DeviceBatch, concat_reads, fastq_block, oracle_db
from kmer_id_amd import KID_DB_OPT_MIN_BASE_QUALITY, KID_FLAG_REF_GEOMETRY, KmerDB, _lib
from kmer_id_amd.api import SEGMENT_DTYPE, SUPPORT_DTYPE
from read_calls import KINDS, genome_world, header_constant, same_segments, status
from read_hits_model import HitModel, trim_ranges
from read_segments_model import SegmentModel
from read_support_model import SupportModel

pytestmark = pytest.mark.gpu

SETTINGS = [(1, 1), (63, 63), (64, 64), (65, 13), (100, 50), (121, 121), (10 ** 6, 10 ** 6)]
RULES = [(0, 0), (2, 25)]
LANE_HITS = header_constant("kid_support.hip.h", "KID_SUPPORT_LANE_HITS")


def call(db, bases, off, seg, rule, start=None, stop=None):
    return db.read_segments(bases, off, start, stop, seg_len=seg[0], seg_step=seg[1], min_hits=rule[0], min_permille=rule[1])


class World(read_calls.World):
    """a database, its models and a batch of reads; the model's segments per (setting, rule) are computed once"""

    def __init__(self, parent, keys, targets, bases, off, log2_slots, start=None, stop=None):
        super().__init__(parent, keys, targets, bases, off, log2_slots)
        self.seg = SegmentModel(self.sm, bases, off, start, stop)
        self.start, self.stop = start, stop
        self._exp = {}

    def exp(self, seg, rule):
        if (seg, rule) not in self._exp:
            self._exp[(seg, rule)] = self.seg.direct(seg[0], seg[1], rule)
        return self._exp[(seg, rule)]

    def check(self, db, settings, rules, what=""):
        for seg in settings:
            for rule in rules:
                same_segments(call(db, self.bases, self.off, seg, rule, self.start, self.stop), self.exp(seg, rule), SEGMENT_DTYPE,
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


# ------------------------------------------------------------------ 1. the model, three table kinds
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_segments_equal_the_model(world, kind):
    assert world.off.size - 1 == 2605
    d = world.db(KINDS[kind])
    world.check(d, SETTINGS, RULES, kind)
    # one segment per read: the six shared fields are kid_db_read_support's of the same call
    for rule in RULES:
        got = call(d, world.bases, world.off, (10 ** 6, 10 ** 6), rule)
        sup = d.read_support(world.bases, world.off, min_hits=rule[0], min_permille=rule[1])
        has = sup["n_kmers"] > 0
        # (a read of k or more bytes that are not all bases has windows, a segment, and n_kmers = 0)
        per = np.diff(got.offsets.astype(np.int64))
        assert np.all(per <= 1) and np.all(per[has] == 1) and not sup["n_hits"][per == 0].any()
        for f in SUPPORT_DTYPE.names:
            assert np.array_equal(got.records[f], sup[f][per == 1]), (rule, f)
        assert not got.records["pos"].any() and np.array_equal(got.records["n_pos"], world.seg.P[per == 1])
    e = world.exp((100, 50), (2, 25))[1]
    assert int((e["confident"] != e["final"]).sum()) > 0 and int((e["n_hits"] == 0).sum()) > 1000  # the rule bites; the list is dense
    d.close()


# ------------------------------------------------------------------ 2. tile edges
def test_tile_edges(world):
    rng = np.random.default_rng(6464)
    parent = world.parent
    g, keys, tg = genome_world(rng, [8, 6, 5, 36, 35, 8, 6, 1], 4000, 1)
    d = KmerDB(keys, tg, parent, k=30, log2_slots=16)
    odb = oracle_db(parent, keys, tg, 16)
    sm = SupportModel(HitModel(odb, keys, tg, 30), parent)
    for P in (1, 63, 64, 65, 127, 128, 129, 192):
        p0 = int(rng.integers(0, len(g) - (P + 29)))
        stretch = g[p0:p0 + P + 29]
        with_n = bytearray(stretch)
        for m in range(64, len(stretch), 64):  # an N exactly at, and one base before, every multiple of 64 from the read's start
            with_n[m] = with_n[m - 1] = ord("N")
        for copy, seq in (("plain", stretch), ("N", bytes(with_n))):
            # twice, a read of fewer than k bases and an empty one in between; the second is the batch's last read
            bases, off = concat_reads([seq, b"ACGTACGTAC", b"", seq])
            model = SegmentModel(sm, bases, off)
            for seg_len in (1, 32, 64, 65, 128):
                for seg_step in sorted({1, seg_len} | ({64} if 64 <= seg_len else set())):
                    if seg_len > 1024 * seg_step:
                        continue
                    for rule in [(0, 0), (2, 25)]:
                        exp = model.direct(seg_len, seg_step, rule)
                        what = "P %d %s %d:%d %s" % (P, copy, seg_len, seg_step, rule)
                        same_segments(call(d, bases, off, (seg_len, seg_step), rule), exp, SEGMENT_DTYPE, what)
                        rec = exp[1]
                        assert int(exp[0][1]) * 2 == rec.size == int(exp[0][4]) and exp[0][1] == exp[0][2] == exp[0][3], what
                        if copy == "plain":
                            assert np.array_equal(rec["n_kmers"], rec["n_pos"]) and np.array_equal(rec["n_hits"], rec["n_pos"]), what
                        elif P > 35:
                            # the windows 34 .. 64 hold the N at bytes 63, 64: a segment that covers one of them counts fewer k-mers
                            around = (rec["pos"] <= 64) & (rec["pos"] + rec["n_pos"] > 34)
                            assert around.any() and np.all(rec["n_kmers"][around] < rec["n_pos"][around]), what
    d.close()


# ------------------------------------------------------------------ 3. the work split
def test_work_split(world):
    rng = np.random.default_rng(640)
    parent = world.parent
    x = next(int(t) for t in world.targets if t > 1 and sc.top_level(parent, int(t)) != 5)
    g, keys, tg = genome_world(rng, [8, 6, 5, 36, 35, 8, 6, x], 4000, 1)
    counts = [LANE_HITS - 1, LANE_HITS, LANE_HITS + 1, 63, 64, 65, 200]

    def dense(h):
        p = int(rng.integers(0, len(g) - (h + 29)))
        return g[p:p + h + 29]

    d = KmerDB(keys, tg, parent, k=30, log2_slots=16)
    sm = SupportModel(HitModel(oracle_db(parent, keys, tg, 16), keys, tg, 30), parent)
    for i in range(len(counts)):
        # fillers without a hit: one segment each up to read 64; behind it every other one is empty or shorter than k
        batch = [rng.choice(sc.ACGT, 100).tobytes() if j <= 64 or j % 3 == 0 else (b"", b"ACGT")[j % 2] for j in range(260)]
        batch[0], batch[63], batch[64] = dense(counts[i]), dense(counts[(i + 1) % 7]), dense(counts[(i + 2) % 7])
        batch[198] = dense(counts[(i + 3) % 7])
        bases, off = concat_reads(batch)
        model = SegmentModel(sm, bases, off)
        for rule in [(0, 0), (3, 0), (2, 25), (0, 1000)]:
            exp = model.direct(300, 300, rule)
            assert exp[1].size >= 130 and [int(exp[0][j]) for j in (0, 63, 64)] == [0, 63, 64]
            assert [int(exp[1]["n_hits"][j]) for j in (0, 63, 64)] == [counts[i], counts[(i + 1) % 7], counts[(i + 2) % 7]]
            assert int(exp[1]["n_hits"][1:63].sum()) == 0
            same_segments(call(d, bases, off, (300, 300), rule), exp, SEGMENT_DTYPE, "batch %d rule %s" % (i, rule))
    # the same counts as segments INSIDE one record: stretches of the genome between hit-free spacers of 300 bases
    parts = []
    for h in counts:
        parts += [dense(h), rng.choice(sc.ACGT, 300).tobytes()]
    bases, off = concat_reads([b"".join(parts)] + [rng.choice(sc.ACGT, 100).tobytes() for _ in range(3)])
    model = SegmentModel(sm, bases, off)
    for seg in [(64, 64), (229, 1), (300, 150)]:
        for rule in [(0, 0), (3, 0), (2, 25)]:
            exp = model.direct(seg[0], seg[1], rule)
            same_segments(call(d, bases, off, seg, rule), exp, SEGMENT_DTYPE, "one record %s rule %s" % (seg, rule))
    assert int(model.direct(229, 1, (0, 0))[1]["n_hits"].max()) >= 200
    # no read at all; reads without a window only
    empty = d.read_segments(np.zeros(0, np.uint8), np.zeros(1, np.uint64), seg_len=5)
    assert empty.records.size == 0 and empty.offsets.tolist() == [0]
    bases, off = concat_reads([b"", b"ACGT", b""])
    none = d.read_segments(bases, off, seg_len=5)
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


# ------------------------------------------------------------------ 5. a chimera
def test_a_chimera(world):
    rng = np.random.default_rng(3000)
    parent = world.parent
    x = next(int(t) for t in world.targets if t > 1 and sc.top_level(parent, int(t)) != 5)
    ga, ka, ta = genome_world(rng, [8, 6, 5], 3000, 1)
    gb, kb, tb = genome_world(rng, [x], 3000, 1)
    keys, tg = np.concatenate([ka, kb]), np.concatenate([ta, tb])
    bases, off = concat_reads([rng.choice(sc.ACGT, 150).tobytes(), ga + gb, rng.choice(sc.ACGT, 150).tobytes()])
    w = World(parent, keys, tg, bases, off, 16)
    d = w.db()
    for rule in [(0, 0), (0, 600)]:
        got = call(d, bases, off, (500, 250), rule)
        same_segments(got, w.exp((500, 250), rule), SEGMENT_DTYPE, "chimera %s" % (rule,))
        rec = got.of(1)
        assert rec.size == 23 and int(rec["pos"][-1] + rec["n_pos"][-1]) == 6000 - 29
        left = rec[rec["pos"] + rec["n_pos"] + 29 <= 3000]   # every window inside the first genome
        right = rec[rec["pos"] >= 3000]
        assert left.size >= 9 and right.size >= 9
        assert set(left["final"].tolist()) <= {5, 6, 8} and set(left["confident"].tolist()) <= {5, 6, 8}
        assert np.all(right["final"] == x) and np.all(right["confident"] == x)
    whole = d.read_support(bases, off, min_permille=600)[1]
    # the record as a whole: msca keeps the deeper node of a lineage, so final is the second lineage's; the rule says the root
    assert int(whole["final"]) == x and int(whole["confident"]) == 1 and int(whole["s_confident"]) == int(whole["n_hits"])
    d.close()


# ------------------------------------------------------------------ 6. trees
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
    for _ in range(200):
        pick = rng.integers(0, keys.size, int(rng.integers(1, 15)))
        seqs.append(sc.implanted(rng, [sc.cases.key_seq(keys[j], 30) for j in pick]))
    bases, off = concat_reads(seqs)
    w = World(parent, keys, tg, bases, off, 12)
    e = w.exp((40, 20), (2, 0))[1]
    assert int((e["n_hits"] > 1).sum()) > 50 and int(((e["confident"] != e["final"]) & (e["confident"] > 0)).sum()) > 0
    for flags in (0, KID_FLAG_REF_GEOMETRY):
        d = w.db(flags)
        assert d.info.tree_depth == depth
        w.check(d, [(40, 20), (10 ** 6, 10 ** 6)], [(0, 0), (2, 0), (2, 25)], "depth %d flags %d" % (depth, flags))
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
    start, stop, keep = trim_ranges(quals, [len(s) for s in seqs], 30)
    assert 0 < int((~keep).sum()) and int(keep.sum()) > 800
    text, recs = fastq_block(seqs, quals, eol=b"\r\n", blank_every=5)  # CRLF line ends, blank lines between records

    def expect(the_seqs, seg, rule):
        b, o = concat_reads(the_seqs)
        return SegmentModel(world.sm, b, o, start, stop, keep).direct(seg[0], seg[1], rule)

    for seg, rule in [((40, 20), (0, 0)), ((64, 64), (2, 25)), ((10 ** 6, 10 ** 6), (2, 25))]:
        got = db.read_segments_fastq(text, recs, seg_len=seg[0], seg_step=seg[1], min_hits=rule[0], min_permille=rule[1])
        same_segments(got, expect(seqs, seg, rule), SEGMENT_DTYPE, "fastq %s %s" % (seg, rule))
        per = np.diff(got.offsets.astype(np.int64))
        assert not per[~keep].any() and np.all(per[keep] >= 1)  # a dropped record has no segment
        assert np.array_equal(got.records["pos"][got.offsets[:-1][keep].astype(np.int64)], start[keep])
    # masked bases: the records are those on the text with the masked bases replaced by N
    masked, n_masked = mask_block(text, recs, 20)
    assert n_masked > 0
    mseqs = [masked[int(r[0]):int(r[0] + r[1])].tobytes() for r in recs]
    plain = db.read_segments_fastq(text, recs, seg_len=40, seg_step=20, min_hits=2, min_permille=25)
    db.set_option(KID_DB_OPT_MIN_BASE_QUALITY, 20)
    try:
        on = db.read_segments_fastq(text, recs, seg_len=40, seg_step=20, min_hits=2, min_permille=25)
    finally:
        db.set_option(KID_DB_OPT_MIN_BASE_QUALITY, 0)
    same_segments(on, expect(mseqs, (40, 20), (2, 25)), SEGMENT_DTYPE, "masked")
    off_masked = db.read_segments_fastq(masked, recs, seg_len=40, seg_step=20, min_hits=2, min_permille=25)
    assert on.records.tobytes() == off_masked.records.tobytes() and on.records.tobytes() != plain.records.tobytes()
    assert np.array_equal(on.offsets, plain.offsets)  # (the ranges come from the quality line alone)


# ------------------------------------------------------------------ 8. the sizing convention, splits, repeats
def test_sizing_splits_and_repeats(world, db):
    lib = _lib.load()
    bases, off = world.bases, world.off
    n = off.size - 1
    exp = world.exp((65, 13), (2, 25))
    total = int(exp[0][-1])
    so = np.full(n + 1, 7, np.uint64)
    tot = C.c_uint64(0)
    small = np.full((total - 1) * 8, 0xA5A5A5A5, np.uint32)
    args = (db._h, bases.ctypes.data, off.ctypes.data, None, None, n, 65, 13, 2, 25, so.ctypes.data)
    assert lib.kid_db_read_segments(*args, small.ctypes.data, total - 1, C.byref(tot)) == 0
    assert tot.value == total and np.array_equal(so, exp[0]) and np.all(small == 0xA5A5A5A5)  # nothing written, the count is right
    assert lib.kid_db_read_segments(*args, None, 0, C.byref(tot)) == 0 and tot.value == total
    full = np.zeros(total + 2, SEGMENT_DTYPE)
    full[-2:] = 0xA5
    assert lib.kid_db_read_segments(*args, full.ctypes.data, total, C.byref(tot)) == 0
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
    sel = np.flatnonzero(ok)
    b2, o2 = concat_reads([bases[int(off[r]):int(off[r + 1])].tobytes() for r in sel])
    model = SegmentModel(world.sm, b2, o2, start[ok], stop[ok])
    same_segments(call(db, b2, o2, (40, 20), (2, 25), start[ok], stop[ok]), model.direct(40, 20, (2, 25)), SEGMENT_DTYPE, "trimmed")


# ------------------------------------------------------------------ 9. the device form, the timer
def test_device_form_and_time(world, db):
    bases, off = world.bases, world.off
    n = off.size - 1
    seg, rule = (100, 50), (2, 25)
    exp = world.exp(seg, rule)
    n_seg = int(exp[0][-1])
    n_hits = int(world.seg._whole()[0].offsets[-1])
    host = call(db, bases, off, seg, rule)
    db.read_segments_time(), db.read_hits_time()
    with DeviceBatch(bases, off, n_hits) as d:
        d_so, d_ns = d.dev((n + 1) * 8), d.dev(8)
        canary = np.full((n_seg + 2) * 8, 0xA5A5A5A5, np.uint32)

        def run(hits_cap, seg_cap):
            d_seg = d.dev(canary.nbytes, canary)
            db.read_segments_device(d.d_bases.value, d.nbytes, d.d_off.value, n, seg[0], seg[1], d_so.value, d.d_tot.value, d_ns.value,
                                    min_hits=rule[0], min_permille=rule[1], d_hits=d.d_hits.value if hits_cap else 0, hits_cap=hits_cap,
                                    d_segments=d_seg.value if seg_cap else 0, seg_cap=seg_cap)
            _lib.check(d.lib.kid_dev_sync(0))
            return (d.down(d_seg, np.uint32, canary.size), d.down(d_so, np.uint64, n + 1), int(d.down(d.d_tot, np.uint64, 1)[0]),
                    int(d.down(d_ns, np.uint64, 1)[0]))

        out, so, nh, ns = run(n_hits, n_seg)
        assert (nh, ns) == (n_hits, n_seg) and np.array_equal(so, exp[0])
        assert out[:n_seg * 8].tobytes() == host.records.tobytes() == exp[1].tobytes() and np.all(out[n_seg * 8:] == 0xA5A5A5A5)
        assert np.all(d.down(d.d_hits, np.uint32, d.canary.size)[n_hits * 3:] == 0xA5A5A5A5)
        for hits_cap, seg_cap in [(n_hits - 1, n_seg), (n_hits, n_seg - 1), (0, n_seg), (n_hits, 0)]:
            out, so, nh, ns = run(hits_cap, seg_cap)
            assert (nh, ns) == (n_hits, n_seg) and np.array_equal(so, exp[0]), (hits_cap, seg_cap)  # both counts are reported
            assert np.all(out == 0xA5A5A5A5), (hits_cap, seg_cap)                                      # and no segment is written
        ms, calls, reads = db.read_segments_time()
        assert calls == 5 and reads == 5 * n and ms > 0
        assert db.read_segments_time() == (0.0, 0, 0)
        hms, hcalls, hreads = db.read_hits_time()
        assert hcalls == 5 and hreads == 5 * n  # the hit pass stays in its own timer
    call(db, bases, off, seg, rule)
    call(db, bases, off[:101], seg, rule)
    ms, calls, reads = db.read_segments_time()
    assert calls == 4 and reads == 2 * (n + 100) and ms > 0  # (read_segments is the sizing call and the filling call)
    assert db.read_segments_time() == (0.0, 0, 0)
    assert db.read_support_time()[1] == 0


# ------------------------------------------------------------------ 10. errors
def test_error_statuses(world, db):
    bases, off = world.bases[:int(world.off[600])], world.off[:601]

    for seg_len, seg_step in [(0, 1), (10, 0), (10, 11), (2048, 1), (0, 0)]:
        assert status(lambda: db.read_segments(bases, off, seg_len=seg_len, seg_step=seg_step)) == -1, (seg_len, seg_step)
    assert status(lambda: db.read_segments(bases, off, seg_len=10, min_permille=1001)) == -1
    assert len(db.read_segments(bases, off, seg_len=1024, seg_step=1, min_permille=1000)) == 600
    bad = off[:10].copy()
    bad[4] = bad[3] - np.uint64(1)
    assert status(lambda: db.read_segments(bases, bad, seg_len=10)) == -1  # offsets that are not monotone
    n = 9
    start, stop = np.zeros(n, np.int32), (np.diff(off[:n + 1].astype(np.int64)) - 1).astype(np.int32)
    stop[2] += 1  # one past the read
    assert status(lambda: db.read_segments(bases, off[:n + 1], start, stop, seg_len=10)) == -1
    text, recs = fastq_block([bases[int(off[3]):int(off[4])].tobytes()] * 4, [b"I" * int(off[4] - off[3])] * 4, eol=b"\r\n", blank_every=5)
    assert len(db.read_segments_fastq(text, recs, seg_len=10)) == 4
    for seg_len, seg_step in [(0, 1), (10, 0), (10, 11), (2048, 1)]:
        assert status(lambda: db.read_segments_fastq(text, recs, seg_len=seg_len, seg_step=seg_step)) == -1
    recs[2, 3] -= 1  # a quality line shorter than its sequence
    assert status(lambda: db.read_segments_fastq(text, recs, seg_len=10)) == -9
    lib = _lib.load()
    so, tot = np.zeros(2, np.uint64), C.c_uint64(0)
    assert lib.kid_db_read_segments(db._h, None, None, None, None, 1 << 31, 10, 10, 0, 0, so.ctypes.data, None, 0, C.byref(tot)) == -1
    assert lib.kid_db_read_segments(None, None, None, None, None, 0, 10, 10, 0, 0, so.ctypes.data, None, 0, C.byref(tot)) == -1
    assert lib.kid_db_read_segments_fastq(None, None, 0, None, 0, 10, 10, 0, 0, so.ctypes.data, None, 0, C.byref(tot)) == -1
    assert lib.kid_db_read_segments_fastq(db._h, None, 0, None, 1 << 31, 10, 10, 0, 0, so.ctypes.data, None, 0, C.byref(tot)) == -1
    assert lib.kid_db_read_segments_device(None, None, 0, None, None, None, 0, 10, 10, 0, 0, None, 0, None, None, 0, None, None, None) == -1
    assert lib.kid_db_read_segments_time(None, None, None, None) == -1
    with DeviceBatch(bases, off, 4) as d:
        d_so, d_ns = d.dev(601 * 8), d.dev(8)
        dev = lambda *geo: lib.kid_db_read_segments_device(db._h, d.d_bases, d.nbytes, d.d_off, None, None, 600, *geo, None, 0, d_so, None, 0,  # noqa: E731
                                                           d.d_tot, d_ns, None)
        for geo in [(0, 1, 0, 0), (10, 0, 0, 0), (10, 11, 0, 0), (2048, 1, 0, 0), (10, 10, 0, 1001)]:
            assert dev(*geo) == -1, geo
        assert lib.kid_db_read_segments_device(db._h, d.d_bases, d.nbytes, d.d_off, None, None, 1 << 31, 10, 10, 0, 0, None, 0, d_so, None, 0,
                                               d.d_tot, d_ns, None) == -1
        assert dev(10, 10, 0, 0) == 0  # (the sizing call of the device form)
        _lib.check(d.lib.kid_dev_sync(0))
