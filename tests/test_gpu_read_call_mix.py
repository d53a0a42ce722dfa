"""The five families of calls over the hit pass -- kid_db_read_hits*, kid_db_read_support*, kid_db_read_segments*,
kid_db_read_fragments*, kid_db_read_votes* -- mixed on one kid_db with one tally sample: they share the database's lock,
its grow-only scratch, the `want_valid` switch of the hit pass and five timers, and no other test crosses from one family
into the next.  Two tests: the first four families alone, then all five.

test_mixed_calls_share_one_state: one seeded sequence of 41 calls: every entry point of the four families (host buffers, FASTQ blocks, device memory; with
and without a tally), a segments call directly before and directly after every call of another family, batch sizes that go
up and down (1, 2, 64, 65, 257, 1030 reads, then 2 again; a batch of fragments has the next even number).  The batches are
slices of the read-fragments pool (read_fragments_cases.fragments over read_support_cases.database: the ragged reads of
read_hits_cases, synthetic reads and the hand-built mates).  Every output is compared for equality with the independent
models (HitModel, SupportModel, SegmentModel, FragmentModel), the tally's gcount and seen bits with a SampleMirror, and
after every call each of the four *_time queries must report exactly the calls and reads made since it was last asked.

test_mixed_calls_with_votes_share_one_state: the vote calls are the only family with a hook of its own on the shared call
path, a second kernel and scratch of its own (a list, a counter, one row per compute unit).  A pool of its own (VotePool:
the reads above over a database that also holds every window of a small genome, and six stretches of that genome with
more hits than KID_VOTE_WAVE_HITS, so that the second vote kernel has reads) and a seeded sequence of 56 calls: the five
families in three forms, each at least twice; in the first 49 a segments call in front of and behind every call of
another family, in the last 7 a vote call directly in front of and behind a call of each other family; the same batch
sizes; every other host and FASTQ call of support, fragments and votes tallies into the one sample, the mirror counting a
vote call with the vote record's `confident`.  After every call all five *_time queries report exactly that call; at the
end kid_sample_end equals the mirror.

test_vote_families_alternate_on_one_scratch: the three families with a second kernel -- votes, fragment votes, segment
votes -- alternate twice on one kid_db.  Each binds a list, a counter and rows through the same function; the segment
votes bind the rows of the votes.  Every batch holds one unit for the second kernel (KID_VOTE_WAVE_HITS + 1 hits) and one for
a lane; the records equal those of the same call on a database that has seen no other call."""
from types import SimpleNamespace

import numpy as np
import pytest

import read_fragments_cases as fc
import read_support_cases as sc
from helpers import DeviceBatch, concat_reads, fastq_block, oracle_db
from hit_list_cases import LANE_HITS, WAVE_HITS
from kmer_id_amd import FRAGMENT_DTYPE, FRAGMENT_VOTE_DTYPE, SEGMENT_VOTE_DTYPE, VOTE_DTYPE, KmerDB, _lib
from kmer_id_amd.api import SEGMENT_DTYPE, SUPPORT_DTYPE
from read_calls import genome_world, same_records
from read_depth_model import depth_of
from read_fragments_model import FragmentModel, fragment_csr
from read_hits_model import HitModel, Hits, trim_ranges, windows
from read_segments_model import SegmentModel
from read_support_model import SupportModel
from read_votes_model import VoteModel
from sample_life import N_ENTRIES, SampleMirror, csr_take

pytestmark = pytest.mark.gpu

K = sc.K
SIZES = [1, 2, 64, 65, 257, 1030, 2]
RULES = [(0, 0), (2, 25)]
SEGS = [(100, 50), (64, 64)]
FAMILIES = ("hits", "support", "segments", "fragments")
FORMS = ("host", "fastq", "device")
SEED = 20264
VOTE_SEED = 20270  # the first behind SEED whose plan has reads for the second vote kernel where the test below wants them


class Facts:
    """the hits of every read of the pool under one input form, and its support record under every rule (with a vote
    model: its vote record too)"""

    def __init__(self, sm, hits, vm=None):
        self.hits = hits
        finals = sm.finals(hits)
        self.rec = {rule: sm.batch_identity(hits, rule, finals) for rule in RULES}
        if vm:
            calls = vm.calls_anc(hits)
            self.votes = {rule: vm.batch_anc(hits, rule, calls) for rule in RULES}

    def sub(self, a, n):
        """the CSR of the reads [a, a + n)"""
        idx, per = csr_take(self.hits.offsets, np.arange(a, a + n))
        off = np.zeros(n + 1, np.uint64)
        off[1:] = np.cumsum(per)
        h = self.hits
        return Hits(off, h.n_kmers[a:a + n], h.pos[idx], h.target[idx], h.entry[idx])


class Pool:
    def __init__(self):
        parent, cum, keys, targets = sc.database()
        bases, off, _ = fc.fragments(parent, cum, keys, targets)
        self.build(parent, keys, targets, bases, off)

    def build(self, parent, keys, targets, bases, off, votes=False):
        self.parent, self.keys, self.targets, self.ntar = parent, keys, targets, parent.size
        self.bases, self.off = bases, off
        self.n = self.off.size - 1
        self.hm = HitModel(oracle_db(parent, keys, targets, 20), keys, targets, K)
        self.sm = SupportModel(self.hm, parent)
        self.fm = FragmentModel(self.sm)
        vm = VoteModel(self.sm) if votes else None
        self.plain = Facts(self.sm, self.hm.batch(self.bases, self.off), vm)
        # as records of a FASTQ block with qualities that trim nothing: process_qual still drops what is not longer than k
        raw = bytes(self.bases)
        self.seqs = [raw[int(self.off[r]):int(self.off[r + 1])] for r in range(self.n)]
        self.quals = [b"I" * len(s) for s in self.seqs]
        self.start, self.stop, self.keep = trim_ranges(self.quals, [len(s) for s in self.seqs], K)
        st, sp = self.start.copy(), self.stop.copy()
        st[~self.keep], sp[~self.keep] = 0, -1  # a dropped record has no window and no hit
        self.fastq = Facts(self.sm, self.hm.batch(self.bases, self.off, st, sp), vm)

    def mirror_world(self):
        """what a SampleMirror reads of its world; its bitmap has sample_life.N_ENTRIES bits, of which this database uses the first"""
        targets = np.zeros(N_ENTRIES, np.uint32)
        targets[:self.targets.size] = self.targets
        return SimpleNamespace(ntar=self.ntar, hits=self.plain.hits, rec=self.plain.rec, sm=self.sm, targets=targets)

    def db(self):
        return KmerDB(self.keys, self.targets, self.parent, k=K, log2_slots=20)


class Mirror(SampleMirror):
    def count(self, hits, rec, counted):
        """units counted as a tally counts them: hits is the CSR of the units, rec their records"""
        self.gcount += self.w.sm.tally(hits, rec, counted, self.w.targets)[0]
        self.seen |= depth_of(hits, rec, counted, N_ENTRIES) > 0


class VotePool(Pool):
    """a pool in which the second vote kernel runs: the database of Pool plus every window of a seeded genome of 800 bases
    under targets drawn from 8, 6, 5, 36, 35 and X (a node of another top-level lineage) -- a stretch of h + 29 bases of the
    genome is a read of h hits -- and among Pool's reads six such stretches of more than KID_VOTE_WAVE_HITS hits, each with
    a shorter stretch as its mate, alternately as mate 1 and mate 2"""
    GENOME_LEN = 800
    BIG = [(WAVE_HITS + 1, 0), (WAVE_HITS + 40, 3), (600, 40), (700, 70), (771, 9), (WAVE_HITS + 2, 200)]  # hits of the stretch and of its mate

    def __init__(self):
        parent, cum, keys, targets = sc.database()
        bases, off, _ = fc.fragments(parent, cum, keys, targets)
        rng = np.random.default_rng(VOTE_SEED)
        first = np.sort(np.unique(keys, return_index=True)[1])
        x = next(int(t) for t in targets[first] if t > 1 and sc.top_level(parent, int(t)) != 5)
        g = rng.choice(sc.ACGT, self.GENOME_LEN).tobytes()
        gkeys, _ = windows(g, 0, self.GENOME_LEN - 1, K)
        gtargets = np.array([8, 6, 5, 36, 35, x], np.uint32)[rng.integers(0, 6, gkeys.size)]
        assert gkeys.size == self.GENOME_LEN - K + 1 == self.BIG[4][0]
        raw = bytes(bases)
        seqs = [raw[int(off[r]):int(off[r + 1])] for r in range(off.size - 1)]

        def stretch(h):
            p = int(rng.integers(0, gkeys.size - h + 1))
            return g[p:p + h + K - 1] if h else b""

        n_fragments = len(seqs) // 2
        for i, (h, h_mate) in reversed(list(enumerate(self.BIG))):  # from the back: an insertion moves what lies behind it
            pair = [stretch(h), stretch(h_mate)]
            at = 2 * ((2 * i + 1) * n_fragments // 12)
            seqs[at:at] = pair if i % 2 == 0 else pair[::-1]
        bases, off = concat_reads(seqs)
        self.build(parent, np.concatenate([keys, gkeys]), np.concatenate([targets, gtargets]), bases, off, votes=True)
        per = np.diff(self.plain.hits.offsets.astype(np.int64))
        self.big = np.flatnonzero(per > WAVE_HITS)
        assert sorted(per[self.big].tolist()) == sorted(h for h, _ in self.BIG)
        assert np.array_equal(per[self.big], np.diff(self.fastq.hits.offsets.astype(np.int64))[self.big])


@pytest.fixture(scope="module")
def pool():
    return Pool()


@pytest.fixture(scope="module")
def vote_pool():
    return VotePool()


def same_csr(what, got_off, got_nk, got_hits, exp):
    assert np.array_equal(got_off, exp.offsets), what
    assert np.array_equal(got_nk, exp.n_kmers), what
    got_hits = np.asarray(got_hits, np.uint32).reshape(-1, 3)
    for j, f in enumerate(("pos", "target", "entry")):
        assert np.array_equal(got_hits[:, j], getattr(exp, f)), "%s: %s" % (what, f)


class Mix:
    """the calls; each compares what it got and returns {family: (calls, units)}: what the timers must have seen of it"""

    def __init__(self, pool, db, sample, mirror):
        self.p, self.db, self.t, self.m = pool, db, sample, mirror

    # ---- a batch in its three forms
    def offsets(self, a, n):
        return self.p.bases, self.p.off[a:a + n + 1]  # (absolute: the calls rebase offsets that do not begin at 0)

    def block(self, ids):
        return fastq_block([self.p.seqs[r] for r in ids], [self.p.quals[r] for r in ids], eol=b"\r\n", blank_every=3)

    def device(self, a, n, cap):
        p = self.p
        b0, b1 = int(p.off[a]), int(p.off[a + n])
        return DeviceBatch(p.bases[b0:b1], p.off[a:a + n + 1] - p.off[a], cap)

    def device_hits(self, what, d, exp, cap):
        d.run(self.db, cap)
        assert int(d.down(d.d_tot, np.uint64, 1)[0]) == cap, what
        same_csr(what, d.down(d.d_ho, np.uint64, d.n + 1), d.down(d.d_nk, np.uint32, d.n), d.down(d.d_hits, np.uint32, cap * 3), exp)

    def tallied(self, what):
        t, m, n_entries = self.t, self.m, self.db.info.n_entries
        assert np.array_equal(t.gcount(), m.gcount), what
        bits = np.unpackbits(t.seen_export(0, t.seen_bytes()), bitorder="little").astype(bool)
        assert np.array_equal(bits[:n_entries], m.seen[:n_entries]) and not bits[n_entries:].any() and not m.seen[n_entries:].any(), what

    # ---- hits
    def hits_host(self, what, a, n, rule, seg, tally):
        exp = self.p.plain.sub(a, n)
        got = self.db.read_hits(*self.offsets(a, n))
        same_csr(what, got.offsets, got.n_kmers, np.stack([got.pos, got.target, got.entry], 1), exp)
        c = 1 + (int(exp.offsets[-1]) > 0)  # (the sizing call, and the call that fills)
        return {"hits": (c, c * n)}

    def hits_fastq(self, what, a, n, rule, seg, tally):
        exp = self.p.fastq.sub(a, n)
        got = self.db.read_hits_fastq(*self.block(range(a, a + n)))
        same_csr(what, got.offsets, got.n_kmers, np.stack([got.pos, got.target, got.entry], 1), exp)
        c = 1 + (int(exp.offsets[-1]) > 0)
        return {"hits": (c, c * n)}

    def hits_device(self, what, a, n, rule, seg, tally):
        exp = self.p.plain.sub(a, n)
        with self.device(a, n, int(exp.offsets[-1])) as d:
            self.device_hits(what, d, exp, int(exp.offsets[-1]))
        return {"hits": (1, n)}

    # ---- support
    def support_host(self, what, a, n, rule, seg, tally):
        got = self.db.read_support(*self.offsets(a, n), min_hits=rule[0], min_permille=rule[1], tally=self.t if tally else None)
        same_records(got, self.p.plain.rec[rule][a:a + n], SUPPORT_DTYPE, what)
        if tally:
            self.m.tally(np.arange(a, a + n), rule)
            self.tallied(what)
        return {"hits": (1, n), "support": (1, n)}

    def support_fastq(self, what, a, n, rule, seg, tally):
        text, recs = self.block(range(a, a + n))
        got = self.db.read_support_fastq(text, recs, min_hits=rule[0], min_permille=rule[1], tally=self.t if tally else None)
        exp = self.p.fastq.rec[rule][a:a + n]
        same_records(got, exp, SUPPORT_DTYPE, what)
        if tally:
            self.m.count(self.p.fastq.sub(a, n), exp, self.p.keep[a:a + n])
            self.tallied(what)
        return {"hits": (1, n), "support": (1, n)}

    def support_device(self, what, a, n, rule, seg, tally):
        exp = self.p.plain.sub(a, n)
        cap = int(exp.offsets[-1])
        with self.device(a, n, cap) as d:
            self.device_hits(what, d, exp, cap)
            d_out = d.dev(n * 24, np.full(n * 6, 0xA5A5A5A5, np.uint32))
            self.db.support_from_hits_device(d.d_ho.value, d.d_hits.value, d.d_nk.value, n, d_out.value, min_hits=rule[0], min_permille=rule[1])
            _lib.check(d.lib.kid_dev_sync(0))
            same_records(d.down(d_out, np.uint32, n * 6).view(SUPPORT_DTYPE), self.p.plain.rec[rule][a:a + n], SUPPORT_DTYPE, what)
        return {"hits": (1, n), "support": (1, n)}

    # ---- votes (a VotePool's facts)
    def votes_host(self, what, a, n, rule, seg, tally):
        got = self.db.read_votes(*self.offsets(a, n), min_hits=rule[0], min_permille=rule[1], tally=self.t if tally else None)
        exp = self.p.plain.votes[rule][a:a + n]
        same_records(got, exp, VOTE_DTYPE, what)
        if tally:
            self.m.count(self.p.plain.sub(a, n), exp, np.ones(n, bool))
            self.tallied(what)
        return {"hits": (1, n), "votes": (1, n)}

    def votes_fastq(self, what, a, n, rule, seg, tally):
        text, recs = self.block(range(a, a + n))
        got = self.db.read_votes_fastq(text, recs, min_hits=rule[0], min_permille=rule[1], tally=self.t if tally else None)
        exp = self.p.fastq.votes[rule][a:a + n]
        same_records(got, exp, VOTE_DTYPE, what)
        if tally:
            self.m.count(self.p.fastq.sub(a, n), exp, self.p.keep[a:a + n])
            self.tallied(what)
        return {"hits": (1, n), "votes": (1, n)}

    def votes_device(self, what, a, n, rule, seg, tally):
        exp = self.p.plain.sub(a, n)
        cap = int(exp.offsets[-1])
        with self.device(a, n, cap) as d:
            self.device_hits(what, d, exp, cap)
            d_out = d.dev(n * 32, np.full(n * 8, 0xA5A5A5A5, np.uint32))
            self.db.votes_from_hits_device(d.d_ho.value, d.d_hits.value, d.d_nk.value, n, d_out.value, min_hits=rule[0], min_permille=rule[1])
            _lib.check(d.lib.kid_dev_sync(0))
            same_records(d.down(d_out, np.uint32, n * 8).view(VOTE_DTYPE), self.p.plain.votes[rule][a:a + n], VOTE_DTYPE, what)
        return {"hits": (1, n), "votes": (1, n)}

    # ---- fragments (n: reads, even)
    def fragments_host(self, what, a, n, rule, seg, tally):
        hits = self.p.plain.sub(a, n)
        exp = self.p.fm.batch(hits, rule)
        got = self.db.read_fragments(*self.offsets(a, n), min_hits=rule[0], min_permille=rule[1], tally=self.t if tally else None)
        same_records(got, exp, FRAGMENT_DTYPE, what)
        if tally:
            self.m.count(fragment_csr(hits), exp, np.ones(n // 2, bool))
            self.tallied(what)
        return {"hits": (1, n), "fragments": (1, n // 2)}

    def fragments_fastq(self, what, a, n, rule, seg, tally):
        hits = self.p.fastq.sub(a, n)
        exp = self.p.fm.batch(hits, rule)
        (t1, r1), (t2, r2) = self.block(range(a, a + n, 2)), self.block(range(a + 1, a + n, 2))
        got = self.db.read_fragments_fastq(t1, r1, t2, r2, min_hits=rule[0], min_permille=rule[1], tally=self.t if tally else None)
        same_records(got, exp, FRAGMENT_DTYPE, what)
        if tally:
            keep = self.p.keep[a:a + n]
            self.m.count(fragment_csr(hits), exp, keep[0::2] | keep[1::2])  # counted when at least one mate is kept
            self.tallied(what)
        return {"hits": (1, n), "fragments": (1, n // 2)}

    def fragments_device(self, what, a, n, rule, seg, tally):
        hits = self.p.plain.sub(a, n)
        cap = int(hits.offsets[-1])
        with self.device(a, n, cap) as d:
            self.device_hits(what, d, hits, cap)
            d_out = d.dev(n * 16, np.full(n * 4, 0xA5A5A5A5, np.uint32))
            self.db.fragments_from_hits_device(d.d_ho.value, d.d_hits.value, d.d_nk.value, n, d_out.value, min_hits=rule[0], min_permille=rule[1])
            _lib.check(d.lib.kid_dev_sync(0))
            same_records(d.down(d_out, np.uint32, n * 4).view(FRAGMENT_DTYPE), self.p.fm.batch(hits, rule), FRAGMENT_DTYPE, what)
        return {"hits": (1, n), "fragments": (1, n // 2)}

    # ---- segments
    def same_segments(self, what, got, exp, n):
        assert got.offsets.dtype == np.uint64 and np.array_equal(got.offsets, exp[0]), what
        same_records(got.records, exp[1], SEGMENT_DTYPE, what)
        c = 1 + (exp[1].size > 0)
        return {"hits": (c, c * n), "segments": (c, c * n)}

    def segments_host(self, what, a, n, rule, seg, tally):
        bases, off = self.offsets(a, n)
        exp = SegmentModel(self.p.sm, bases, off).direct(seg[0], seg[1], rule)
        got = self.db.read_segments(bases, off, seg_len=seg[0], seg_step=seg[1], min_hits=rule[0], min_permille=rule[1])
        return self.same_segments(what, got, exp, n)

    def segments_fastq(self, what, a, n, rule, seg, tally):
        p = self.p
        bases, off = self.offsets(a, n)
        exp = SegmentModel(p.sm, bases, off, p.start[a:a + n], p.stop[a:a + n], p.keep[a:a + n]).direct(seg[0], seg[1], rule)
        got = self.db.read_segments_fastq(*self.block(range(a, a + n)), seg_len=seg[0], seg_step=seg[1], min_hits=rule[0], min_permille=rule[1])
        return self.same_segments(what, got, exp, n)

    def segments_device(self, what, a, n, rule, seg, tally):
        bases, off = self.offsets(a, n)
        exp = SegmentModel(self.p.sm, bases, off).direct(seg[0], seg[1], rule)
        hits = self.p.plain.sub(a, n)
        n_hits, n_seg = int(hits.offsets[-1]), int(exp[0][-1])
        with self.device(a, n, n_hits) as d:
            d_so, d_ns = d.dev((n + 1) * 8), d.dev(8)
            canary = np.full((n_seg + 2) * 8, 0xA5A5A5A5, np.uint32)
            d_seg = d.dev(canary.nbytes, canary)
            self.db.read_segments_device(d.d_bases.value, d.nbytes, d.d_off.value, n, seg[0], seg[1], d_so.value, d.d_tot.value, d_ns.value,
                                         min_hits=rule[0], min_permille=rule[1], d_hits=d.d_hits.value if n_hits else 0, hits_cap=n_hits,
                                         d_segments=d_seg.value if n_seg else 0, seg_cap=n_seg)
            _lib.check(d.lib.kid_dev_sync(0))
            assert (int(d.down(d.d_tot, np.uint64, 1)[0]), int(d.down(d_ns, np.uint64, 1)[0])) == (n_hits, n_seg), what
            assert np.array_equal(d.down(d_so, np.uint64, n + 1), exp[0]), what
            out = d.down(d_seg, np.uint32, canary.size)
            same_records(out[:n_seg * 8].view(SEGMENT_DTYPE), exp[1], SEGMENT_DTYPE, what)
            assert np.all(out[n_seg * 8:] == 0xA5A5A5A5), what
        return {"hits": (1, n), "segments": (1, n)}


def sequence(rng):
    """-> [(family, form)]: a segments call in front of and behind every call of another family"""
    others = [(fam, form) for fam in FAMILIES if fam != "segments" for form in FORMS]
    drawn = [others[i] for i in rng.permutation(9)] + [others[i] for i in rng.permutation(9)] + [others[i] for i in rng.integers(0, 9, 2)]
    segs = [("segments", FORMS[i]) for i in rng.permutation(np.repeat(np.arange(3), 7))]
    calls = []
    for s, o in zip(segs, drawn):
        calls += [s, o]
    return calls + [segs[-1]]


def test_mixed_calls_share_one_state(pool):
    rng = np.random.default_rng(SEED)
    calls = sequence(rng)
    assert len(calls) == 41 and {c for c in calls} == {(fam, form) for fam in FAMILIES for form in FORMS}
    assert all(calls[i][0] == "segments" for i in range(0, 41, 2)) and all(calls[i][0] != "segments" for i in range(1, 41, 2))
    db = pool.db()
    assert db.info.n_entries <= pool.keys.size <= N_ENTRIES
    t = db.sample()
    mix = Mix(pool, db, t, Mirror(pool.mirror_world()))
    queries = {"hits": db.read_hits_time, "support": db.read_support_time, "segments": db.read_segments_time, "fragments": db.read_fragments_time}
    tallies, seen_before = 0, {}
    for i, (fam, form) in enumerate(calls):
        n = SIZES[i % len(SIZES)]
        if fam == "fragments":
            n += n & 1
        a = 2 * int(rng.integers(0, (pool.n - n) // 2 + 1))  # (even: a batch of fragments begins with a mate 1)
        rule, seg = RULES[int(rng.integers(0, 2))], SEGS[int(rng.integers(0, 2))]
        seen_before[fam, form] = seen_before.get((fam, form), -1) + 1
        tally = fam in ("support", "fragments") and form != "device" and seen_before[fam, form] % 2 == 0  # every other call of the four
        tallies += tally
        what = "call %d: %s %s, reads [%d, %d), rule %s, segments %s, tally %s" % (i, fam, form, a, a + n, rule, seg, tally)
        made = getattr(mix, "%s_%s" % (fam, form))(what, a, n, rule, seg, tally)
        for name, query in queries.items():
            ms, c, units = query()
            assert (c, units) == made.get(name, (0, 0)), "%s: the %s timer" % (what, name)
            assert (ms > 0) == (c > 0), "%s: the %s timer" % (what, name)
    assert tallies >= 4
    g, u = t.end()
    assert np.array_equal(g, mix.m.gcount) and np.array_equal(u, mix.m.ucount()) and int(g.sum()) > 0
    t.close()
    db.close()


# ------------------------------------------------------------------ the fifth family
FIVE = ("hits", "support", "segments", "fragments", "votes")
TALLYING = ("support", "fragments", "votes")


def vote_sequence(rng):
    """-> [(family, form)] of 56 calls.  The first 49: the twelve (family, form) of the four families that are not
    segments, twice, each time in another order, a segments call in front of and behind every one of them.  The last 7: a
    vote call directly in front of and directly behind a hits, a support and a fragments call (what stands directly beside a
    segments call the first 49 have shown for every family)."""
    others = [(fam, form) for fam in FIVE if fam != "segments" for form in FORMS]
    drawn = [others[i] for i in rng.permutation(12)] + [others[i] for i in rng.permutation(12)]
    segs = [("segments", FORMS[i]) for i in rng.permutation(np.repeat(np.arange(3), 9))]
    calls = []
    for s, o in zip(segs, drawn):
        calls += [s, o]
    calls.append(segs[-1])
    votes = [("votes", FORMS[i]) for i in rng.permutation(3)] + [("votes", "host")]
    beside = [(fam, FORMS[int(rng.integers(0, 3))]) for fam in ("hits", "support", "fragments")]
    for v, o in zip(votes, beside):
        calls += [v, o]
    return calls + [votes[-1]]


def vote_plan(pool_n, rng):
    """the calls with their batches -> [(family, form, first read, reads, rule, segment geometry, tally)]: SIZES go up and
    down as in the test above; every other host and FASTQ call of the three families that can tallies"""
    plan, seen_before = [], {}
    for i, (fam, form) in enumerate(vote_sequence(rng)):
        n = SIZES[i % len(SIZES)]
        if fam == "fragments":
            n += n & 1
        a = 2 * int(rng.integers(0, (pool_n - n) // 2 + 1))
        rule, seg = RULES[int(rng.integers(0, 2))], SEGS[int(rng.integers(0, 2))]
        seen_before[fam, form] = seen_before.get((fam, form), -1) + 1
        tally = fam in TALLYING and form != "device" and seen_before[fam, form] % 2 == 0
        plan.append((fam, form, a, n, rule, seg, tally))
    return plan


def test_mixed_calls_with_votes_share_one_state(vote_pool):
    pool = vote_pool
    plan = vote_plan(pool.n, np.random.default_rng(VOTE_SEED))
    calls = [(fam, form) for fam, form, *_ in plan]
    assert len(calls) == 56 and all(calls.count((fam, form)) >= 2 for fam in FIVE for form in FORMS)
    assert all(calls[i][0] == "segments" for i in range(0, 49, 2)) and all(calls[i][0] != "segments" for i in range(1, 49, 2))
    for fam in FIVE:
        if fam != "votes":
            assert any(calls[i][0] == "votes" and calls[i + 1][0] == fam for i in range(55)), fam
            assert any(calls[i][0] == fam and calls[i + 1][0] == "votes" for i in range(55)), fam
    # the second vote kernel has reads in at least two calls that tally, and in a call of each form
    with_big = [(form, tally) for fam, form, a, n, _, _, tally in plan if fam == "votes" and ((pool.big >= a) & (pool.big < a + n)).any()]
    assert sum(tally for _, tally in with_big) >= 2 and {form for form, _ in with_big} == set(FORMS)
    db = pool.db()
    assert db.info.n_entries <= pool.keys.size <= N_ENTRIES // 4
    t = db.sample()
    mix = Mix(pool, db, t, Mirror(pool.mirror_world()))
    queries = {"hits": db.read_hits_time, "support": db.read_support_time, "segments": db.read_segments_time,
               "fragments": db.read_fragments_time, "votes": db.read_votes_time}
    for i, (fam, form, a, n, rule, seg, tally) in enumerate(plan):
        what = "call %d: %s %s, reads [%d, %d), rule %s, segments %s, tally %s" % (i, fam, form, a, a + n, rule, seg, tally)
        made = getattr(mix, "%s_%s" % (fam, form))(what, a, n, rule, seg, tally)
        for name, query in queries.items():
            ms, c, units = query()
            assert (c, units) == made.get(name, (0, 0)), "%s: the %s timer" % (what, name)
            assert (ms > 0) == (c > 0), "%s: the %s timer" % (what, name)
    assert sum(tally for *_, tally in plan) >= 6
    g, u = t.end()
    assert np.array_equal(g, mix.m.gcount) and np.array_equal(u, mix.m.ucount()) and int(g.sum()) > 0
    t.close()
    db.close()


def test_vote_families_alternate_on_one_scratch():
    parent, spine, sibs = sc.chain_taxonomy(12)  # 26 nodes
    g, keys, tg = genome_world(np.random.default_rng(513), spine + sibs, 1300, 1)
    big, small = WAVE_HITS + 1, LANE_HITS  # hits of a stretch of the genome: its windows
    cut = lambda p, h: g[p:p + h + K - 1]  # noqa: E731

    def batches(p):
        """-> {family: (the call's arguments, the hits its two units must have)}, from the genome at p on"""
        reads = concat_reads([cut(p, big), cut(p + 600, small)])
        mates = concat_reads([cut(p, 300), cut(p + 300, big - 300), cut(p + 600, small // 2), cut(p + 650, small - small // 2)])
        return {"votes": (reads, {}), "fragment_votes": (mates, {}), "segment_votes": (reads, {"seg_len": big})}

    def call(db, family, args):
        (bases, off), kw = args
        got = getattr(db, "read_" + family)(bases, off, min_hits=2, min_permille=25, **kw)
        return (got.offsets, got.records) if family == "segment_votes" else (None, got)

    dtypes = {"votes": VOTE_DTYPE, "fragment_votes": FRAGMENT_VOTE_DTYPE, "segment_votes": SEGMENT_VOTE_DTYPE}
    plan = [(family, args) for p in (0, 40) for family, args in batches(p).items()]
    exp = []
    for family, args in plan:  # each call on a database of its own
        fresh = KmerDB(keys, tg, parent, k=K, log2_slots=12)
        exp.append(call(fresh, family, args))
        fresh.close()
        assert exp[-1][1]["n_hits"].tolist() == [big, small], family  # one unit for the second kernel, one for a lane
    db = KmerDB(keys, tg, parent, k=K, log2_slots=12)
    for i, (family, args) in enumerate(plan):
        off, rec = call(db, family, args)
        assert off is None or np.array_equal(off, exp[i][0]), (i, family)
        same_records(rec, exp[i][1], dtypes[family], "call %d: %s" % (i, family))
    db.close()
