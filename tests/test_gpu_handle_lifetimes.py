"""The handles of the host library and the memory behind them: what a database, its samples and its hit scratch took
from the device comes back when they are destroyed; their grow-only buffers follow batches that grow and shrink; and
a call refused by the host-side checks leaves its handle as it was.  Answers are compared with the oracle's (exact)."""
import ctypes as C

import numpy as np
import pytest

from helpers import K, concat_reads, fastq_block, ob, oracle_db, small_db, synth
from kmer_id_amd import KidError, KmerDB, PinnedBuffer, _lib
from kmer_id_amd.api import ReadHits
from kmer_id_amd.builder import device_mem_info
from read_hits_model import HitModel, trim_ranges
from read_support_model import SupportModel

pytestmark = pytest.mark.gpu

LOG2_SLOTS = 16
N, L = 9000, 150       # the largest batch; the others are its first 64, 2 000 and 5 000 reads
KID_ERR_ARG = -1


class World:
    """One database's entries, N reads, and what the oracle says about every read (a read's answers do not depend on
    the batch it comes in, so every batch of the tests is a prefix of these)."""

    def __init__(self):
        self.parent, self.cum, self.keys, self.targets = small_db(1e-4)
        self.odb = oracle_db(self.parent, self.keys, self.targets, LOG2_SLOTS)
        self.bases = synth.reads(self.cum, self.parent, N, L, K, r0=31337).reshape(N, L)
        self.quals = synth.qualities(N, L, r0=31337)
        self.flat = self.bases.reshape(-1)
        self.off = synth.fixed_offsets(N, L)
        self.start, self.stop, self.keep = trim_ranges([q.tobytes() for q in self.quals], [L] * N, K)
        assert 0 < int((~self.keep).sum()) < N // 4
        os_ = ob.OracleSample(self.odb)
        self.final = os_.classify(self.flat, self.off)                       # whole reads
        os_.close()
        kept = np.flatnonzero(self.keep)
        os_ = ob.OracleSample(self.odb)
        self.final_fq = np.zeros(N, np.uint32)                               # trimmed reads; 0 where process_qual drops one
        self.final_fq[kept] = os_.classify(self.bases[kept].reshape(-1), synth.fixed_offsets(kept.size, L),
                                           self.start[kept], self.stop[kept])
        os_.close()
        model = HitModel(self.odb, self.keys, self.targets, K)
        self.hits = model.batch(self.flat, self.off)
        no_range = (np.where(self.keep, self.start, 1).astype(np.int32), np.where(self.keep, self.stop, 0).astype(np.int32))
        self.hits_fq = model.batch(self.flat, self.off, *no_range)
        assert int(self.hits.offsets[64]) > 0 and int(self.hits_fq.offsets[64]) > 0
        self.blocks = {}

    def new_db(self):
        return KmerDB(self.keys, self.targets, self.parent, k=K, log2_slots=LOG2_SLOTS)

    def block(self, n):
        if n not in self.blocks:
            self.blocks[n] = fastq_block([b.tobytes() for b in self.bases[:n]], [q.tobytes() for q in self.quals[:n]])
        return self.blocks[n]

    def counts(self, whole, trimmed):
        """the oracle's (gcount, ucount) of a sample that got the first n reads whole for every n of `whole`, and
        trimmed as a FASTQ block for every n of `trimmed`"""
        os_ = ob.OracleSample(self.odb)
        for n in whole:
            os_.classify(self.flat[:n * L], self.off[:n + 1])
        for n in trimmed:
            kept = np.flatnonzero(self.keep[:n])
            os_.classify(self.bases[kept].reshape(-1), synth.fixed_offsets(kept.size, L), self.start[kept], self.stop[kept])
        g, u = os_.counts()
        os_.close()
        return g, u


@pytest.fixture(scope="module")
def world():
    return World()


def same_prefix(got, exp, n, what):
    """a ReadHits of the first n reads against the first n reads of the model's"""
    h = int(exp.offsets[n])
    assert np.array_equal(got.offsets, exp.offsets[:n + 1]), what
    assert np.array_equal(got.n_kmers, exp.n_kmers[:n]), what
    assert np.array_equal(got.pos, exp.pos[:h]) and np.array_equal(got.target, exp.target[:h]), what
    assert np.array_equal(got.entry, exp.entry[:h]), what


def test_buffers_follow_batches_that_grow_and_shrink(world):
    """64, 5 000, 64, 9 000 reads through one sample and one database: every ensure() site ordinary reads reach --
    descriptors, slot text, slot per-read arrays, slot records, the hits scratch -- grows twice and is reused twice."""
    w = world
    sizes = (64, 5000, 64, 9000)
    db = w.new_db()
    s = db.sample()
    outs = [np.empty(n, np.uint32) for n in sizes]
    for pair in ((0, 1), (2, 3)):   # two batches in flight, the later ticket waited for first
        tickets = [s.classify_async(w.flat[:sizes[i] * L], w.off[:sizes[i] + 1], out=outs[i]) for i in pair]
        s.wait(tickets[1])
        s.wait(tickets[0])
    for n, out in zip(sizes, outs):
        assert np.array_equal(out, w.final[:n]), "classify_batch_async, %d reads" % n
    for n in sizes:
        text, recs = w.block(n)
        fin, start, stop = s.classify_fastq(text, recs)
        keep = w.keep[:n]
        assert np.array_equal(stop - start >= K, keep), "classify_fastq_async, %d reads" % n
        assert np.array_equal(start[keep], w.start[:n][keep]) and np.array_equal(stop[keep], w.stop[:n][keep])
        assert np.array_equal(fin, w.final_fq[:n]), "classify_fastq_async, %d reads" % n
    for n in sizes:
        same_prefix(db.read_hits(w.flat[:n * L], w.off[:n + 1]), w.hits, n, "read_hits, %d reads" % n)
        same_prefix(db.read_hits_fastq(*w.block(n)), w.hits_fq, n, "read_hits_fastq, %d reads" % n)
    g, u = s.end()
    eg, eu = w.counts(sizes, sizes)
    assert np.array_equal(g, eg) and np.array_equal(u, eu)
    s.close(); db.close()


class Mixed:
    """n reads of the world from read `first` on, three of them cut short: fewer than k bases (no window, no tile),
    exactly 64 windows (one tile) and 65 windows (two tiles); as an offsets batch and as a FASTQ block, each with the
    model's hits.  The cut reads get a flawless quality line, so that process_qual leaves them their windows."""

    def __init__(self, w, model, first, n, cut):
        seqs = [w.bases[first + i].tobytes() for i in range(n)]
        quals = [w.quals[first + i].tobytes() for i in range(n)]
        for i, length in cut.items():
            seqs[i], quals[i] = seqs[i][:length], b"I" * length
        self.n = n
        self.flat, self.off = concat_reads(seqs)
        self.text, self.recs = fastq_block(seqs, quals)
        self.hits = model.batch(self.flat, self.off)
        start, stop, self.keep = trim_ranges(quals, [len(s) for s in seqs], K)
        start[~self.keep], stop[~self.keep] = 1, 0   # no range: no window, no hit
        self.hits_fq = model.batch(self.flat, self.off, start, stop)
        for h in (self.hits, self.hits_fq):
            assert sorted(int(h.n_kmers[i]) for i in cut) == [0, 64, 65][3 - len(cut):]


def hits_in_one_call(call, n):
    """kid_db_read_hits* once, into a buffer with room for a hit at every window of n reads of L bases -> ReadHits"""
    cap = n * (L - K + 1)
    offsets, n_kmers, hits, total = np.empty(n + 1, np.uint64), np.empty(n, np.uint32), np.empty(cap * 3, np.uint32), C.c_uint64(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    _lib.check(call(n, p(offsets), p(n_kmers), p(hits), cap, C.byref(total)))
    return ReadHits(offsets, n_kmers, hits[:total.value * 3])


def same_support(got, exp, what):
    for f in exp.dtype.names:
        assert np.array_equal(got[f], exp[f]), "%s: %s" % (what, f)


def test_hits_and_support_calls_interleave_on_one_database(world):
    """read_hits, read_support, read_hits_fastq, read_support_fastq with a tally, read_hits on one handle, 1025, 7, 1,
    1025 and 7 reads: the calls share the database's grow-only scratch (1025 reads cross the 1024-element scan block)
    and its two timers.  Every hits step is one library call, so that the hit-pass timer counts one call per step."""
    w = world
    lib = _lib.load()
    model = HitModel(w.odb, w.keys, w.targets, K)
    support = SupportModel(model, w.parent)
    big = Mixed(w, model, 0, 1025, {3: K - 10, 500: 64 + K - 1, 1024: 65 + K - 1})
    small = Mixed(w, model, 1126, 7, {1: K - 1, 3: 64 + K - 1, 6: 65 + K - 1})
    one = Mixed(w, model, 3, 1, {0: 65 + K - 1})
    assert int(small.hits.offsets[-1]) >= 8 and int(one.hits_fq.offsets[-1]) >= 2
    assert int(big.hits.offsets[-1]) > 100 and int(big.hits_fq.offsets[-1]) > 100 and 0 < int((~big.keep).sum()) < 1025 // 4
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    db = w.new_db()
    t = db.sample()

    def read_hits(b):
        return hits_in_one_call(lambda n, *out: lib.kid_db_read_hits(db._h, p(b.flat), p(b.off), None, None, n, *out), b.n)

    same_prefix(read_hits(big), big.hits, big.n, "1. read_hits, 1025 reads")
    rule = (2, 25)
    exp = support.batch_identity(small.hits, rule, support.finals(small.hits))
    same_support(db.read_support(small.flat, small.off, min_hits=rule[0], min_permille=rule[1]), exp, "2. read_support, 7 reads")
    got = hits_in_one_call(lambda n, *out: lib.kid_db_read_hits_fastq(db._h, p(one.text), one.text.size, p(one.recs), n, *out), one.n)
    same_prefix(got, one.hits_fq, one.n, "3. read_hits_fastq, 1 read")
    rule = (1, 10)
    exp = support.batch_identity(big.hits_fq, rule, support.finals(big.hits_fq))
    same_support(db.read_support_fastq(big.text, big.recs, min_hits=rule[0], min_permille=rule[1], tally=t), exp,
                 "4. read_support_fastq, 1025 reads")
    same_prefix(read_hits(small), small.hits, small.n, "5. read_hits, 7 reads")
    g, u = t.end()
    eg, eu = support.tally(big.hits_fq, exp, big.keep, w.targets)   # a record process_qual drops is counted nowhere
    assert np.array_equal(g, eg) and np.array_equal(u, eu) and int(g.sum()) == int(big.keep.sum()) and int(u.sum()) > 0
    ms, calls, reads = db.read_hits_time()   # a read_support call runs the hit pass too
    assert (calls, reads) == (5, 1025 + 7 + 1 + 1025 + 7) and ms > 0
    ms, calls, reads = db.read_support_time()
    assert (calls, reads) == (2, 7 + 1025) and ms > 0
    assert db.read_hits_time() == (0.0, 0, 0) and db.read_support_time() == (0.0, 0, 0)
    t.close(); db.close()


def refused(call, fragment):
    with pytest.raises(KidError) as e:
        call()
    assert e.value.status == KID_ERR_ARG and fragment in str(e.value), str(e.value)


def test_a_refused_call_leaves_the_handle_usable(world):
    """Every refusal here is the host's, before anything is queued: status, message, and then business as usual."""
    w = world
    n = 2000
    flat, off = w.flat[:n * L], w.off[:n + 1].copy()
    text, recs = w.block(n)
    db = w.new_db()
    s = db.sample()
    lib = _lib.load()
    whole, trimmed = [], []

    def valid_batches():
        assert np.array_equal(s.classify(flat, off), w.final[:n])
        assert np.array_equal(s.classify_fastq(text, recs)[0], w.final_fq[:n])
        same_prefix(db.read_hits(flat, off), w.hits, n, "read_hits")
        same_prefix(db.read_hits_fastq(text, recs), w.hits_fq, n, "read_hits_fastq")
        whole.append(n); trimmed.append(n)

    valid_batches()   # (the buffers exist from here on)
    # offsets that go backwards
    bad_off = off.copy()
    bad_off[7] = bad_off[6] - np.uint64(1)
    refused(lambda: s.classify(flat, bad_off), "offsets not monotone at read 6")
    refused(lambda: db.read_hits(flat, bad_off), "offsets not monotone at read 6")
    valid_batches()
    # [start, stop] outside a read
    start, stop = np.zeros(n, np.int32), np.full(n, L - 1, np.int32)
    stop[11] = L
    refused(lambda: s.classify(flat, off, start, stop), "read 11: [start,stop] = [0,150] outside the read of length 150")
    refused(lambda: db.read_hits(flat, off, start, stop), "read 11: [start,stop] = [0,150] outside the read of length 150")
    valid_batches()
    # a FASTQ record beyond its block
    bad_recs = recs.copy()
    bad_recs[5, 2] = text.size - 10
    refused(lambda: s.classify_fastq(text, bad_recs), "record 5 lies outside the text block")
    refused(lambda: db.read_hits_fastq(text, bad_recs), "record 5 lies outside the text block")
    valid_batches()
    # room for hits announced, no buffer for them
    ho, total = np.empty(n + 1, np.uint64), C.c_uint64(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    refused(lambda: _lib.check(lib.kid_db_read_hits(db._h, p(flat), p(off), None, None, n, p(ho), None, None, 5, C.byref(total))),
            "cap without a hits buffer")
    refused(lambda: _lib.check(lib.kid_db_read_hits_fastq(db._h, p(text), text.size, p(recs), n, p(ho), None, None, 5, C.byref(total))),
            "cap without a hits buffer")
    valid_batches()
    g, u = s.end()
    eg, eu = w.counts(whole, trimmed)
    assert len(whole) == 5 and int(g.sum()) == 5 * (n + int(w.keep[:n].sum()))
    assert np.array_equal(g, eg) and np.array_equal(u, eu)
    s.close(); db.close()


def test_handles_give_back_what_they_took(world):
    """Free device memory after the 20th build-use-destroy round equals free memory after the first (the runtime keeps
    pools of its own after first use, so the state before the first round is no yardstick).  hipMemGetInfo is the
    runtime's number: what it moves by across 20 readings with nothing in between is allowed on top, and printed.

    Two rounds that are not counted come first.  Measured on an MI355X: in a process that has launched no kernel yet,
    free memory falls by 199 229 440 bytes in its first round and by another 16 777 216 in its second, then stays where
    it is to the byte for rounds 3 to 40 (idle wobble 0).  The library with hand-written free lists that this one
    replaced gives the same three figures, and rounds that build and destroy handles without classifying show no second
    step: both steps are the runtime's, taken at its first two batches of launches in a process, not memory a handle
    kept.  With them behind it the test reads the same whether it runs alone or after others."""
    w = world
    n = 2000
    text, recs = w.block(n)
    pinned = PinnedBuffer(n * L)
    pinned.array[:] = w.flat[:n * L]

    def one_round():
        db = w.new_db()
        a, b = db.sample(), db.sample()
        out = np.empty(n, np.uint32)
        a.wait(a.classify_async(w.flat[:n * L], w.off[:n + 1], out=out))   # offsets
        b.wait(b.classify_fixed_async(pinned.ptr, L, n))                    # fixed layout
        fin = b.classify_fastq(text, recs)[0]                               # FASTQ block
        hits = db.read_hits(w.flat[:n * L], w.off[:n + 1])
        a.close(); b.close(); db.close()
        return out, fin, hits

    for _ in range(2):   # the runtime's own two steps (see above)
        one_round()
    idle = [device_mem_info()[0] for _ in range(20)]
    wobble = max(idle) - min(idle)
    free = []
    for r in range(20):
        out, fin, hits = one_round()
        free.append(device_mem_info()[0])
        if r == 0:
            assert np.array_equal(out, w.final[:n]) and np.array_equal(fin, w.final_fq[:n])
            same_prefix(hits, w.hits, n, "read_hits")
    pinned.close()
    print("free bytes after rounds 1, 2, 20: %d, %d, %d; idle wobble %d" % (free[0], free[1], free[19], wobble))
    assert abs(free[19] - free[1]) <= wobble
    assert abs(free[19] - free[0]) <= wobble
