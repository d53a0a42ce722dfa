"""A kid_sample held to the mirror of tests/sample_life.py across long mixed call sequences: the regimes of the hit log, the
bitmap's pieces and the long-record list that depend on a sample's history, not on one batch.

  T1  a pass over the hit log started by the pace (in front of the 257th launch), with launches queued behind it
  T2  the log switched off by the device in stream order, launches queued behind it; reset switches it on
  T3  bits at the edges of the apply pass's pieces and of the bitmap, launches of 1 .. 520 reads
  T4  more long records in a batch than the long-record list holds (KID_LONG_MAX = 1024)
  T5  a seeded life of 400 mixed steps, kid_sample_end, kid_sample_reset and a second life on the same handle

T1 and T2 prove the regime they reached with Sample.log_state() (kid_sample_log_state); every comparison is of exact
integers against SampleMirror, whose facts come from the oracle and the suite's models.  Every index handed to the library
is in range: the argument errors have their own tests."""
import numpy as np
import pytest

import kmer_id_amd
import sample_life as sl
from kmer_id_amd import KID_FLAG_REF_GEOMETRY, KID_OPT_ENTRY_DEPTH, KID_OPT_INPUTS_READY, KID_OPT_MIN_BASE_QUALITY, KmerDB
from kmer_id_amd._lib import KID_OPT_LONG_RECORD_KMERS

pytestmark = pytest.mark.gpu

K, L, PIECE = sl.K, sl.L, sl.PIECE


@pytest.fixture(scope="module")
def w():
    return sl.world()


@pytest.fixture(scope="module")
def dbs(w):
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = KmerDB(w.keys, w.targets, w.parent, k=K, log2_slots=sl.LOG2_SLOTS,
                                flags=KID_FLAG_REF_GEOMETRY if kind == "ref_geometry" else 0)
            assert made[kind].info.n_entries == sl.N_ENTRIES and made[kind].info.geometry == (0 if kind == "ref_geometry" else 1)
        return made[kind]
    yield get
    for db in made.values():
        db.close()


class DevicePool:
    """the pool resident in HBM: text (padded), offsets and the [start, stop] of every read"""

    def __init__(self, w):
        import torch
        self.torch = torch
        pad = np.zeros(w.bases.size + 64, np.uint8)
        pad[:w.bases.size] = w.bases
        self.bases = torch.from_numpy(pad).cuda()
        self.off = torch.from_numpy(w.off.view(np.int64)).cuda()
        self.start, self.stop = torch.from_numpy(w.start).cuda(), torch.from_numpy(w.stop).cuda()
        self.nbytes = int(w.bases.size)
        torch.cuda.synchronize()

    def out(self, n):
        """a result array of n reads, filled with -1 before anybody launches into it"""
        t = self.torch.full((max(n, 1),), -1, dtype=self.torch.int32, device="cuda")
        self.torch.cuda.current_stream().synchronize()
        return t


@pytest.fixture(scope="module")
def pool(w):
    return DevicePool(w)


class Rig:
    """one kid_sample and its mirror, driven by the same calls"""

    def __init__(self, w, db, pool, tag, depth=False):
        self.w, self.db, self.pool, self.tag = w, db, pool, tag
        self.s = db.sample()
        if depth:
            self.s.set_option(KID_OPT_ENTRY_DEPTH, 1)
        self.depth = depth
        self.m = sl.SampleMirror(w)
        self.step = 0
        self.tickets = []   # [ticket, keep-alive, out, expected]
        self.pending = []   # (device tensor, expected): compared once the device is idle
        assert self.s.seen_bytes() == w.seen_bytes

    def at(self, what=""):
        return "%s, step %d%s" % (self.tag, self.step, what and ": " + what)

    # ---- the calls
    def host(self, ids, ranges=False):
        b, o, st, sp = sl.batch_of(self.w, ids, ranges)
        got, exp = self.s.classify(b, o, st, sp), self.m.classify(ids)
        assert np.array_equal(got, exp), self.at("classify")

    def host_async(self, ids, ranges=False):
        b, o, st, sp = sl.batch_of(self.w, ids, ranges)
        out = np.full(len(ids), 0xFFFFFFFF, np.uint32)
        t = self.s.classify_async(b, o, st, sp, out=out)
        self.tickets.append([t, (b, o, st, sp), out, self.m.classify(ids)])

    def fixed_async(self, first, n, want_out=True):
        assert first + n <= self.w.n_fixed
        out = np.full(n, 0xFFFFFFFF, np.uint32) if want_out else None
        t = self.s.classify_fixed_async(self.w.bases.ctypes.data + first * L, L, n, out.ctypes.data if want_out else 0)
        self.tickets.append([t, None, out, self.m.classify(np.arange(first, first + n))])

    def fixed_device(self, first, n, d_out=None, stream=0):
        assert first % 8 == 0 and first + n <= self.w.n_fixed  # (16-byte aligned text)
        self.s.classify_fixed_device(self.pool.bases.data_ptr() + first * L, L, n, d_out=d_out.data_ptr() if d_out is not None else 0,
                                     stream=stream)
        exp = self.m.classify(np.arange(first, first + n))
        if d_out is not None:
            self.pending.append((d_out[:n], exp))

    def device(self, first, n, d_out=None, ranges=False, stream=0):
        assert first + n <= self.w.n_pool
        p = self.pool
        self.s.classify_device(p.bases.data_ptr(), p.nbytes, p.off.data_ptr() + 8 * first, n,
                               d_start=p.start.data_ptr() + 4 * first if ranges else 0, d_stop=p.stop.data_ptr() + 4 * first if ranges else 0,
                               d_out=d_out.data_ptr() if d_out is not None else 0, stream=stream)
        exp = self.m.classify(np.arange(first, first + n))
        if d_out is not None:
            self.pending.append((d_out[:n], exp))

    def fastq(self, block, q):
        b = self.w.blocks[block]
        self.s.set_option(KID_OPT_MIN_BASE_QUALITY, q)
        got, exp = self.s.classify_fastq(b["text"], b["recs"]), self.m.classify_fastq(block, q)
        for g, e, name in zip(got, exp, ("final", "start", "stop")):
            assert np.array_equal(g, e), self.at("classify_fastq block %d Q %d: %s" % (block, q, name))

    def tally(self, ids, rule, ranges=False):
        b, o, st, sp = sl.batch_of(self.w, ids, ranges)
        got = self.db.read_support(b, o, st, sp, min_hits=rule[0], min_permille=rule[1], tally=self.s)
        exp = self.m.tally(ids, rule)
        for name in exp.dtype.names:
            assert np.array_equal(got[name], exp[name]), self.at("read_support %s: %s" % (rule, name))

    def seen_or(self, bits):
        a = np.zeros(self.w.seen_bytes, np.uint8)
        bits = np.asarray(bits, np.int64)
        np.bitwise_or.at(a, bits >> 3, (1 << (bits & 7)).astype(np.uint8))
        self.s.seen_or(0, a)
        self.m.seen_or(bits)

    def reset(self):
        self.settle()
        self.s.reset()
        self.m.reset()

    # ---- the comparisons
    def wait(self, i, again=False):
        t, _, out, exp = self.tickets[i]
        self.s.wait(t)
        if again:
            self.s.wait(t)
        if out is not None:
            assert np.array_equal(out, exp), self.at("results of ticket %d" % t)
        del self.tickets[i]

    def settle(self, rng=None):
        """every ticket waited for (in random order), the device idle, every result on the device compared"""
        while self.tickets:
            self.wait(int(rng.integers(0, len(self.tickets))) if rng is not None else len(self.tickets) - 1)
        self.pool.torch.cuda.synchronize()
        for d_out, exp in self.pending:
            assert np.array_equal(d_out.cpu().numpy().view(np.uint32), exp), self.at("results on the device")
        self.pending = []

    def sub_ranges(self):
        bits = self.w.seen_bytes * 8
        return [(0, 128), (PIECE - 128, PIECE + 128), (bits - 128, bits)]

    def check_gcount(self):
        assert np.array_equal(self.s.gcount(), self.m.gcount), self.at("gcount")

    def check_ucount(self, ranges):
        for a, b in ranges:
            assert np.array_equal(self.s.ucount_range(a, b), self.m.ucount(a, b)), self.at("ucount_range(%d, %d)" % (a, b))

    def check_export(self):
        got, exp = self.s.seen_export(0, self.w.seen_bytes), self.m.bitmap_bytes()
        diff = np.flatnonzero(got != exp)
        assert diff.size == 0, self.at("seen_export: %d bytes differ, the first at byte %d (%#x, expected %#x)" % (
            diff.size, diff[0], got[diff[0]], exp[diff[0]]))

    def check_depth(self):
        if self.depth:
            assert np.array_equal(self.s.entry_depth(), self.m.depth), self.at("entry_depth")

    def check_all(self, what, rng=None):
        self.settle(rng)
        self.check_gcount()  # (does not flush the log)
        self.check_ucount([(0, self.w.seen_bytes * 8)] + self.sub_ranges())
        self.check_export()
        st, exp = self.s.stats(), self.m.stats()
        assert {k: st[k] for k in exp} == exp, self.at("%s: stats" % what)
        assert self.s.masked_bases() == self.m.masked, self.at("%s: masked_bases" % what)
        self.check_depth()

    def close(self):
        self.s.close()


def slices_of(ids, n=64):
    return [int(ids[i]) for i in range(0, len(ids) - n + 1, n)]


def sparse_slices(w):
    """the first reads of the 65 slices of 64 reads of A and C"""
    return slices_of(w.A) + slices_of(w.C)


# ------------------------------------------------------------------ T1
@pytest.mark.parametrize("entry", ["fixed_device", "host_async"])
def test_a_pass_started_by_the_pace_loses_no_bit(w, dbs, pool, entry):
    """300 launches of 64 sparse reads without a counter read or a synchronising call: kid_seenlog_pace queues the pass over
    the log in front of the 257th, and the launches behind it go on logging into the regions the pass has emptied"""
    import torch
    rig = Rig(w, dbs("minloc"), pool, "pace/%s, seed %d" % (entry, w.seed))
    firsts = sparse_slices(w)
    stream = torch.cuda.Stream()

    def launches(i0, n):
        d_out = pool.out(n * 64) if entry == "fixed_device" else None
        for i in range(i0, i0 + n):
            rig.step = i
            first = firsts[i % len(firsts)]
            if entry == "fixed_device":
                rig.fixed_device(first, 64, d_out[(i - i0) * 64:], stream=stream.cuda_stream)
            else:
                rig.host_async(np.arange(first, first + 64))

    launches(0, 300)
    st = rig.s.log_state()
    print("T1 %s after 300 launches: %s" % (entry, st))
    assert st["has_log"] and st["passes"] >= 1 and st["logging"], rig.at("the pace has not started a pass: %s" % st)
    rng = np.random.default_rng(1)
    if rig.tickets:  # late, out of order, one of them twice
        rig.wait(len(rig.tickets) // 2, again=True)
    rig.check_all("after 300 launches", rng)
    launches(300, 10)
    rig.settle(rng)
    g, u = rig.s.end()
    assert np.array_equal(g, rig.m.gcount) and np.array_equal(u, rig.m.ucount()), rig.at("end")
    rig.check_all("after end")
    rig.close()


# ------------------------------------------------------------------ T2
def test_dense_reads_switch_the_log_off_between_queued_launches(w, dbs, pool):
    """300 unsynchronised launches of 64 dense reads: the pass in front of the 257th finds more than 8 places per read and
    takes the log out of the argument blocks of the launches queued behind it, which set their bits with atomics"""
    rig = Rig(w, dbs("minloc"), pool, "switch, seed %d" % w.seed)
    dense, sparse = slices_of(w.B), sparse_slices(w)

    def launches(firsts, n):
        d_out = pool.out(n * 64)
        for i in range(n):
            rig.device(firsts[i % len(firsts)], 64, d_out[i * 64:])
            rig.step += 1

    launches(dense, 300)
    st = rig.s.log_state()
    print("T2 after 300 dense launches: %s" % st)
    assert st["has_log"] and st["passes"] >= 1, rig.at("the pace has not started a pass: %s" % st)
    assert not st["logging"], rig.at("the pass has not switched the log off: %s" % st)
    rig.check_all("after the switch")
    # no reset: the resolvers set bits with atomics (the second slice of B holds the reads across the word at 2^18)
    launches(sparse[::3] + [dense[1]], 50)
    assert not rig.s.log_state()["logging"]
    rig.check_all("sparse reads behind the switch")
    rig.reset()
    st = rig.s.log_state()
    assert st["logging"] and st["passes"] == 0, rig.at("reset has not switched the log on: %s" % st)
    launches(sparse, 300)
    st = rig.s.log_state()
    print("T2 after reset and 300 sparse launches: %s" % st)
    assert st["passes"] >= 1 and st["logging"], rig.at("second life: %s" % st)
    rig.check_all("second life")
    g, u = rig.s.end()
    assert np.array_equal(g, rig.m.gcount) and np.array_equal(u, rig.m.ucount()), rig.at("end")
    rig.close()


# ------------------------------------------------------------------ T3
@pytest.mark.parametrize("kind", ["minloc", "ref_geometry"])
def test_bits_at_piece_and_bitmap_edges(w, dbs, pool, kind):
    """single launches of 1 .. 520 boundary reads (fewer and more than 64 workgroups: few and all regions of the log), each
    followed by an export; the same reads tallied into a second sample; kid_sample_seen_or of the three edge bits"""
    db = dbs(kind)
    rig = Rig(w, db, pool, "edges/%s, seed %d" % (kind, w.seed))
    tallied = Rig(w, db, pool, "edges/%s tallied, seed %d" % (kind, w.seed))
    c0 = a0 = 0
    for n in (1, 8, 9, 63, 64, 65, 520):
        nc = min(n, sl.NC)
        ids = np.concatenate([w.C[(c0 + np.arange(nc)) % sl.NC], w.A[a0:a0 + n - nc]])
        c0, a0 = c0 + nc, a0 + n - nc
        rig.step = tallied.step = n
        # (from nothing every time: the pass behind a launch of a few boundary reads, whose lookups meet full table lines,
        #  may find more than 8 places per read and switch the log off, and the next launch is to be logged again)
        rig.reset()
        tallied.reset()
        st = rig.s.log_state()
        assert st["has_log"] == (kind == "minloc") and st["logging"] == st["has_log"] and st["passes"] == 0, rig.at(str(st))
        rig.host(ids)
        rig.check_export()
        assert rig.s.log_state()["passes"] == (1 if kind == "minloc" else 0), rig.at("the export has not applied the log")
        rig.check_ucount(rig.sub_ranges())
        tallied.tally(ids, (0, 0))
        tallied.check_export()
        assert np.array_equal(tallied.s.seen_export(0, w.seen_bytes), rig.s.seen_export(0, w.seen_bytes)), rig.at("tallied bitmap")
    print("T3 %s after the last launch: %s" % (kind, rig.s.log_state()))
    rig.check_all("after the last launch")
    fresh = Rig(w, db, pool, "edges/%s seen_or, seed %d" % (kind, w.seed))
    fresh.seen_or([sl.N_ENTRIES - 1, PIECE, 0])
    fresh.host(np.concatenate([w.C[8:], w.A[:8]]))  # one logged launch on top (C[:8] would set those three bits itself)
    fresh.check_export()
    fresh.check_all("seen_or and a launch")
    for r in (rig, tallied, fresh):
        r.close()


# ------------------------------------------------------------------ T4
@pytest.mark.parametrize("entry", ["host", "host_async", "device_resident"])
def test_more_long_records_than_the_list_holds(w, dbs, pool, entry):
    """batches with 1100, 0, 1024 and 1025 records beyond KID_OPT_LONG_RECORD_KMERS = 256: the prepare kernel leaves those
    that no longer fit into the list (whichever they are) to the classify kernels; the option changes between batches"""
    import torch
    rig = Rig(w, dbs("minloc"), pool, "long/%s, seed %d" % (entry, w.seed))
    rng = np.random.default_rng(4)
    mixed = rng.permutation(np.concatenate([w.D, w.A[:200]]))
    batches = [(mixed, 256), (w.A[200:400], 256), (w.D[:1024], 256), (w.D[:1025], 256), (mixed, 0), (mixed, 256)]
    resident = []
    if entry == "device_resident":
        for ids, _ in batches:
            b, o, _, _ = sl.batch_of(w, ids)
            pad = np.zeros(b.size + 64, np.uint8)
            pad[:b.size] = b
            resident.append((torch.from_numpy(pad).cuda(), torch.from_numpy(o.view(np.int64)).cuda(), b.size, pool.out(len(ids))))
        torch.cuda.synchronize()
    for i, (ids, cut) in enumerate(batches):
        rig.step = i
        rig.s.set_option(KID_OPT_LONG_RECORD_KMERS, cut)
        if entry == "host":
            rig.host(ids)
        elif entry == "host_async":
            rig.host_async(ids)  # (batch 6 goes in while batch 5 is in flight)
        else:
            d_b, d_o, nbytes, d_out = resident[i]
            rig.s.classify_device(d_b.data_ptr(), nbytes, d_o.data_ptr(), len(ids), d_out=d_out.data_ptr())
            rig.pending.append((d_out[:len(ids)], rig.m.classify(ids)))
    rig.check_all("six batches", rng)
    rig.step = 6
    rig.s.set_option(KID_OPT_LONG_RECORD_KMERS, 256)
    rig.fastq(w.long_block, 0)  # a FASTQ block never takes the long path
    rig.check_all("a FASTQ block of records of 300 k-mers")
    g, u = rig.s.end()
    assert np.array_equal(g, rig.m.gcount) and np.array_equal(u, rig.m.ucount()), rig.at("end")
    rig.close()


# ------------------------------------------------------------------ T5
def _draw(w, rng, n, dense_share, long_share=0.15):
    """n reads of the pool; -> (ids, whether some have a [start, stop] of their own).  dense_share 0: a sparse life, reads
    of A, C, S and AT alone (fewer than 8 places in the hit log per read: the log stays on)"""
    sparse = dense_share == 0
    r = rng.random()
    if r < 0.1:
        trimmed = w.AT if sparse else np.concatenate([w.AT, w.BT])
        return np.concatenate([rng.choice(trimmed, n // 2 + 1), rng.choice(w.A, n // 2)])[:n], True
    if sparse:
        dense_share = long_share = 0.0
    share = np.array([1.0 - dense_share - long_share - 0.1, dense_share, 0.07, long_share, 0.03])
    groups = [w.A, w.B, w.C, w.D, w.S]
    which = rng.choice(len(groups), n, p=share / share.sum())
    ids = np.empty(n, np.int64)
    for g, group in enumerate(groups):
        ids[which == g] = rng.choice(group, int((which == g).sum()))
    return ids, False


def _first(w, rng, n, dense_share, fixed):
    """where a slice of n consecutive reads of the pool starts (fixed: 150-base reads only, 16-byte aligned); a life with
    few dense reads mostly stays clear of B"""
    if rng.random() < 1.0 - 4.0 * dense_share:
        if fixed or dense_share == 0 or rng.random() < 0.5:
            return 8 * int(rng.integers(0, (sl.NA - n) // 8 + 1))
        return int(rng.integers(int(w.C[0]), w.n_pool - n + 1))
    if fixed:
        return 8 * int(rng.integers(0, (w.n_fixed - n) // 8 + 1))
    return int(rng.integers(0, w.n_pool - n + 1))


def _life(rig, rng, n_steps, dense_share, every=40, first_reader=0):
    import torch
    w, s = rig.w, rig.s
    streams = [0] + [x.cuda_stream for x in rig.streams]
    reuse = rig.pool.out(600)  # one result array for many fixed-layout launches: the held argument block
    n_checkpoints = first_reader
    for i in range(n_steps):
        rig.step = i
        n = int(rng.integers(1, 601))
        if i % every == every - 1:
            which = n_checkpoints % 4
            n_checkpoints += 1
            rig.settle(rng)
            if which == 0:
                rig.check_gcount()
            elif which == 1:
                rig.check_ucount([(0, w.seen_bytes * 8)])
            elif which == 2:
                rig.check_ucount(rig.sub_ranges())
            else:
                rig.check_export()
            rig.check_depth()
            if rng.random() < 0.5:  # (nothing is in flight)
                rig.inputs_ready = not rig.inputs_ready
                s.set_option(KID_OPT_INPUTS_READY, int(rig.inputs_ready))
            continue
        op = rng.choice(["host", "async", "fixed_async", "fixed_device", "device", "fastq", "tally", "seen_or", "long_option"],
                        p=[0.16, 0.16, 0.1, 0.12, 0.16, 0.08, 0.12, 0.04, 0.06])
        if op == "host":
            ids, ranges = _draw(w, rng, n, dense_share)
            rig.host(ids, ranges or rng.random() < 0.3)
        elif op == "async":
            while len(rig.tickets) >= 5:
                rig.wait(int(rng.integers(0, len(rig.tickets))), again=rng.random() < 0.3)
            ids, ranges = _draw(w, rng, n, dense_share)
            rig.host_async(ids, ranges)
        elif op == "fixed_async":
            while len(rig.tickets) >= 5:
                rig.wait(int(rng.integers(0, len(rig.tickets))), again=rng.random() < 0.3)
            rig.fixed_async(_first(w, rng, n, dense_share, fixed=True), n, want_out=rng.random() < 0.7)
        elif op == "fixed_device":
            first = _first(w, rng, n, dense_share, fixed=True)
            how = rng.random()
            if how < 0.3:
                rig.fixed_device(first, n, None, stream=streams[int(rng.integers(0, 3))])
            else:  # the same result pointer as the launch before into it, another slice
                rig.settle(rng)
                rig.fixed_device(first, n, reuse, stream=streams[int(rng.integers(0, 3))])
                if how < 0.6:
                    first2 = _first(w, rng, n, dense_share, fixed=True)
                    torch.cuda.synchronize()
                    rig.settle(rng)
                    rig.fixed_device(first2, n, reuse, stream=streams[int(rng.integers(0, 3))])
        elif op == "device":
            first = _first(w, rng, n, dense_share, fixed=False)
            d_out = rig.pool.out(n) if rng.random() < 0.7 else None
            rig.device(first, n, d_out, ranges=first + n > int(w.AT[0]) or rng.random() < 0.3, stream=streams[int(rng.integers(0, 3))])
        elif op == "fastq":
            blocks = [0, 2] if dense_share == 0 else list(range(len(w.blocks)))  # (0 and 2: over slices of A)
            rig.fastq(blocks[int(rng.integers(0, len(blocks)))], int(rng.choice(sl.QS)))
        elif op == "tally":
            ids, ranges = _draw(w, rng, n, dense_share)
            rig.tally(ids, sl.RULES[int(rng.integers(0, 2))], ranges)
        elif op == "seen_or":
            rig.seen_or(rng.choice(w.valid_bits, int(rng.integers(1, 80))))
        else:
            s.set_option(KID_OPT_LONG_RECORD_KMERS, int(rng.choice([0, 256, 65536])))
    rig.settle(rng)


@pytest.mark.parametrize("kind", ["minloc", "ref_geometry"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_a_samples_life(w, dbs, pool, seed, kind):
    """400 seeded steps of every way to count into a sample, the counters read in between by every kind of reader; then
    kid_sample_end, the refusals behind it, kid_sample_reset and a second life of 100 steps on the same handle.  The first
    life mixes dense reads and long records in (the first reader's pass switches the log off); the second is sparse, and
    there the log must still be on behind every kind of reader."""
    import torch
    rig = Rig(w, dbs(kind), pool, "life/%s, seed %d" % (kind, seed), depth=True)
    rig.streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    rig.inputs_ready = False
    dense_share = (0.03, 0.1, 0.25)[seed]
    for life, (n_steps, rng_seed, dense) in enumerate([(400, seed, dense_share), (100, 1000 + seed, 0.0)]):
        rig.tag = "life/%s, seed %d, life %d" % (kind, seed, life + 1)
        rng = np.random.default_rng(rng_seed)
        _life(rig, rng, n_steps, dense, every=40 if life == 0 else 20, first_reader=life)
        st = rig.s.log_state()
        print("T5 %s seed %d life %d: %s, %s" % (kind, seed, life + 1, st, rig.m.stats()))
        if life == 1 and kind == "minloc":  # five checkpoints, four of them readers that apply the log, logged launches between them
            assert st["has_log"] and st["passes"] >= 4 and st["logging"], rig.at("the sparse life has not kept its log: %s" % st)
        g, u = rig.s.end()
        rig.step = n_steps
        assert np.array_equal(g, rig.m.gcount) and np.array_equal(u, rig.m.ucount()), rig.at("end")
        rig.check_all("after end", rng)
        b, o, _, _ = sl.batch_of(w, w.C)
        for refused in (lambda: rig.s.classify(b, o), lambda: rig.db.read_support(b, o, tally=rig.s),
                        lambda: rig.s.classify_fixed_device(pool.bases.data_ptr(), L, 8)):
            with pytest.raises(kmer_id_amd.KidError) as e:
                refused()
            assert e.value.status == -10, rig.at("a call after kid_sample_end")
        rig.check_all("after the refused calls", rng)  # nothing of them was counted
        rig.reset()
    rig.close()
