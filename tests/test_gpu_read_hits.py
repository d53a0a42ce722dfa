"""kid_db_read_hits* (every read's k-mer hits, in read-position order) against the independent model of
tests/read_hits_model.py, against the classify path of the same library, and against its own contract.
Every comparison is exact: the values are integers."""
import ctypes as C

import numpy as np
import pytest

import read_hits_cases as cases
from helpers import DeviceBatch, concat_reads, fastq_block, ob, oracle_db
from kmer_id_amd import KID_FLAG_HOST_BUILD, KID_FLAG_REF_GEOMETRY, KID_FLAG_U_IS_T, KidError, KmerDB, _lib, synth
from read_calls import KINDS
from read_hits_model import HitModel, trim_ranges, windows

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", np.uint8)


def same_hits(got, exp, what=""):
    """offsets, n_kmers, pos, target, entry equal; names the first read that differs"""
    n = exp.offsets.size - 1
    assert got.offsets.size == n + 1 and got.n_kmers.size == n, what
    if not np.array_equal(got.n_kmers, exp.n_kmers):
        r = int(np.flatnonzero(got.n_kmers != exp.n_kmers)[0])
        raise AssertionError("%s: read %d looked up %d windows, the model %d" % (what, r, got.n_kmers[r], exp.n_kmers[r]))
    for r in range(n):
        g, e = got.of(r), exp.of(r)
        if not all(np.array_equal(a, b) for a, b in zip(g, e)):
            raise AssertionError("%s: read %d: hits (pos, target, entry)\n  got   %s\n  model %s" % (
                what, r, list(zip(*[x.tolist() for x in g])), list(zip(*[x.tolist() for x in e]))))
    assert np.array_equal(got.offsets, exp.offsets), what
    assert got.pos.dtype == got.target.dtype == got.entry.dtype == np.uint32 and got.offsets.dtype == np.uint64


def seeded_reads(cum, parent, keys, k):
    """150- and 250-base synthetic reads, then the adversarial ragged set (31, 30, 29 bases and odd bytes among them)"""
    parts = []
    for n, length in ((4000, 150), (600, 250)):
        b, o = cases.synth_reads(cum, parent, n, length, k=k)
        parts += [b[int(o[i]):int(o[i + 1])].tobytes() for i in range(n)]
    b, o = cases.adversarial_reads(keys, k, seed=5)
    raw = bytes(b)
    parts += [raw[int(o[i]):int(o[i + 1])] for i in range(o.size - 1)]
    return concat_reads(parts)


def gpu_fold(db, hits):
    """process_read's left fold of every read's hits, with the library's msca (KmerDB.msca), all reads in step"""
    n = len(hits)
    per = np.diff(hits.offsets.astype(np.int64))
    f = np.zeros(n, np.int64)
    for j in range(int(per.max()) if n else 0):
        rs = np.flatnonzero(per > j)
        t = hits.target[hits.offsets[rs].astype(np.int64) + j].astype(np.int64)
        cur = f[rs]
        new = t.copy()
        m = cur > 0
        if m.any():
            new[m] = db.msca(t[m], cur[m])
        f[rs] = new
    return f


def seen_entries(sample):
    bits = np.unpackbits(sample.seen_export(0, sample.seen_bytes()), bitorder="little")
    return np.flatnonzero(bits)


# ------------------------------------------------------------------ 1. the model, three table kinds, duplicate keys
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_seeded_reads_equal_the_model(kind):
    parent, cum, keys, targets = cases.database(30, 2e-4, dup=True)
    odb = oracle_db(parent, keys, targets, 20)
    model = HitModel(odb, keys, targets, 30)
    bases, off = seeded_reads(cum, parent, keys, 30)
    exp = model.batch(bases, off)
    # the case set is worth something: enough hits, reads with several, and an order that matters
    per = np.diff(exp.offsets.astype(np.int64))
    assert int(exp.offsets[-1]) >= 1000 and int((per >= 3).sum()) >= 100
    assert any(model.fold(exp.of(r)[1]) != model.fold(exp.of(r)[1][::-1]) for r in np.flatnonzero(per >= 2))
    lens = np.diff(off.astype(np.int64))
    assert {150, 250, 31, 30, 29} <= set(lens.tolist())
    db = KmerDB(keys, targets, parent, k=30, log2_slots=20, flags=KINDS[kind])
    info = db.info
    assert info.geometry == (1 if kind == "minloc" else 0) and info.host_built == (1 if kind == "host_build" else 0)
    got = db.read_hits(bases, off)
    same_hits(got, exp, kind)
    # duplicates: no hit names an entry of the re-inserted tail, though many hits have a key that was inserted twice
    n_orig = int(cum[-1])
    assert keys.size > n_orig and int(got.entry.max()) < n_orig
    assert int(np.isin(keys[got.entry], keys[n_orig:]).sum()) > 100


def test_table_kinds_are_byte_identical_and_runs_repeat():
    parent, cum, keys, targets = cases.database(30, 2e-4, dup=True)
    bases, off = seeded_reads(cum, parent, keys, 30)
    outs = []
    for kind in sorted(KINDS):
        db = KmerDB(keys, targets, parent, k=30, log2_slots=20, flags=KINDS[kind])
        for _ in range(2):
            h = db.read_hits(bases, off)
            outs.append(b"".join(a.tobytes() for a in (h.offsets, h.n_kmers, h.pos, h.target, h.entry)))
        db.close()
    assert len(set(outs)) == 1


# ------------------------------------------------------------------ 2. cross-checks against the classify path
def cross_check(db, bases, off, start=None, stop=None):
    hits = db.read_hits(bases, off, start, stop)
    s = db.sample()
    final = s.classify(bases, off, start, stop)
    st = s.stats()
    assert np.array_equal(gpu_fold(db, hits), final.astype(np.int64)), "fold(hit list) != final target"
    assert int(hits.n_kmers.sum()) == st["lookups"]
    assert int(hits.offsets[-1]) == st["hits"]
    assert np.array_equal(np.unique(hits.entry[hits.target > 1]), seen_entries(s)), "{entries hit} != seen bitmap"
    s.close()
    return hits, final


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_hits_explain_the_classify_path(kind):
    parent, cum, keys, targets = cases.database(30, 2e-4, dup=True)
    bases, off = seeded_reads(cum, parent, keys, 30)
    db = KmerDB(keys, targets, parent, k=30, log2_slots=20, flags=KINDS[kind])
    hits, final = cross_check(db, bases, off)
    assert int((final > 1).sum()) > 1000


# ------------------------------------------------------------------ 3. edges
def heap_taxonomy(ntar, rng, fan=8):
    """a heap-shaped tree under root 1 with its ids shuffled: ancestors anywhere in the id range"""
    i = np.arange(ntar)
    hp = np.ones(ntar, np.int64)
    hp[2:] = (i[2:] - 2) // fan + 1
    perm = np.arange(ntar)
    perm[2:] = 2 + rng.permutation(ntar - 2)
    parent = np.ones(ntar, np.int32)
    parent[perm[2:]] = perm[hp[2:]]
    return parent


def genome_database(parent, k, rng, n_genomes, genome_len, every=1):
    """the canonical k-mers (every `every`-th window) of random genomes; genome 0 under the last target alone, the
    others walking a lineage with a few foreign nodes in between -> genomes, keys, targets"""
    ntar = parent.size
    genomes, keys, targets = [], [], []
    for g in range(n_genomes):
        seq = rng.choice(ACGT, genome_len).tobytes()
        key, _ = windows(seq, 0, genome_len - 1, k)
        key = key[::every]
        if g == 0:
            tg = np.full(key.size, ntar - 1, np.uint32)
        else:
            t0 = int(rng.integers(ntar // 2, ntar))
            lineage = np.array([t0, parent[t0], parent[parent[t0]]], np.uint32)
            tg = lineage[rng.integers(0, 3, key.size)]
            foreign = rng.random(key.size) < 0.03
            tg[foreign] = rng.integers(2, ntar, int(foreign.sum())).astype(np.uint32)
        genomes.append(seq)
        keys.append(key)
        targets.append(tg)
    return genomes, np.concatenate(keys), np.concatenate(targets)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_large_targets_odd_last_target_and_hit_dense_reads(kind):
    rng = np.random.default_rng(40001)
    ntar, k = 40001, 30  # ids >= 32768; the last target has an odd place in a two-per-word histogram
    parent = heap_taxonomy(ntar, rng)
    genomes, keys, targets = genome_database(parent, k, rng, 24, 1200)
    comp = cases.COMP
    seqs = []
    for i in range(300):
        g = genomes[0 if i % 6 == 0 else int(rng.integers(0, len(genomes)))]
        length = int(rng.integers(60, 200)) + k - 1
        p = int(rng.integers(0, len(g) - length + 1))
        s = g[p:p + length]
        seqs.append(s.translate(comp)[::-1] if i % 2 else s)
    bases, off = concat_reads(seqs)
    odb = oracle_db(parent, keys, targets, 16)
    exp = HitModel(odb, keys, targets, k).batch(bases, off)
    per = np.diff(exp.offsets.astype(np.int64))
    assert int(per.min()) >= 60 and np.array_equal(per, exp.n_kmers)  # every window a hit
    assert int((exp.target >= 32768).sum()) > 1000 and int((exp.target == ntar - 1).sum()) > 1000
    db = KmerDB(keys, targets, parent, k=k, log2_slots=16, flags=KINDS[kind])
    same_hits(db.read_hits(bases, off), exp, kind)
    cross_check(db, bases, off)


@pytest.mark.parametrize("kind", ["minloc", "ref_geometry"])
def test_long_records(kind):
    """a 200 kb record (more windows than KID_OPT_LONG_RECORD_KMERS' default, 65536), one of 60 kb below it, short reads
    around them; every 40th window of the records is in the database"""
    rng = np.random.default_rng(200000)
    k = 30
    parent, cum, keys0, targets0 = cases.database(k, 1e-4)
    genomes, gkeys, gt = genome_database(parent, k, rng, 3, 200000, every=40)
    keys = np.concatenate([keys0, gkeys])
    targets = np.concatenate([targets0, (gt % np.uint32(parent.size - 2)) + np.uint32(2)])
    sb, so = cases.synth_reads(cum, parent, 50, 150)
    short = [sb[int(so[i]):int(so[i + 1])].tobytes() for i in range(50)]
    g1 = bytearray(genomes[1])
    g1[30000] = ord("N")
    seqs = short[:20] + [genomes[0]] + short[20:30] + [bytes(g1)[:60000]] + short[30:] + [genomes[2][:65536 + k - 1], genomes[2][:65537 + k - 1]]
    bases, off = concat_reads(seqs)
    odb = oracle_db(parent, keys, targets, 18)
    exp = HitModel(odb, keys, targets, k).batch(bases, off)
    per = np.diff(exp.offsets.astype(np.int64))
    assert int(per[20]) >= 4000 and int(per[31]) >= 1000
    db = KmerDB(keys, targets, parent, k=k, log2_slots=18, flags=KINDS[kind])
    same_hits(db.read_hits(bases, off), exp, kind)
    cross_check(db, bases, off)


def test_probe_cap_of_m3_on_a_nearly_full_table():
    parent, cum, keys, targets = cases.database(30, 2e-4)
    keys, targets = keys[:15000], targets[:15000]
    bases, off = cases.adversarial_reads(keys, 30, seed=3, n=900)
    capped = oracle_db(parent, keys, targets, 14, max_probes=16)
    free = oracle_db(parent, keys, targets, 14)
    exp = HitModel(capped, keys, targets, 30).batch(bases, off)
    unbounded = HitModel(free, keys, targets, 30).batch(bases, off)
    assert 0 < int(exp.offsets[-1]) < int(unbounded.offsets[-1])  # the cap hides keys
    db = KmerDB(keys, targets, parent, k=30, log2_slots=14, max_probes=16)
    same_hits(db.read_hits(bases, off), exp, "max_probes 16")
    cross_check(db, bases, off)
    db2 = KmerDB(keys, targets, parent, k=30, log2_slots=14, flags=KID_FLAG_HOST_BUILD)
    same_hits(db2.read_hits(bases, off), unbounded, "unbounded")


def test_u_is_t():
    parent, cum, keys, targets = cases.database(30, 1e-4)
    bases, off = cases.adversarial_reads(keys, 30, seed=11, u=True)
    totals = []
    for oflag, flag in ((0, 0), (ob.KO_FLAG_U_IS_T, KID_FLAG_U_IS_T)):
        odb = oracle_db(parent, keys, targets, 18, flags=oflag)
        exp = HitModel(odb, keys, targets, 30, u_is_t=bool(flag)).batch(bases, off)
        for geo in (0, KID_FLAG_REF_GEOMETRY):
            db = KmerDB(keys, targets, parent, k=30, log2_slots=18, flags=flag | geo)
            same_hits(db.read_hits(bases, off), exp, "flags %d" % (flag | geo))
        totals.append(int(exp.offsets[-1]))
    assert totals[1] > totals[0]


@pytest.mark.parametrize("k", [15, 21, 31])
def test_other_k(k):
    parent, cum, keys, targets = cases.database(k, 1e-4, dup=True)
    odb = oracle_db(parent, keys, targets, 18, k=k)
    model = HitModel(odb, keys, targets, k)
    b1, o1 = cases.synth_reads(cum, parent, 800, 150, k=k)
    b2, o2 = cases.adversarial_reads(keys, k, seed=k)
    raw1, raw2 = bytes(b1), bytes(b2)
    bases, off = concat_reads([raw1[int(o1[i]):int(o1[i + 1])] for i in range(800)] +
                              [raw2[int(o2[i]):int(o2[i + 1])] for i in range(o2.size - 1)])
    exp = model.batch(bases, off)
    assert int(exp.offsets[-1]) > 500
    for kind in sorted(KINDS):
        db = KmerDB(keys, targets, parent, k=k, log2_slots=18, flags=KINDS[kind])
        same_hits(db.read_hits(bases, off), exp, "k %d %s" % (k, kind))
        cross_check(db, bases, off)


# ------------------------------------------------------------------ 4. the contract
@pytest.fixture(scope="module")
def contract():
    parent, cum, keys, targets = cases.database(30, 2e-4)
    bases, off = seeded_reads(cum, parent, keys, 30)
    db = KmerDB(keys, targets, parent, k=30, log2_slots=20)
    return db, parent, cum, keys, targets, bases, off, db.read_hits(bases, off)


def raw_call(db, bases, off, hits, cap, start=None, stop=None):
    lib = _lib.load()
    n = off.size - 1
    ho = np.full(n + 1, 0xDEADBEEF, np.uint64)
    nk = np.full(n, 0xDEADBEEF, np.uint32)
    tot = C.c_uint64(12345)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
    rc = lib.kid_db_read_hits(db._h, p(bases), p(off), p(start), p(stop), n, p(ho), p(nk), p(hits), cap, C.byref(tot))
    return rc, ho, nk, tot.value


def test_sizing_call_and_cap(contract):
    db, parent, cum, keys, targets, bases, off, ref = contract
    total = int(ref.offsets[-1])
    assert total > 1000
    rc, ho, nk, tot = raw_call(db, bases, off, None, 0)  # the sizing call
    assert rc == 0 and tot == total and np.array_equal(ho, ref.offsets) and np.array_equal(nk, ref.n_kmers)
    canary = np.full((total + 8) * 3, 0xA5A5A5A5, np.uint32)
    buf = canary.copy()
    rc, ho, nk, tot = raw_call(db, bases, off, buf, total - 1)  # one short: nothing written, KID_OK, the true count
    assert rc == 0 and tot == total and np.array_equal(buf, canary) and np.array_equal(ho, ref.offsets)
    rc, ho, nk, tot = raw_call(db, bases, off, buf, total)  # exact
    assert rc == 0 and tot == total
    got = buf[:total * 3].reshape(-1, 3)
    assert np.array_equal(got[:, 0], ref.pos) and np.array_equal(got[:, 1], ref.target) and np.array_equal(got[:, 2], ref.entry)
    assert np.array_equal(buf[total * 3:], canary[total * 3:])


def test_empty_batch_and_reads_without_windows(contract):
    db = contract[0]
    h = db.read_hits(np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    assert h.offsets.tolist() == [0] and h.n_kmers.size == 0 and h.pos.size == 0
    bases, off = concat_reads([b"", b"ACGT" * 7, b"N" * 100, b"ACGT" * 7 + b"A", b""])  # 0, 28, 100 x N, 29, 0 bytes
    h = db.read_hits(bases, off)
    assert h.offsets.tolist() == [0] * 6 and h.n_kmers.tolist() == [0] * 5


def test_any_split_into_calls_concatenates(contract):
    db, parent, cum, keys, targets, bases, off, ref = contract
    n = off.size - 1
    for parts in (1, 2, 7):
        cuts = [n * i // parts for i in range(parts + 1)]
        pos, tgt, ent, nk, counts = [], [], [], [], []
        for a, b in zip(cuts[:-1], cuts[1:]):
            h = db.read_hits(bases, off[a:b + 1])  # offsets that do not start at 0
            pos.append(h.pos); tgt.append(h.target); ent.append(h.entry); nk.append(h.n_kmers)
            counts.append(np.diff(h.offsets.astype(np.int64)))
        assert np.array_equal(np.concatenate(pos), ref.pos) and np.array_equal(np.concatenate(tgt), ref.target)
        assert np.array_equal(np.concatenate(ent), ref.entry) and np.array_equal(np.concatenate(nk), ref.n_kmers)
        assert np.array_equal(np.concatenate(counts), np.diff(ref.offsets.astype(np.int64)))


def test_fastq_block_form_equals_host_form(contract):
    db, parent, cum, keys, targets = contract[:5]
    n, length = 1500, 150
    bases, off = cases.synth_reads(cum, parent, n, length)
    quals = synth.qualities(n, length)
    seqs = [bases[i * length:(i + 1) * length].tobytes() for i in range(n)]
    qs = [q.tobytes() for q in quals]
    seqs += [b"ACGT" * 5, b"", seqs[3][:31]]  # records too short for a k-mer
    qs += [b"I" * 20, b"", b"I" * 31]
    start, stop, keep = trim_ranges(qs, [len(s) for s in seqs], 30)
    assert 0 < int((~keep).sum()) and int(keep.sum()) > 1000
    start[~keep], stop[~keep] = 1, 0  # the host form's way of saying "no range"
    text, recs = fastq_block(seqs, qs)
    got = db.read_hits_fastq(text, recs)
    b2, o2 = concat_reads(seqs)
    host = db.read_hits(b2, o2, start, stop)
    same_hits(got, host, "FASTQ block vs host form")
    odb = oracle_db(parent, keys, targets, 20)
    same_hits(got, HitModel(odb, keys, targets, 30).batch(b2, o2, start, stop), "FASTQ block vs model")
    assert int(got.offsets[-1]) > 500 and np.all(got.n_kmers[~keep] == 0)
    # a quality line shorter than its sequence: qual.at() throws in the reference
    recs_bad = recs.copy()
    recs_bad[7, 3] -= 1
    with pytest.raises(KidError) as e:
        db.read_hits_fastq(text, recs_bad)
    assert e.value.status == -9  # KID_ERR_FORMAT
    same_hits(db.read_hits_fastq(text, recs), got, "after the error")


def test_argument_errors(contract):
    db, parent, cum, keys, targets, bases, off, ref = contract
    bad = off[:10].copy()
    bad[4] = bad[3] - np.uint64(1)
    with pytest.raises(KidError) as e:
        db.read_hits(bases, bad)
    assert e.value.status == -1
    n = 9
    start, stop = np.zeros(n, np.int32), np.full(n, 149, np.int32)
    stop[2] = 150  # one past the read
    with pytest.raises(KidError) as e:
        db.read_hits(bases, off[:10], start, stop)
    assert e.value.status == -1
    lib = _lib.load()
    tot = C.c_uint64(0)
    ho = np.zeros(1, np.uint64)
    rc = lib.kid_db_read_hits(db._h, None, None, None, None, 1 << 31, ho.ctypes.data_as(C.c_void_p), None, None, 0, C.byref(tot))
    assert rc == -1  # more than 2^31-1 reads


def test_device_form_equals_host_form(contract):
    db, parent, cum, keys, targets, bases, off, ref = contract
    n = off.size - 1
    total = int(ref.offsets[-1])
    db.read_hits_time()
    with DeviceBatch(bases, off, total) as d:
        for cap, filled in ((0, False), (total - 1, False), (total, True)):
            d.run(db, cap)
            assert int(d.down(d.d_tot, np.uint64, 1)[0]) == total
            assert np.array_equal(d.down(d.d_ho, np.uint64, n + 1), ref.offsets)
            assert np.array_equal(d.down(d.d_nk, np.uint32, n), ref.n_kmers)
            h = d.down(d.d_hits, np.uint32, d.canary.size)
            if filled:
                got = h[:total * 3].reshape(-1, 3)
                assert np.array_equal(got[:, 0], ref.pos) and np.array_equal(got[:, 1], ref.target) and np.array_equal(got[:, 2], ref.entry)
                assert np.array_equal(h[total * 3:], d.canary[total * 3:])
            else:
                assert np.array_equal(h, d.canary)
        ms, calls, reads = db.read_hits_time()
        assert calls == 3 and reads == 3 * n and ms > 0
        assert db.read_hits_time() == (0.0, 0, 0)


def test_more_tiles_than_the_text_can_hold_are_refused_not_written(contract):
    """The tile scratch of the device form is sized by bases_nbytes / 64 + reads.  Offsets that reach beyond the
    bases_nbytes the caller named make more tiles than that: the batch gets no hits (every offset 0, nothing written),
    the next kid_db_read_hits_time says KID_ERR_ARG, and the call after that works."""
    db, parent, cum, keys, targets, bases, off, ref = contract
    n = off.size - 1
    total = int(ref.offsets[-1])
    db.read_hits_time()
    with DeviceBatch(bases, off, total) as d:
        d.run(db, total, nbytes=64)
        assert int(d.down(d.d_tot, np.uint64, 1)[0]) == 0
        assert not d.down(d.d_ho, np.uint64, n + 1).any() and not d.down(d.d_nk, np.uint32, n).any()
        assert np.array_equal(d.down(d.d_hits, np.uint32, d.canary.size), d.canary)
        with pytest.raises(KidError) as e:
            db.read_hits_time()
        assert e.value.status == -1
        d.run(db, total)
        assert np.array_equal(d.down(d.d_ho, np.uint64, n + 1), ref.offsets)
        db.read_hits_time()


def test_fastq_records_that_share_their_sequence_bytes(contract):
    """records may alias or overlap in the text block (the classify form accepts them too): as many tiles as records,
    in a text of a few hundred bytes"""
    db, parent, cum, keys, targets, bases, off, ref = contract
    per = np.diff(ref.offsets.astype(np.int64))
    r = int(np.flatnonzero((per >= 3) & (np.diff(off.astype(np.int64)) == 250))[0])
    seq = bases[int(off[r]):int(off[r + 1])].tobytes()
    text, recs = fastq_block([seq], [b"I" * len(seq)])
    n = 3000
    many = np.repeat(recs, n, axis=0)
    many[1::2, 0] += 40   # every other record: the same line from byte 40 on
    many[1::2, 1] -= 40
    many[1::2, 3] -= 40
    got = db.read_hits_fastq(text, many)
    b2, o2 = concat_reads([seq if i % 2 == 0 else seq[40:] for i in range(n)])
    same_hits(got, db.read_hits(b2, o2), "aliased records")
    assert int(got.offsets[-1]) >= 3 * n // 2 and np.array_equal(got.of(0)[0], ref.of(r)[0])


def test_a_samples_counters_are_untouched(contract):
    db, parent, cum, keys, targets, bases, off, ref = contract
    s = db.sample()
    s.classify(bases[:int(off[500])], off[:501])
    before = (s.gcount().copy(), s.stats(), s.seen_export(0, s.seen_bytes()).copy())
    db.read_hits(bases, off)
    text, recs = fastq_block([bases[:150].tobytes()] * 3, [b"I" * 150] * 3)
    db.read_hits_fastq(text, recs)
    with DeviceBatch(bases, off, int(ref.offsets[-1])) as d:
        d.run(db, int(ref.offsets[-1]))
        assert np.array_equal(d.down(d.d_ho, np.uint64, off.size), ref.offsets)
    after = (s.gcount(), s.stats(), s.seen_export(0, s.seen_bytes()))
    assert np.array_equal(before[0], after[0]) and before[1] == after[1] and np.array_equal(before[2], after[2])
    g, u = s.end()
    s2 = db.sample()
    s2.classify(bases[:int(off[500])], off[:501])
    g2, u2 = s2.end()
    assert np.array_equal(g, g2) and np.array_equal(u, u2)
