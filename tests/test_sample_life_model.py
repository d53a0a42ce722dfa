"""tests/sample_life.py on the CPU: the mirror of a sample against the oracle, and the properties of the seeded pool that
tests/test_gpu_sample_life.py relies on.  The latter are conditions on the inputs: a seed that misses one is replaced,
the assertion stays."""
import numpy as np
import pytest

import sample_life as sl
from helpers import ob
from read_support_cases import random_keys


@pytest.fixture(scope="module")
def w():
    return sl.world()


def _oracle_over_everything(w):
    """the pool and the kept records of every FASTQ block (minimum base quality 0) through one oracle sample"""
    os_ = ob.OracleSample(w.odb)
    os_.classify(w.bases, w.off, w.start, w.stop)
    for b in w.blocks:
        kept = np.flatnonzero(b["keep"])
        raw = bytes(b["text"])
        seqs = [np.frombuffer(raw[so:so + sl_], np.uint8) for so, sl_, _, _ in b["recs"][kept].tolist()]
        bases, off = sl.gather(seqs)
        os_.classify(bases, off, b["start"][kept], b["stop"][kept])
    return os_.counts(), os_.stats()


def test_the_vectorised_keys_are_random_keys():
    assert np.array_equal(sl.random_canonical_keys(np.random.default_rng(3), 200), random_keys(np.random.default_rng(3), 200))


def test_database_layout(w):
    assert sl.N_ENTRIES == 528289 and w.keys.size == sl.N_ENTRIES and sl.N_ENTRIES % 128 == 33
    assert w.seen_bytes * 8 == 3 * sl.PIECE - (sl.PIECE - 128 * 32)  # two whole pieces and 128 words of the third
    assert int((w.targets == 1).sum()) == 12
    # the duplicates repeat earlier keys under another target
    for d, s in zip(sl.DUPS, w.dup_sources):
        assert w.keys[d] == w.keys[s] and s < d and w.targets[d] != w.targets[s] and w.targets[d] > 1
    # the two boundary entries are neighbouring windows of one genome
    g = w.genomes[w.boundary_genome]
    a = sl.HitModel(w.odb, w.keys, w.targets, sl.K).batch(g[w.boundary_window:w.boundary_window + 31], np.array([0, 31], np.uint64))
    assert a.entry.tolist() == [sl.PIECE - 1, sl.PIECE]


@pytest.mark.parametrize("split", ["in_order", "reversed_in_uneven_batches", "shuffled_with_repeats_of_nothing"])
def test_the_mirror_equals_the_oracle(w, split):
    (eg, eu), est = _oracle_over_everything(w)
    m = sl.SampleMirror(w)
    rng = np.random.default_rng(5)
    blocks = list(range(len(w.blocks)))
    if split == "in_order":
        assert np.array_equal(m.classify(np.arange(w.n_pool)), w.final)
        for b in blocks:
            m.classify_fastq(b, 0)
    elif split == "reversed_in_uneven_batches":
        ids = np.arange(w.n_pool)[::-1]
        cuts = np.unique(np.concatenate([[0, 1, 9, 73, 74, w.n_pool], rng.integers(0, w.n_pool, 40)]))
        for b in blocks[::-1]:
            m.classify_fastq(b, 0)
        for a, b in zip(cuts[:-1], cuts[1:]):
            m.classify(ids[a:b])
    else:
        ids = rng.permutation(w.n_pool)
        parts = np.array_split(ids, 23)
        for i, p in enumerate(parts):
            m.classify(p)
            if i < len(blocks):
                m.classify_fastq(blocks[i], 0)
            m.classify(np.empty(0, np.int64))
    assert np.array_equal(m.gcount, eg) and np.array_equal(m.ucount(), eu)
    dropped = sum(int((~b["keep"]).sum()) for b in w.blocks)
    assert m.stats() == {"reads": int(eg.sum()) + dropped, "lookups": est["lookups"], "hits": est["hits"]}
    assert m.reads == w.n_pool + sum(b["n"] for b in w.blocks) and dropped > 0
    assert np.array_equal(m.ucount(0, sl.PIECE) + m.ucount(sl.PIECE, 2 * sl.PIECE) + m.ucount(2 * sl.PIECE, None), eu)
    bm = m.bitmap_bytes()
    assert bm.size == w.seen_bytes and int(np.unpackbits(bm).sum()) == int(eu.sum())
    assert not m.seen[sl.DUPS].any() and not m.seen[w.targets == 1].any()


def test_a_tally_under_0_0_counts_what_classifying_counts(w):
    a, b = sl.SampleMirror(w), sl.SampleMirror(w)
    ids = np.random.default_rng(9).permutation(w.n_pool)
    a.classify(ids)
    for p in np.array_split(ids, 7):
        b.tally(p, (0, 0))
    assert np.array_equal(a.gcount, b.gcount) and np.array_equal(a.seen, b.seen)
    assert b.stats() == {"reads": 0, "lookups": 0, "hits": 0} and int(b.depth.sum()) > int(b.seen.sum())
    assert np.array_equal(b.depth > 0, b.seen)
    c = sl.SampleMirror(w)
    c.tally(ids, (2, 25))
    assert int(c.gcount[0]) > int(a.gcount[0]) and int(c.seen.sum()) < int(a.seen.sum())
    c.seen_or([0, sl.PIECE, sl.N_ENTRIES - 1])
    assert c.seen[0] and c.seen[sl.PIECE] and c.bitmap_bytes()[(sl.N_ENTRIES - 1) // 8] >> ((sl.N_ENTRIES - 1) % 8) & 1


def test_the_pool_has_what_the_gpu_tests_rely_on(w):
    entries_of = lambda ids: set(w.hits.entry[sl.csr_take(w.hits.offsets, ids)[0]].tolist())  # noqa: E731
    everything = np.array(sorted(entries_of(np.arange(w.n_pool))))
    for piece in range(3):  # hits in all three pieces
        assert ((everything >> 18) == piece).any()
    # every planted ordinal is hit by the C reads that carry it
    for r, which in zip(w.C, w.c_planted):
        assert set(which) <= entries_of([r]), (r, which)
    assert {o for which in w.c_planted for o in which} == set(sl.PLANTED)
    # dense reads across the piece boundary
    crossing = [r for r in w.B if {sl.PIECE - 1, sl.PIECE} <= entries_of([r])]
    assert len(set(crossing) & set(w.B[64:128].tolist())) >= 8  # (the second slice of 64: T2 launches it behind the switch)
    per_read = np.diff(w.hits.offsets.astype(np.int64))
    assert per_read[w.B].mean() > 30 and per_read[w.A].mean() < 4 and per_read[w.C].mean() < 4  # dense / sparse by a wide margin around 8
    # target-1 hits and reads without a hit
    assert int((w.hits.target == 1).sum()) >= 10 and int((w.final[w.A] == 1).sum()) >= 1
    none = int((per_read[w.A] == 0).sum())
    assert 0.4 * sl.NA < none < 0.6 * sl.NA
    # the long records: the fold order matters for at least a tenth
    assert int((per_read[w.D] >= 1).all()) and int((w.n_kmers[w.D] == 300).all())
    assert int((w.final_reversed_D != w.final[w.D]).sum()) >= 110
    assert w.n_kmers[w.S].tolist() == [0, 0, 0, 1, 2] and per_read[w.S].tolist() == [0, 0, 0, 1, 1]
    # trimmed reads: ranges inside the reads, some cut, some without a window
    lens = np.diff(w.off.astype(np.int64))
    t = np.concatenate([w.AT, w.BT])
    assert ((w.start[t] > w.stop[t]) | ((w.start[t] >= 0) & (w.stop[t] < lens[t]))).all()
    assert int((w.n_kmers[t] < 121).sum()) > 50 and int((w.n_kmers[t] == 0).sum()) >= 1
    # FASTQ: kept and dropped records, a final that changes under Q = 20, masked bases
    keep = np.concatenate([b["keep"] for b in w.blocks])
    assert keep.any() and (~keep).any()
    changed = sum(int((b[0]["final"] != b[20]["final"]).sum()) for b in w.blocks)
    assert changed >= 1 and all(b[0]["masked"] == 0 for b in w.blocks) and sum(b[20]["masked"] for b in w.blocks) > 100
    lb = w.blocks[w.long_block]
    assert lb["keep"].all() and np.array_equal(lb[0]["final"], w.final[w.D[:20]]) and lb[20]["masked"] == 0
