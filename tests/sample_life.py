"""Inputs and a model for the tests of a sample's life (tests/test_sample_life_model.py on the CPU,
tests/test_gpu_sample_life.py on the GPU): one database whose entry ordinals sit on the edges of the seen-bitmap's pieces,
a pool of reads whose per-read facts are computed once, and SampleMirror, a sample's counters as plain arithmetic on those
facts.  No test functions here.

The facts come from the oracle (OracleSample.classify: `final`) and from the independent models of the suite
(read_hits_model.HitModel: windows looked up and the hits {pos, target, entry}; read_support_model.SupportModel and
read_depth_model.depth_of: what a tally counts).  Nothing of the library under test decides an expectation.

The database (k = 30, taxonomy bact10, 2^21 slots): N_ENTRIES = 2 * 2^18 + 4001 entries, so the bitmap has three pieces of
2^18 bits, the last one with 128 valid words, and N_ENTRIES % 128 = 33.
  * random canonical keys under random targets > 1 everywhere else
  * the k-mers of 40 random genomes (2529 bases, 2500 windows each; genome_cases.genome_db) at the ordinals
    [2^18 - 50000, 2^18 + 50000), rotated so that two NEIGHBOURING windows of one genome, both canonical, are the entries
    2^18 - 1 and 2^18: the hits of a dense read cross the piece boundary
  * PLANTED ordinals (0, 31, 32, 2^18 - 1, 2^18, 2^19 - 1, 2^19, N_ENTRIES - 1): each holds the first insert of a canonical
    key of target > 1 -- the two inside the genome block are those two genome k-mers
  * twelve entries of target 1, and at the ordinals N_ENTRIES - 21 .. N_ENTRIES - 2 twenty duplicates of earlier keys under
    another target, whose bits are never set

The pool (every read 150 bases unless said otherwise; ids in this order):
  A   4096 sparse reads: random bases, about half with one or two implanted database k-mers from outside the genome
      block (either strand), some of target 1
  B   2048 dense reads cut from the genomes, both strands; B[70:80] cover the two windows at the piece boundary
  C   64 boundary reads with the planted k-mers of one, two or three edge ordinals
  D   1100 records of 329 bases (300 windows) with one to three implanted k-mers of unrelated targets, then S: reads of
      0, 1, 29, 30 and 31 bases
  AT, BT   A[:512] and B[:256] once more, with the [start, stop] process_qual gives for synth.qualities
  E   FASTQ blocks over slices of A and B with synth.qualities, and one of twenty D records of quality 'I'; their facts
      under KID_OPT_MIN_BASE_QUALITY 0 and 20 (the masked case by the header's defining property: the masked bytes
      replaced by 'N', then the oracle)
"""
import functools

import numpy as np

from genome_cases import genome_db
from helpers import K, fastq_block, ob, oracle_db, synth
from read_depth_model import depth_of, saturating_add
from read_hits_model import Hits, HitModel, trim_ranges
from read_support_model import SupportModel

ACGT = np.frombuffer(b"ACGT", np.uint8)
COMP = np.zeros(256, np.uint8)
for _a, _b in zip(b"ACGTN", b"TGCAN"):
    COMP[_a] = _b
PIECE = 1 << 18
N_ENTRIES = 2 * PIECE + 4001
LOG2_SLOTS = 21
PLANTED = [0, 31, 32, PIECE - 1, PIECE, 2 * PIECE - 1, 2 * PIECE, N_ENTRIES - 1]
G0, G1 = PIECE - 50000, PIECE + 50000
N_GENOMES, GENOME_LEN, GENOME_WIN = 40, 2529, 2500
DUPS = np.arange(N_ENTRIES - 21, N_ENTRIES - 1)
L = 150
LD = 329
NA, NB, NC, ND = 4096, 2048, 64, 1100
SHORT = [0, 1, 29, 30, 31]
NAT, NBT = 512, 256
RULES = [(0, 0), (2, 25)]
QS = (0, 20)
SEED = 20260


def random_canonical_keys(rng, n, k=K):
    """read_support_cases.random_keys(rng, n) for all n at once: the same draws, the same keys"""
    c = np.searchsorted(ACGT, rng.choice(ACGT, n * k)).reshape(n, k).astype(np.uint64)
    kf = np.zeros(n, np.uint64)
    kr = np.zeros(n, np.uint64)
    for j in range(k):
        kf = (kf << np.uint64(2)) | c[:, j]
        kr = (kr << np.uint64(2)) | (np.uint64(3) - c[:, k - 1 - j])
    return np.minimum(kf, kr)


def revcomp_keys(keys, k=K):
    keys = np.asarray(keys, np.uint64)
    r = np.zeros(keys.size, np.uint64)
    for i in range(k):
        r = (r << np.uint64(2)) | (np.uint64(3) - ((keys >> np.uint64(2 * i)) & np.uint64(3)))
    return r


def key_bases(key, k=K):
    """the k bases of a key as uint8"""
    return ACGT[[(int(key) >> (2 * (k - 1 - i))) & 3 for i in range(k)]]


def revcomp(seq):
    return COMP[np.asarray(seq, np.uint8)[::-1]]


def gather(seqs):
    bases = np.concatenate(seqs) if seqs else np.empty(0, np.uint8)
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([s.size for s in seqs])
    return np.ascontiguousarray(bases, np.uint8), off


def csr_take(offsets, ids):
    """indices into a CSR's value arrays of the rows `ids` (repeats allowed), and the rows' lengths"""
    ids = np.asarray(ids, np.int64)
    a = offsets[ids].astype(np.int64)
    n = offsets[ids + 1].astype(np.int64) - a
    first = np.cumsum(n) - n
    return np.repeat(a - first, n) + np.arange(int(n.sum())), n


class World:
    pass


def _database(w, rng):
    parent, _ = synth.load_taxonomy("bact10")
    keys = random_canonical_keys(rng, N_ENTRIES)
    targets = rng.integers(2, parent.size, N_ENTRIES).astype(np.uint32)
    genomes, gk, gt = genome_db(parent, N_GENOMES, GENOME_LEN, rng)
    assert gk.size == G1 - G0
    canon = gk < revcomp_keys(gk)
    # two neighbouring canonical windows of one genome, far enough from its ends for a read around them
    j = next(j for j in range(51000, gk.size - 1)
             if canon[j] and canon[j + 1] and 300 <= j % GENOME_WIN < GENOME_WIN - 300 and gt[j] > 1 and gt[j + 1] > 1)
    roll = j - (PIECE - 1 - G0)
    keys[G0:G1] = np.roll(gk, -roll)
    targets[G0:G1] = np.roll(gt, -roll)
    assert keys[PIECE - 1] == gk[j] and keys[PIECE] == gk[j + 1]
    w.boundary_genome, w.boundary_window = j // GENOME_WIN, j % GENOME_WIN
    w.root_entries = np.sort(rng.choice(np.arange(1000, G0 - 1000), 12, replace=False))
    targets[w.root_entries] = 1
    src = np.concatenate([[0, PIECE, PIECE - 1, 32], rng.choice(np.arange(100, G0), 8, replace=False),
                          rng.choice(np.arange(G0, G1), 8, replace=False)])
    keys[DUPS] = keys[src]
    targets[DUPS] = (targets[src] - 2 + 7) % (parent.size - 2) + 2
    w.dup_sources = src
    assert np.unique(keys).size == N_ENTRIES - DUPS.size, "a seed whose keys collide: take another"
    assert all(targets[o] > 1 for o in PLANTED) and N_ENTRIES % 128 == 33
    w.parent, w.keys, w.targets, w.genomes = parent, keys, targets, genomes
    w.ntar = parent.size
    w.odb = oracle_db(parent, keys, targets, LOG2_SLOTS)
    w.hm = HitModel(w.odb, keys, targets, K)
    w.sm = SupportModel(w.hm, parent)
    first = np.zeros(N_ENTRIES, bool)
    first[w.hm.first] = True
    w.valid_bits = np.flatnonzero(first & (targets > 1))  # the bits a hit can set
    assert not first[DUPS].any() and all(first[o] for o in PLANTED)


def _implant(read, at, key, flip):
    b = key_bases(key)
    read[at:at + K] = revcomp(b) if flip else b


def _reads(w, rng):
    keys = w.keys
    a = rng.choice(ACGT, (NA, L))
    with_hit = np.flatnonzero(rng.random(NA) < 0.5)
    # (no genome k-mers in A: the windows beside one share its minimizer, whose table line is full -- and every lookup on
    #  a full line asks for a place in the hit log, as a hit does; A has to stay well below the 8 places per read at which
    #  a pass switches the log off: about 5 % of this table's lines are full, 6 of a random read's 121 lookups.)
    outside = np.concatenate([np.arange(0, G0), np.arange(G1, N_ENTRIES)])
    for i, r in enumerate(with_hit):
        for at in (5, 45)[:int(rng.integers(1, 3))]:
            o = int(w.root_entries[i % 12]) if i % 37 == 0 and at == 5 else int(rng.choice(outside))
            _implant(a[r], at, keys[o], rng.random() < 0.5)
    b = np.empty((NB, L), np.uint8)
    gi = rng.integers(0, N_GENOMES, NB)
    pos = rng.integers(0, GENOME_LEN - L + 1, NB)
    gi[70:80] = w.boundary_genome
    pos[70:80] = w.boundary_window - 60 + 5 * np.arange(10)  # windows pos .. pos + 120 hold both boundary windows
    for r in range(NB):
        s = w.genomes[gi[r]][pos[r]:pos[r] + L]
        b[r] = revcomp(s) if r % 2 else s
    c = rng.choice(ACGT, (NC, L))
    w.c_planted = []
    for r in range(NC):
        which = [PLANTED[r % 8]] + ([PLANTED[(r // 8 + r) % 8]] if r >= 8 else []) + ([PLANTED[(r // 4 + 3) % 8]] if r >= 32 else [])
        for at, o in zip((5, 45, 85), which):
            _implant(c[r], at, keys[o], (r + at) % 2 == 1)
        w.c_planted.append(which)
    live = np.setdiff1d(w.valid_bits, np.arange(G0, G1))  # random keys of random, unrelated targets
    d = rng.choice(ACGT, (ND, LD))
    for r in range(ND):
        for at in (20, 150, 280)[:1 + r % 3]:
            _implant(d[r], at, keys[int(rng.choice(live))], rng.random() < 0.5)
    short = [rng.choice(ACGT, n) for n in SHORT]
    short[3][:] = key_bases(keys[int(live[5])])
    _implant(short[4], 1, keys[int(live[6])], True)
    seqs = list(a) + list(b) + list(c) + list(d) + short + list(a[:NAT]) + list(b[:NBT])
    w.A = np.arange(0, NA)
    w.B = np.arange(NA, NA + NB)
    w.C = np.arange(NA + NB, NA + NB + NC)
    w.D = np.arange(w.C[-1] + 1, w.C[-1] + 1 + ND)
    w.S = np.arange(w.D[-1] + 1, w.D[-1] + 1 + len(SHORT))
    w.AT = np.arange(w.S[-1] + 1, w.S[-1] + 1 + NAT)
    w.BT = np.arange(w.AT[-1] + 1, w.AT[-1] + 1 + NBT)
    w.n_fixed = NA + NB + NC  # the reads [0, n_fixed) lie back to back, L bases each
    w.n_pool = len(seqs)
    w.bases, w.off = gather(seqs)
    lens = np.diff(w.off.astype(np.int64))
    w.start = np.zeros(w.n_pool, np.int32)
    w.stop = (lens - 1).astype(np.int32)
    q = np.concatenate([synth.qualities(NAT, L, r0=11), synth.qualities(NBT, L, r0=22)])
    st, sp, keep = trim_ranges([x.tobytes() for x in q], np.full(NAT + NBT, L), K)
    odd = ~((st > sp) | ((st >= 0) & (sp < L)))  # a range the library would refuse: the reference never hands it on either
    st[odd], sp[odd] = 0, -1
    w.start[w.AT[0]:], w.stop[w.AT[0]:] = st, sp
    w.trim_keep = keep


def _facts(w):
    os_ = ob.OracleSample(w.odb)
    w.final = os_.classify(w.bases, w.off, w.start, w.stop)
    w.pool_counts, w.pool_stats = os_.counts(), os_.stats()
    os_.close()
    w.hits = w.hm.batch(w.bases, w.off, w.start, w.stop)
    w.n_kmers = w.hits.n_kmers.astype(np.int64)
    w.rec = {rule: w.sm.batch_identity(w.hits, rule, w.final) for rule in RULES}
    w.final_reversed_D = np.array([w.hm.fold(w.hits.of(r)[1][::-1]) for r in w.D], np.uint32)


def _block(w, seqs, quals):
    """a FASTQ block and its facts under the two qualities -> {"text", "recs", "n", q: {...}}"""
    text, recs = fastq_block([s.tobytes() for s in seqs], [x.tobytes() for x in quals])
    n = len(seqs)
    lens = np.array([s.size for s in seqs])
    start, stop, keep = trim_ranges([x.tobytes() for x in quals], lens, K)
    blk = {"text": text, "recs": recs, "n": n, "start": start, "stop": stop, "keep": keep}
    kept = np.flatnonzero(keep)
    for q in QS:
        masked, n_masked = [], 0
        for s, x in zip(seqs, quals):
            m = x.view(np.int8) < q + 33 if q else np.zeros(s.size, bool)
            t = s.copy()
            t[m] = ord("N")
            masked.append(t)
            n_masked += int(m.sum())
        bases, off = gather([masked[i] for i in kept])
        os_ = ob.OracleSample(w.odb)
        fk = os_.classify(bases, off, start[kept], stop[kept])
        os_.close()
        hk = w.hm.batch(bases, off, start[kept], stop[kept])
        final = np.zeros(n, np.uint32)
        final[kept] = fk
        blk[q] = {"final": final, "final_kept": fk, "hits": hk, "masked": n_masked}
    return blk


def _blocks(w):
    w.blocks = []
    for ids, r0 in ((w.A[0:300], 100), (w.B[0:200], 200), (w.A[2000:2300], 300), (w.B[1000:1200], 400)):
        seqs = [w.bases[int(w.off[i]):int(w.off[i + 1])] for i in ids]
        w.blocks.append(_block(w, seqs, list(synth.qualities(len(ids), L, r0=r0))))
    seqs = [w.bases[int(w.off[i]):int(w.off[i + 1])] for i in w.D[:20]]
    w.blocks.append(_block(w, seqs, [np.full(LD, ord("I"), np.uint8)] * 20))
    w.long_block = len(w.blocks) - 1


@functools.lru_cache(maxsize=None)
def world(seed=SEED):
    w = World()
    w.seed = seed
    rng = np.random.default_rng(seed)
    _database(w, rng)
    _reads(w, rng)
    _facts(w)
    _blocks(w)
    w.seen_bytes = (N_ENTRIES + 127) // 128 * 16  # one bit per entry, whole 16-byte groups
    return w


def batch_of(w, ids, ranges=False):
    """the reads `ids` of the pool as a batch -> (bases, offsets, start, stop); start = stop = None unless ranges"""
    ids = np.asarray(ids, np.int64)
    idx, n = csr_take(w.off, ids)
    off = np.zeros(ids.size + 1, np.uint64)
    off[1:] = np.cumsum(n)
    bases = np.ascontiguousarray(w.bases[idx])
    if not ranges:
        return bases, off, None, None
    return bases, off, np.ascontiguousarray(w.start[ids]), np.ascontiguousarray(w.stop[ids])


class SampleMirror:
    """what a kid_sample holds after the same calls: gcount, the seen bits, the depth counters and the statistics (reads:
    the reads and records handed to the classify calls; lookups and hits: the oracle's)"""

    def __init__(self, w):
        self.w = w
        self.reset()

    def reset(self):
        w = self.w
        self.gcount = np.zeros(w.ntar, np.int64)
        self.seen = np.zeros(N_ENTRIES, bool)
        self.depth = np.zeros(N_ENTRIES, np.uint32)
        self.reads = self.lookups = self.hits = self.masked = 0

    def _classified(self, final, n_kmers, target, entry):
        self.gcount += np.bincount(final.astype(np.int64), minlength=self.w.ntar)
        self.seen[entry[target > 1]] = True
        self.reads += int(final.size)
        self.lookups += int(n_kmers.sum())
        self.hits += int(target.size)

    def classify(self, read_ids):
        """-> the finals of the reads"""
        w = self.w
        ids = np.asarray(read_ids, np.int64)
        idx, _ = csr_take(w.hits.offsets, ids)
        self._classified(w.final[ids], w.n_kmers[ids], w.hits.target[idx], w.hits.entry[idx])
        return w.final[ids]

    def classify_fastq(self, block, q):
        """-> (final, start, stop) of the block's records; a dropped record is counted nowhere"""
        b = self.w.blocks[block]
        f = b[q]
        self._classified(f["final_kept"], f["hits"].n_kmers.astype(np.int64), f["hits"].target, f["hits"].entry)
        self.reads += b["n"] - int(b["keep"].sum())  # (kid_sample_stats counts the records handed in; gcount does not see a dropped one)
        self.masked += f["masked"]
        return f["final"], b["start"], b["stop"]

    def tally(self, read_ids, rule):
        """the reads counted as kid_db_read_support(..., tally) counts them -> their support records"""
        w = self.w
        ids = np.asarray(read_ids, np.int64)
        idx, n = csr_take(w.hits.offsets, ids)
        off = np.zeros(ids.size + 1, np.uint64)
        off[1:] = np.cumsum(n)
        sub = Hits(off, w.hits.n_kmers[ids], w.hits.pos[idx], w.hits.target[idx], w.hits.entry[idx])
        rec = w.rec[rule][ids]
        counted = np.ones(ids.size, bool)
        g, u = w.sm.tally(sub, rec, counted, w.targets)
        d = depth_of(sub, rec, counted, N_ENTRIES)
        assert np.array_equal(u, np.bincount(w.targets[d > 0].astype(np.int64), minlength=w.ntar))  # the two models agree
        self.gcount += g
        self.seen |= d > 0
        self.depth = saturating_add(self.depth, d)
        return rec

    def seen_or(self, bits):
        self.seen[np.asarray(bits, np.int64)] = True

    def ucount(self, bit_begin=0, bit_end=None):
        """the first-insert targets of the set bits in [bit_begin, bit_end)"""
        o = np.flatnonzero(self.seen[bit_begin:bit_end]) + bit_begin
        return np.bincount(self.w.targets[o].astype(np.int64), minlength=self.w.ntar).astype(np.int64)

    def bitmap_bytes(self):
        out = np.zeros(self.w.seen_bytes, np.uint8)
        packed = np.packbits(self.seen, bitorder="little")
        out[:packed.size] = packed
        return out

    def stats(self):
        return {"reads": self.reads, "lookups": self.lookups, "hits": self.hits}
