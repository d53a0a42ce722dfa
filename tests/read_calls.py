"""What the tests of the call families over the hit pass share (kid_db_read_support*, _fragments*, _votes*,
_fragment_votes*, _segments*, _segment_votes*, and the tests of depth, the call mix and the synthetic hit lists beside
them): the comparisons with a model's records, small probes of a sample and of an error status, the constants of a
kernel header, the base of a test's World, the genome worlds and the paired FASTQ blocks.  A plain module: no fixture,
no mark, no test."""
import os
import re

import numpy as np
import pytest

import read_support_cases as sc
from base_quality_cases import np_mask
from helpers import ROOT, concat_reads, fastq_block, oracle_db
from kmer_id_amd import KID_FLAG_HOST_BUILD, KID_FLAG_REF_GEOMETRY, KidError, KmerDB
from read_fragments_model import interleave
from read_hits_model import HitModel, trim_ranges, windows
from read_support_model import SupportModel

KINDS = {"minloc": 0, "ref_geometry": KID_FLAG_REF_GEOMETRY, "host_build": KID_FLAG_HOST_BUILD}
RC_SETTINGS = [(100, 50), (500, 250), (2000, 2000)]
COMPLEMENT = bytes.maketrans(b"ACGTN", b"TGCAN")


def header_constant(header, name):
    """-> the value of `#define name <digits>u` in kmer_id_amd/csrc/<header>"""
    text = open(os.path.join(ROOT, "kmer_id_amd", "csrc", header)).read()
    return int(re.search(r"#define\s+%s\s+(\d+)u" % name, text).group(1))


def same_records(got, exp, dtype, what=""):
    """got: the records of a call (every field a uint32); exp: the model's"""
    assert got.dtype == dtype and got.dtype.itemsize == 4 * len(dtype.names) and got.shape == exp.shape, what
    for f in dtype.names:
        bad = np.flatnonzero(got[f] != exp[f])
        assert bad.size == 0, "%s: record %d: %s: got %s, the model %s" % (what, int(bad[0]), f, got[bad[0]], exp[bad[0]])


def same_segments(got, exp, dtype, what=""):
    """got: ReadSegments; exp: (offsets, records) of the model"""
    assert got.offsets.dtype == np.uint64 and np.array_equal(got.offsets, exp[0]), what
    assert got.records.dtype == dtype and got.records.shape == exp[1].shape, what
    for f in dtype.names:
        bad = np.flatnonzero(got.records[f] != exp[1][f])
        assert bad.size == 0, "%s: segment %d: %s: got %s, the model %s" % (what, int(bad[0]), f, got.records[bad[0]], exp[1][bad[0]])


def ends_equal(a, b):
    """two (gcount, ucount) pairs"""
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def status(f):
    """-> the status of the KidError that f() must raise"""
    with pytest.raises(KidError) as e:
        f()
    return e.value.status


def seen_bits(s, n_entries):
    return np.unpackbits(s.seen_export(0, s.seen_bytes()), bitorder="little")[:n_entries].astype(bool)


class World:
    """what every family's World starts from: a database's entries, a batch of reads, the oracle's table and the hit and
    support models over it; db(flags) builds the database"""

    def __init__(self, parent, keys, targets, bases, off, log2_slots):
        self.parent, self.keys, self.targets, self.bases, self.off, self.log2_slots = parent, keys, targets, bases, off, log2_slots
        self.odb = oracle_db(parent, keys, targets, log2_slots)
        self.hm = HitModel(self.odb, keys, targets, 30)
        self.sm = SupportModel(self.hm, parent)

    def db(self, flags=0):
        return KmerDB(self.keys, self.targets, self.parent, k=30, log2_slots=self.log2_slots, flags=flags)


def genome_world(rng, lineage, genome_len, every):
    """a database of every `every`-th window of a random genome under targets drawn from `lineage`; a read that is a
    stretch of the genome has a run of consecutive database k-mers"""
    g = rng.choice(sc.ACGT, genome_len).tobytes()
    keys, _ = windows(g, 0, genome_len - 1, 30)
    keys = keys[::every]
    tg = np.array(lineage, np.uint32)[rng.integers(0, len(lineage), keys.size)]
    return g, keys, tg


def revcomp(seq):
    return bytes(seq).translate(COMPLEMENT)[::-1]


def strand_world(parent, targets_of_world, rng=None):
    """the 2029-base genome world: every window of a random genome under targets drawn from [8, 6, 5, 36, 35, 8, 6, X]
    (X on another lineage), the genome as one record (P = 2000) and its reverse complement as a second
    -> keys, targets, bases, offsets"""
    rng = rng or np.random.default_rng(2029)
    x = next(int(t) for t in targets_of_world if t > 1 and sc.top_level(parent, int(t)) != 5)
    g = rng.choice(sc.ACGT, 2029).tobytes()
    keys, _ = windows(g, 0, len(g) - 1, 30)
    tg = np.array([8, 6, 5, 36, 35, 8, 6, x], np.uint32)[rng.integers(0, 8, keys.size)]
    bases, off = concat_reads([g, revcomp(g)])
    return keys, tg, bases, off


def mirrored(off, rec, what=""):
    """the records of read 0 against those of read 1, its reverse complement: segment j is segment n_seg - 1 - j there"""
    a, b = rec[int(off[0]):int(off[1])], rec[int(off[1]):int(off[2])][::-1]
    assert a.size == b.size and a.size > 0, what
    assert np.array_equal(a["n_pos"], b["n_pos"]), what
    P = int(a["pos"][-1] + a["n_pos"][-1])  # (start = 0)
    assert np.array_equal(a["pos"].astype(np.int64), P - b["pos"].astype(np.int64) - b["n_pos"].astype(np.int64)), what
    return a, b


def fastq_world(world):
    """world: a World over read_fragments_cases.fragments, with its `where` and `cum`.
    Two blocks of n + 5 and n + 9 records: fragment i is record 5 + i of block 1 and record 9 + i of block 2"""
    from kmer_id_amd import synth
    n, length = 400, 150
    bases, _ = sc.cases.synth_reads(world.cum, world.parent, 2 * n + 14, length)
    quals = [q.tobytes() for q in synth.qualities(2 * n + 14, length)]
    seqs = [bases[i * length:(i + 1) * length].tobytes() for i in range(2 * n + 14)]
    s1, q1, s2, q2 = seqs[:n + 5], quals[:n + 5], seqs[n + 5:], quals[n + 5:]
    raw = bytes(world.bases)
    for j, name in enumerate(sorted(world.where)):  # the hand-built fragments, qualities that trim nothing
        f = world.where[name]
        a, b = raw[int(world.off[2 * f]):int(world.off[2 * f + 1])], raw[int(world.off[2 * f + 1]):int(world.off[2 * f + 2])]
        s1[5 + 20 + j], q1[5 + 20 + j], s2[9 + 20 + j], q2[9 + 20 + j] = a, b"I" * len(a), b, b"I" * len(b)
    for i in range(0, 60, 3):  # dropped by quality: mate 1 only, mate 2 only, both
        q1[5 + 100 + i] = b"!" * length
        q2[9 + 100 + i + 1] = b"!" * length
        q1[5 + 100 + i + 2] = q2[9 + 100 + i + 2] = b"!" * length
    s2[9 + 200], q2[9 + 200] = b"", b""  # an absent mate (its lines are empty)
    for i in range(210, 230):  # low-quality bases inside reads that are kept: KID_DB_OPT_MIN_BASE_QUALITY changes their hits
        for q in (q1, q2):
            row = bytearray(q[9 + i])
            row[40:44] = b"++++"
            row[90] = ord("2")
            q[9 + i] = bytes(row)
    t1, r1 = fastq_block(s1, q1, eol=b"\r\n", blank_every=5)
    t2, r2 = fastq_block(s2, q2, eol=b"\n", blank_every=3)
    return n, (s1[5:], q1[5:], t1, r1), (s2[9:], q2[9:], t2, r2)


def fastq_model(world, mate1, mate2, q):
    """-> (hits of the 2 n interleaved reads under their trimmed ranges, counted)"""
    per = []
    for seqs, quals in (mate1, mate2):
        start, stop, keep = trim_ranges(quals, [len(s) for s in seqs], 30)
        start[~keep], stop[~keep] = 0, -1  # a dropped mate contributes no hit and no window
        if q:
            seqs = [np_mask(np.frombuffer(s, np.uint8), np.frombuffer(ql, np.uint8)[:len(s)], q)[0].tobytes() if k else s
                    for s, ql, k in zip(seqs, quals, keep)]
        per.append((seqs, start, stop, keep))
    bases, off = concat_reads(interleave(per[0][0], per[1][0]))
    start, stop = np.zeros(off.size - 1, np.int32), np.zeros(off.size - 1, np.int32)
    start[0::2], start[1::2], stop[0::2], stop[1::2] = per[0][1], per[1][1], per[0][2], per[1][2]
    return world.hm.batch(bases, off, start, stop), per[0][3], per[1][3]
