"""What the sample-close, dense-ucount and kernel-times tests share: bact10-synth at scale 1e-4 in a table of
2^18 cells, 4096 reads of 150 bases from synth.reads, and the oracle's answers for them, computed once per process."""
import functools

import numpy as np

from kmer_id_amd import KmerDB, synth
from oracle import binding as ob

K, LOG2_SLOTS, N_READS, READ_LEN = 30, 18, 4096, 150


@functools.lru_cache(maxsize=None)
def world():
    parent, cnt = synth.load_taxonomy("bact10")
    cum = synth.cumulative(synth.scaled_counts(cnt, 1e-4))
    keys, targets = synth.db_keys(cum)
    bases = synth.reads(cum, parent, N_READS, READ_LEN)
    off = synth.fixed_offsets(N_READS, READ_LEN)
    for a in (parent, keys, targets, bases, off):
        a.setflags(write=False)
    return parent, keys, targets, bases, off


def new_db(parent=None, keys=None, targets=None):
    p, k, t, _, _ = world()
    return KmerDB(k if keys is None else keys, t if targets is None else targets, p if parent is None else parent, k=K,
                  log2_slots=LOG2_SLOTS, device=0)


class Oracle:
    """the oracle's sample over the same database (or over another one of the same shape)"""

    def __init__(self, parent=None, keys=None, targets=None):
        p, k, t, _, _ = world()
        parent = p if parent is None else parent
        self.db = ob.OracleDB(parent.size, K, LOG2_SLOTS, parent=parent)
        self.db.add(k if keys is None else keys, t if targets is None else targets)
        self.s = ob.OracleSample(self.db)

    def classify(self, bases, off, start=None, stop=None):
        return self.s.classify(bases, off, start, stop)

    def counts(self):
        return self.s.counts()

    def reset(self):
        self.s.reset()


@functools.lru_cache(maxsize=None)
def expected(times=1):
    """-> (finals, gcount, ucount) of the oracle after the 4096 reads were classified `times` times into one sample"""
    _, _, _, bases, off = world()
    o = Oracle()
    for _ in range(times):
        finals = o.classify(bases, off)
    g, u = o.counts()
    for a in (finals, g, u):
        a.setflags(write=False)
    return finals, g, u


def same(got, exp):
    return all(np.array_equal(np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)) for a, b in zip(got, exp))


def key_reads(n_reads, keys_per_read):
    """reads made of the database's own keys back to back: every one of them hits at least keys_per_read times"""
    _, keys, _, _, _ = world()
    rng = np.random.default_rng(7)
    pick = keys[rng.integers(0, keys.size, n_reads * keys_per_read)]
    text = "".join(synth.key_to_seq(int(k), K) for k in pick)
    bases = np.frombuffer(text.encode(), np.uint8).copy()
    return bases, synth.fixed_offsets(n_reads, keys_per_read * K)
