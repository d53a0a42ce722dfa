"""Shared helpers for the test-suite (imports the oracle: test infrastructure)."""
import ctypes as C
import gzip
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from kmer_id_amd import _lib, synth  # noqa: E402
from oracle import binding as ob  # noqa: E402

K = 30


def unpack_strings(data, off):
    raw = bytes(data)
    off = [int(x) for x in off]
    return [raw[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def parse_probes_text(text, k=K):
    """Host restatement (numpy-free, tiny inputs) of process_kmergz + process_kmer for tests that
    need the (key, target) list in file order; the C oracle has its own parser, this one is
    only used to hand the SAME entries to kid_db_build."""
    keys, targets = [], []
    parts = text.split(b"\n")
    lines = parts[:-1]  # the unterminated tail is dropped (newkmer_10nx.cpp:705-709)
    for line in lines:
        if line.endswith(b"\r"):
            line = line[:-1]
        if not line:
            continue
        f = line.replace(b",", b" ").split()
        if len(f) < 6:
            continue
        try:
            t = int(f[1]); int(f[2]); int(f[3]); int(f[5])
        except ValueError:
            continue
        if t < 0:
            continue
        cpos, key = 0, 0
        for ch in f[0]:
            c = {65: 0, 67: 1, 71: 2, 84: 3}.get(ch, -1)
            if c < 0:
                cpos, key = 0, 0
            else:
                key = ((key << 2) & ((1 << (2 * k)) - 1)) | c
                cpos += 1
            if cpos == k:
                keys.append(key)
                targets.append(t)
                cpos -= 1
    return np.array(keys, np.uint64), np.array(targets, np.uint32)


def small_db(scale, name="bact10", k=K, seed=synth.DB_SEED):
    parent, cnt = synth.load_taxonomy(name)
    cum = synth.cumulative(synth.scaled_counts(cnt, scale))
    keys, targets = synth.db_keys(cum, k, seed=seed)
    return parent, cum, keys, targets


def oracle_db(parent, keys, targets, log2_slots, k=K, max_probes=0, flags=0):
    db = ob.OracleDB(parent.size, k, log2_slots, max_probes, flags, parent=parent)
    db.add(keys, targets)
    return db


def concat_reads(seqs):
    data = np.frombuffer(b"".join(seqs), np.uint8).copy()
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return data, off


def fastq_block(seqs, quals, eol=b"\n", blank_every=0):
    """FASTQ text of the records (seqs[i], quals[i]: bytes) -> (text uint8[], recs uint32[n, 4]: seq_off, seq_len,
    qual_off, qual_len; the lines without their line end).  eol: the line end; blank_every: a blank line (and a bare
    '\\n') behind every blank_every-th record, the first included"""
    text, recs = bytearray(), []
    for i, (s, q) in enumerate(zip(seqs, quals)):
        text += b"@r%d" % i + eol
        so = len(text)
        text += s + eol + b"+" + eol
        qo = len(text)
        text += q + eol
        if blank_every and i % blank_every == 0:
            text += eol + b"\n"
        recs.append((so, len(s), qo, len(q)))
    return np.frombuffer(bytes(text), np.uint8), np.array(recs, np.uint32)


class DeviceBatch:
    """a batch resident in HBM with the output buffers of kid_db_read_hits_device (hits: a canary-filled kid_hit[cap + 4])"""

    def __init__(self, bases, off, cap):
        self.lib = _lib.load()
        self.n, self.nbytes, self.bufs = off.size - 1, bases.size, []
        padded = np.zeros(((bases.size + 15) // 16) * 16 + 32, np.uint8)
        padded[:bases.size] = bases
        self.canary = np.full((cap + 4) * 3, 0xA5A5A5A5, np.uint32)
        self.d_bases, self.d_off = self.dev(padded.nbytes, padded), self.dev(off.nbytes, off)
        self.d_ho, self.d_nk, self.d_tot = self.dev((self.n + 1) * 8), self.dev(max(self.n, 1) * 4), self.dev(8)
        self.d_hits = self.dev(self.canary.nbytes, self.canary)

    def dev(self, nbytes, src=None):
        p = C.c_void_p()
        _lib.check(self.lib.kid_dev_alloc(0, nbytes, C.byref(p)))
        self.bufs.append(p)
        if src is not None:
            _lib.check(self.lib.kid_dev_upload(0, p, src.ctypes.data_as(C.c_void_p), src.nbytes))
        return p

    def down(self, p, dtype, count):
        out = np.empty(count, dtype)
        _lib.check(self.lib.kid_dev_download(0, out.ctypes.data_as(C.c_void_p), p, out.nbytes))
        return out

    def run(self, db, cap, nbytes=None):
        db.read_hits_device(self.d_bases.value, self.nbytes if nbytes is None else nbytes, self.d_off.value, self.n, self.d_ho.value,
                            self.d_tot.value, d_n_kmers=self.d_nk.value, d_hits=self.d_hits.value if cap else 0, cap=cap)
        _lib.check(self.lib.kid_dev_sync(0))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.bufs:
            self.lib.kid_dev_free(0, p)


class DeviceCsr(DeviceBatch):
    """a hit CSR of the caller's making resident in HBM, as the *_from_hits_device calls take it: offsets uint64[n + 1],
    hits uint32[total, 3] (kid_hit: pos, target, entry), n_kmers uint32[n]; and canary-filled outputs with GUARD records of
    canary behind the last one"""
    CANARY, GUARD = 0xA5A5A5A5, 2

    def __init__(self, offsets, hits, n_kmers):
        self.lib = _lib.load()
        self.n, self.bufs = offsets.size - 1, []
        offsets, n_kmers = np.ascontiguousarray(offsets, np.uint64), np.ascontiguousarray(n_kmers, np.uint32)
        hits = np.ascontiguousarray(hits, np.uint32)
        assert hits.shape == (int(offsets[-1]), 3) and n_kmers.size == self.n and np.all(np.diff(offsets.astype(np.int64)) >= 0)
        self.d_ho, self.d_nk, self.d_hits = self.dev(offsets.nbytes, offsets), self.dev(max(self.n, 1) * 4, n_kmers), self.dev(max(hits.nbytes, 16), hits)

    def out(self, n_records, dtype):
        """a buffer of n_records + GUARD records of `dtype`, every word the canary"""
        canary = np.full((n_records + self.GUARD) * dtype.itemsize // 4, self.CANARY, np.uint32)
        return self.dev(canary.nbytes, canary)

    def records(self, d_out, n_records, dtype):
        """-> the n_records records; the guard behind them must be untouched"""
        words = self.down(d_out, np.uint32, (n_records + self.GUARD) * dtype.itemsize // 4)
        assert np.all(words[n_records * dtype.itemsize // 4:] == self.CANARY), "a write behind the last record"
        return words[:n_records * dtype.itemsize // 4].view(dtype)
