"""Seeded inputs shared by the read-votes tests (CPU model test and GPU tests): the database and the reads of
tests/read_support_cases.py plus hand-built reads for the worked cases of the vote rule, nothing else."""
import numpy as np

import read_support_cases as sc

K = sc.K


def hand_built(parent, keys, targets, rng):
    """reads whose hits have chosen targets on 5 -> 6 -> 8, 5 -> 35 -> 36 and a node X of another top-level lineage
    -> {name: read}, X"""
    first = np.unique(keys, return_index=True)[1]
    x = next(int(t) for t in targets[np.sort(first)] if t > 1 and sc.top_level(parent, int(t)) != 5)
    ks = lambda t, j=0: sc.cases.key_seq(sc.key_of(keys, targets, t, j), K)  # noqa: E731
    return {
        "v_8_36": sc.implanted(rng, [ks(8), ks(36)]),                              # a tie at an inner node: call 5, n_best 2
        "v_X_8": sc.implanted(rng, [ks(x), ks(8)]),                                # a tie at the root: call 1
        "v_1_X": sc.implanted(rng, [ks(1), ks(x)]),                                # a root hit counts for X: call X, p_best 2
        "v_8_8_36_36_X": sc.implanted(rng, [ks(8), ks(8), ks(36), ks(36, 1), ks(x)]),  # L = {8, 36}: call 5; the fold ends at 1
        "v_6_8_36": sc.implanted(rng, [ks(6), ks(8), ks(36)]),                     # unique best 8 (P = 2): call 8; the fold says 5
    }, x


def reads(parent, cum, keys, targets):
    """read_support_cases.reads() + the hand-built ones above -> bases, offsets, {name: read index}, X"""
    from helpers import concat_reads
    b, o, where = sc.reads(parent, cum, keys, targets)
    raw = bytes(b)
    seqs = [raw[int(o[i]):int(o[i + 1])] for i in range(o.size - 1)]
    hb, x = hand_built(parent, keys, targets, np.random.default_rng(78))
    where = dict(where)
    for name, s in hb.items():
        where[name] = len(seqs)
        seqs.append(s)
    bases, off = concat_reads(seqs)
    return bases, off, where, x


def reversed_hits(hits):
    """the same Hits with every read's hits in opposite order: what the reverse complement of the read gives"""
    from read_hits_model import Hits
    idx = np.concatenate([np.arange(int(hits.offsets[r + 1]) - 1, int(hits.offsets[r]) - 1, -1) for r in range(hits.offsets.size - 1)]
                         + [np.empty(0, np.int64)]).astype(np.int64)
    return Hits(hits.offsets, hits.n_kmers, hits.pos[idx], hits.target[idx], hits.entry[idx])


def reverse_complement(bases, off):
    """every read of the batch reverse-complemented in place (a byte that is not ACGTacgt stays what it is)"""
    comp = np.arange(256, dtype=np.uint8)
    for a, b in zip(b"ACGTacgt", b"TGCAtgca"):
        comp[a] = b
    out = np.asarray(bases, np.uint8).copy()
    for r in range(off.size - 1):
        a, b = int(off[r]), int(off[r + 1])
        out[a:b] = comp[out[a:b]][::-1]
    return out
