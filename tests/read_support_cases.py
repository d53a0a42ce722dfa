"""Seeded inputs shared by the read-support tests (CPU model test and GPU tests): databases and reads, nothing else."""
import numpy as np

import read_hits_cases as cases
from helpers import concat_reads

ACGT = np.frombuffer(b"ACGT", np.uint8)
K = 30


def random_keys(rng, n, k=K):
    """n canonical k-mers of random bases (as likely to collide with a seeded database as two of its own keys)"""
    from read_hits_model import windows
    seq = rng.choice(ACGT, n * k).tobytes()
    return np.array([windows(seq[i * k:(i + 1) * k], 0, k - 1, k)[0][0] for i in range(n)], np.uint64)


def database():
    """read_hits_cases.database(k=30, scale=2e-4, dup=True) with a few entries appended that the hand-built reads need and
    the scaled database lacks: keys of target 1 (the root), and three more under each of 5, 35 and 6.
    -> parent, cum, keys, targets"""
    parent, cum, keys, targets = cases.database(K, 2e-4, dup=True)
    rng = np.random.default_rng(1234)
    extra_t = np.array([1] * 6 + [5] * 3 + [35] * 3 + [6] * 3, np.uint32)
    extra_k = random_keys(rng, extra_t.size)
    return parent, cum, np.concatenate([keys, extra_k]), np.concatenate([targets, extra_t])


def key_of(keys, targets, t, j=0):
    """the j-th database key whose FIRST insert has target t"""
    first = np.unique(keys, return_index=True)[1]
    idx = np.sort(first[targets[first] == t])
    return keys[idx[j]]


def implanted(rng, kmers, gap=7):
    """a read of random bases with the given k-mers (bytes) implanted in order, `gap` random bases apart"""
    parts = []
    for km in kmers:
        parts.append(rng.choice(ACGT, gap).tobytes())
        parts.append(km)
    parts.append(rng.choice(ACGT, gap).tobytes())
    return b"".join(parts)


def top_level(parent, t):
    """the child of the root on t's root path"""
    while parent[t] != 1:
        t = int(parent[t])
    return t


def hand_built(parent, keys, targets, rng):
    """reads whose hits have chosen targets, for nodes 5 -> 6 -> 8, 5 -> 35 -> 36 and a node X of another top-level lineage
    -> {name: read}"""
    assert parent[8] == 6 and parent[6] == 5 and parent[36] == 35 and parent[35] == 5 and parent[5] == 1
    first = np.unique(keys, return_index=True)[1]
    x = next(int(t) for t in targets[np.sort(first)] if t > 1 and top_level(parent, int(t)) != 5)
    ks = lambda t, j=0: cases.key_seq(key_of(keys, targets, t, j), K)  # noqa: E731
    return {
        "6_36_8": implanted(rng, [ks(6), ks(36), ks(8)]),        # final 8, confident 5 at min_hits 3
        "X_8_6": implanted(rng, [ks(x), ks(8), ks(6)]),          # final 6, confident 1 at min_hits 3
        "root_only": implanted(rng, [ks(1, 0), ks(1, 1), ks(1, 2)]),
        "6_8": implanted(rng, [ks(6), ks(8)]),                   # the header's example: final 8, S(8) = 1, S(6) = 2
        "36_36_35_5": implanted(rng, [ks(36), ks(36, 1), ks(35), ks(5)]),
    }


def reads(parent, cum, keys, targets):
    """adversarial_reads(n=600) + 2000 synthetic 150-bp reads + the hand-built ones -> bases, offsets, {name: read index}"""
    b1, o1 = cases.adversarial_reads(keys, K, seed=5, n=600)
    b2, o2 = cases.synth_reads(cum, parent, 2000, 150)
    raw1, raw2 = bytes(b1), bytes(b2)
    seqs = [raw1[int(o1[i]):int(o1[i + 1])] for i in range(600)] + [raw2[int(o2[i]):int(o2[i + 1])] for i in range(2000)]
    hb = hand_built(parent, keys, targets, np.random.default_rng(77))
    where = {}
    for name, s in hb.items():
        where[name] = len(seqs)
        seqs.append(s)
    bases, off = concat_reads(seqs)
    return bases, off, where


def chain_taxonomy(depth, branch_every=1):
    """a tree of the given depth: a spine 1 -> 2 -> .. -> depth + 1 (node i + 1 at depth i), and beside every spine node
    below the root a leaf sibling under the same parent -> parent array, spine nodes, sibling nodes"""
    spine = list(range(2, depth + 2))
    parent = [1, 1] + [1 if i == 2 else i - 1 for i in spine]
    sibs = []
    for i in spine:
        sibs.append(len(parent))
        parent.append(1 if i == 2 else i - 1)
    return np.array(parent, np.int32), spine, sibs
