"""Seeded inputs shared by the tests that need reads with many hits each: a database made of the k-mers of random genomes."""
import numpy as np

from helpers import K


def genome_db(parent, n_genomes, genome_len, rng):
    """k-mers of random genomes; the targets of one genome walk up and down one lineage (so the msca
    fold has work) with a few k-mers of a foreign lineage in between (so it also meets real LCAs)."""
    depth = np.zeros(parent.size, np.int64)
    for t in range(2, parent.size):
        d, x = 0, t
        while x > 1 and d < 64:
            x = int(parent[x]); d += 1
        depth[t] = d
    leaves = np.flatnonzero(depth >= 3)
    code = np.zeros(256, np.int64)
    for i, ch in enumerate(b"ACGT"):
        code[ch] = i
    genomes, keys, targets = [], [], []
    for g in range(n_genomes):
        seq = rng.choice(np.frombuffer(b"ACGT", np.uint8), genome_len)
        genomes.append(seq)
        c = code[seq]
        nwin = genome_len - K + 1
        key = np.zeros(nwin, np.uint64)
        for j in range(K):
            key = (key << np.uint64(2)) | c[j:j + nwin].astype(np.uint64)
        t0 = int(rng.choice(leaves))
        lineage = [t0, int(parent[t0]), int(parent[int(parent[t0])])]
        tg = np.array(lineage, np.uint32)[rng.integers(0, 3, nwin)]
        foreign = rng.random(nwin) < 0.02
        tg[foreign] = rng.choice(leaves, int(foreign.sum())).astype(np.uint32)
        keys.append(key); targets.append(tg)
    return genomes, np.concatenate(keys), np.concatenate(targets)
