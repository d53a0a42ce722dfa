"""Seeded inputs shared by the read-fragments tests (CPU model test and GPU tests): the database of read_support_cases and
reads dealt into fragments, nothing else."""
import numpy as np

import read_hits_cases as cases
import read_support_cases as sc
from helpers import concat_reads
from read_fragments_model import interleave

K = sc.K
RULES = [(0, 0), (3, 0), (2, 25), (0, 1000)]


def hand_built(parent, keys, targets, rng):
    """fragments whose hits have chosen targets, for nodes 5 -> 6 -> 8, 5 -> 35 -> 36 and a node X of another top-level
    lineage -> {name: (mate 1, mate 2)}"""
    assert parent[8] == 6 and parent[6] == 5 and parent[36] == 35 and parent[35] == 5 and parent[5] == 1
    first = np.unique(keys, return_index=True)[1]
    x = next(int(t) for t in targets[np.sort(first)] if t > 1 and sc.top_level(parent, int(t)) != 5)
    ks = lambda t, j=0: cases.key_seq(sc.key_of(keys, targets, t, j), K)  # noqa: E731
    imp = lambda ts: sc.implanted(rng, [ks(*t) if isinstance(t, tuple) else ks(t) for t in ts])  # noqa: E731
    return {
        "8|X_6": (imp([8]), imp([x, 6])),            # folds 8 -> 1 -> 6; msca(final_1, final_2) = msca(8, 1) = 8
        "X_6|8": (imp([x, 6]), imp([8])),            # the same mates swapped: folds X -> 1 -> 8
        "6_36|8": (imp([6, 36]), imp([8])),          # final 8, confident 5 at min_hits 3
        "X|8_6": (imp([x]), imp([8, 6])),            # final 6, confident 1 at min_hits 3
        "36|36": (imp([36]), imp([(36, 1)])),        # the mates agree: confident 36 at min_hits 2
        "root|root": (imp([(1, 0), (1, 1)]), imp([(1, 2)])),
        "6_8|": (imp([6, 8]), b""),                  # an absent mate 2
        "|6_8": (b"", imp([6, 8])),                  # an absent mate 1
        "|": (b"", b""),
        "same_kmer": (imp([36, 35]), imp([36, 5])),  # one database k-mer in both mates
    }


def fragments(parent, cum, keys, targets):
    """300 fragments dealt from adversarial_reads(n=600) (ragged and empty mates), 300 from 600 synthetic 150-bp reads and
    the hand-built ones -> bases, offsets (2 F reads, interleaved), {name: fragment index}"""
    b1, o1 = cases.adversarial_reads(keys, K, seed=5, n=600)
    b2, o2 = cases.synth_reads(cum, parent, 600, 150)
    raw1, raw2 = bytes(b1), bytes(b2)
    seqs = [raw1[int(o1[i]):int(o1[i + 1])] for i in range(600)] + [raw2[int(o2[i]):int(o2[i + 1])] for i in range(600)]
    m1, m2 = seqs[0::2], seqs[1::2]
    where = {}
    for name, (a, b) in hand_built(parent, keys, targets, np.random.default_rng(78)).items():
        where[name] = len(m1)
        m1.append(a)
        m2.append(b)
    bases, off = concat_reads(interleave(m1, m2))
    return bases, off, where
