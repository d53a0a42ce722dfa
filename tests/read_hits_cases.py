"""Seeded inputs shared by the read-hits tests (CPU model test and GPU tests): databases and reads, nothing else."""
import numpy as np

from helpers import concat_reads, small_db
from kmer_id_amd import synth

COMP = bytes.maketrans(b"ACGT", b"TGCA")


def key_seq(key, k):
    return synth.key_to_seq(key, k).encode()


def database(k=30, scale=2e-4, dup=False):
    """-> parent, cum, keys, targets (synthetic bact10-shaped); dup: every 7th entry and the first 50 once more at the
    end under OTHER targets -- the first insert must win"""
    parent, cum, keys, targets = small_db(scale, k=k)
    if dup:
        again = keys[::7]
        other = np.roll(targets[::7], 3)
        keys = np.concatenate([keys, again, keys[:50]])
        targets = np.concatenate([targets, other, targets[:50][::-1].copy()])
    return parent, cum, keys, targets


def synth_reads(cum, parent, n, length, k=30):
    return synth.reads(cum, parent, n, length, k=k), synth.fixed_offsets(n, length)


def adversarial_reads(keys, k, seed, n=600, u=False):
    """ragged reads (0 .. 300 bytes; 150, 250, 31, 30, 29 among them) of random bases with implanted database k-mers
    (forward and reverse complement, overlapping runs of them too) and bytes that are no bases"""
    rng = np.random.default_rng(seed)
    fixed = [150, 250, 31, 30, 29, k, k - 1, k + 1, 0, 1]
    junk = b"NnRY*-. \t\x00\xff@" + (b"" if u else b"Uu")
    seqs = []
    for i in range(n):
        length = fixed[i % len(fixed)] if i % 3 == 0 else int(rng.integers(0, 301))
        s = bytearray(rng.choice(np.frombuffer(b"ACGT", np.uint8), length).tobytes())
        for _ in range(int(rng.integers(0, 5))):  # implants
            if length < k:
                break
            kmer = key_seq(keys[int(rng.integers(0, keys.size))], k)
            if rng.integers(0, 2):
                kmer = kmer.translate(COMP)[::-1]
            at = int(rng.integers(0, length - k + 1))
            s[at:at + k] = kmer
        mode = int(rng.integers(0, 8))
        if mode == 0:
            s = bytearray(bytes(s).lower())
        elif mode == 1 and length:
            for _ in range(int(rng.integers(1, 4))):
                s[int(rng.integers(0, length))] = junk[int(rng.integers(0, len(junk)))]
        elif mode == 2 and length:  # mixed case
            for j in rng.integers(0, length, length // 3):
                s[j] = ord(chr(s[j]).lower())
        if u and mode in (3, 4):
            s = bytearray(bytes(s).replace(b"T", b"U") if mode == 3 else bytes(s).replace(b"t", b"u").replace(b"T", b"u"))
        seqs.append(bytes(s))
    return concat_reads(seqs)
