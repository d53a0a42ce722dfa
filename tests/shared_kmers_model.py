"""The rule of kid_db_shared_kmers / kid_shared_kmers in numpy, independent of the library: unpack the bits of every
bitmap (bit o = bit o % 32 of little-endian 32-bit word o / 32, which is bit o % 8 of byte o / 8), drop everything at or
beyond n_entries, and count per pair the targets of the entries both have.  Also the lines kmer_shared prints."""
import numpy as np


def seen_bytes(n_entries):
    """the padded size of a bitmap for n_entries entries: whole 16-byte groups, at least one"""
    return max((n_entries + 127) // 128, 1) * 16


def bits_of(bitmap, n_entries):
    """-> bool[n_entries]"""
    return np.unpackbits(np.ascontiguousarray(bitmap, np.uint8), bitorder="little")[:n_entries].astype(bool)


def pack(bits, n_entries=None, pad_ones=False):
    """bool[n_entries] -> a bitmap of seen_bytes(n_entries) bytes; pad_ones: with every padding bit set"""
    n = len(bits) if n_entries is None else n_entries
    full = np.full(seen_bytes(n) * 8, 1 if pad_ones else 0, np.uint8)
    full[:n] = np.asarray(bits, np.uint8)
    return np.packbits(full, bitorder="little")


def shared(targets, ntar, bitmaps):
    """-> int64[n, n, ntar]"""
    targets = np.asarray(targets, np.int64)
    bits = [bits_of(b, targets.size) for b in bitmaps]
    n = len(bits)
    out = np.zeros((n, n, ntar), np.int64)
    for i in range(n):
        for j in range(i, n):
            out[i, j] = out[j, i] = np.bincount(targets[bits[i] & bits[j]], minlength=ntar)
    return out


def cli_lines(paths, matrix, min_shared=0):
    """what kmer_shared prints for the files `paths` whose matrix is `matrix`"""
    n, _, ntar = matrix.shape
    out = ["#%d\t%s\t%d\n" % (f, paths[f], int(matrix[f, f].sum())) for f in range(n)]
    for a in range(n):
        for b in range(a + 1, n):
            for t in range(ntar):
                ka, kb, s = int(matrix[a, a, t]), int(matrix[b, b, t]), int(matrix[a, b, t])
                if ka > 0 and kb > 0 and s >= min_shared:
                    out.append("%d,%d,%d,%d,%d,%d\n" % (a, b, t, ka, kb, s))
    return "".join(out).encode()
