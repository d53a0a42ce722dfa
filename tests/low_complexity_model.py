"""The low-complexity rule (kmer_id_amd.h, "mask low-complexity sequence") in plain Python, two ways:
low_direct recounts the window of every position from nothing, low_sliding adds the triplet that enters and removes the
one that leaves.  Both work on one line; mask_reads / mask_block apply them to a batch."""
import numpy as np

WINDOW = 64
H = WINDOW // 2

_CODE = {ord("A"): 0, ord("a"): 0, ord("C"): 1, ord("c"): 1, ord("G"): 2, ord("g"): 2, ord("T"): 3, ord("t"): 3}
_CODE_U = dict(_CODE)
_CODE_U.update({ord("U"): 3, ord("u"): 3})


def codes_of(line, u_is_t=False):
    """line (bytes or uint8 array) -> list of codes, -1 for a byte that is no base"""
    table = _CODE_U if u_is_t else _CODE
    return [table.get(int(c), -1) for c in bytes(line)]


def triplets_of(codes):
    """value of triplet i (16 a + 4 b + c), -1 where it is not valid; one entry per i in 0 .. len - 3"""
    return [16 * a + 4 * b + c if a >= 0 and b >= 0 and c >= 0 else -1
            for a, b, c in zip(codes, codes[1:], codes[2:])]


def is_low(l, s, t):
    return l >= 2 and 10 * s > t * (l - 1)


def score_direct(codes, p):
    """(l, S) of position p, recounted"""
    n = len(codes)
    lo, hi = max(0, p - H), min(n, p + H)
    count = {}
    for i in range(lo, hi - 2):
        a, b, c = codes[i], codes[i + 1], codes[i + 2]
        if a >= 0 and b >= 0 and c >= 0:
            v = 16 * a + 4 * b + c
            count[v] = count.get(v, 0) + 1
    return sum(count.values()), sum(c * (c - 1) // 2 for c in count.values())


def low_direct(line, t, u_is_t=False):
    codes = codes_of(line, u_is_t)
    return [t > 0 and is_low(*score_direct(codes, p), t) for p in range(len(codes))]


def low_sliding(line, t, u_is_t=False):
    codes = codes_of(line, u_is_t)
    n = len(codes)
    if t <= 0:
        return [False] * n
    trip = triplets_of(codes)
    count = [0] * 64
    l = s = 0
    out = []
    lo = hi = 0  # the triplets counted are lo <= i, i + 3 <= hi
    for p in range(n):
        new_lo, new_hi = max(0, p - H), min(n, p + H)
        for i in range(max(hi - 2, 0), new_hi - 2):  # enter
            v = trip[i]
            if v >= 0:
                s += count[v]
                count[v] += 1
                l += 1
        for i in range(lo, new_lo):  # leave
            v = trip[i] if i < len(trip) else -1
            if v >= 0 and i + 3 <= hi:
                count[v] -= 1
                s -= count[v]
                l -= 1
        lo, hi = new_lo, new_hi
        out.append(is_low(l, s, t))
    return out


def mask_line(line, t, u_is_t=False, low=low_sliding):
    """-> (the line with every low base replaced by 'N', as bytes; how many)"""
    codes = codes_of(line, u_is_t)
    out = bytearray(bytes(line))
    n = 0
    for p, is_l in enumerate(low(line, t, u_is_t)):
        if is_l and codes[p] >= 0:
            out[p] = ord("N")
            n += 1
    return bytes(out), n


def mask_reads(bases, offsets, t, u_is_t=False):
    """bases + offsets (uint8, uint64[n + 1]) -> (masked copy, number masked): read by read, nothing shared"""
    out = np.array(bases, np.uint8, copy=True)
    total = 0
    for r in range(len(offsets) - 1):
        a, b = int(offsets[r]), int(offsets[r + 1])
        m, n = mask_line(out[a:b].tobytes(), t, u_is_t)
        out[a:b] = np.frombuffer(m, np.uint8)
        total += n
    return out, total


def mask_block(text, recs, t, u_is_t=False):
    """a FASTQ block with its line index (rows seq_off, seq_len, qual_off, qual_len) -> (masked copy, number masked)"""
    out = np.array(text, np.uint8, copy=True)
    total = 0
    for so, sl, qo, ql in np.asarray(recs).tolist():
        m, n = mask_line(out[so:so + sl].tobytes(), t, u_is_t)
        out[so:so + sl] = np.frombuffer(m, np.uint8)
        total += n
    return out, total
