"""Independent model of k-mer depth per database entry (KID_OPT_ENTRY_DEPTH) and of its per-target spectrum.

numpy only, on top of tests/read_hits_model.py (HitModel.batch gives the hits) and tests/read_support_model.py
(SupportModel.batch_identity gives `confident`):

  depth[o]        hits with target > 1 and entry o among the counted reads with confident > 0; saturates at 2^32 - 1
  spectrum[t, b]  entries o with targets[o] == t and depth[o] == b for b < bins - 1; the last column: depth[o] >= bins - 1
  ksum[t]         sum of depth over the entries of t;  dmax[t]  the largest
  the depth file  one line i,kmer_hits,distinct,q1,q2,q3,max per target from the spectrum with bins = 256:
                  distinct = columns 1..255; q_p = the smallest d >= 1 with 4 * #{1 <= depth <= d} >= p * distinct (the last
                  column taken as d = 255), 0 when distinct = 0
"""
import numpy as np

DEPTH_MAX = 0xFFFFFFFF
FILE_BINS = 256


def depth_of(hits, rec, counted, n_entries):
    """the counters a tally of the batch leaves in a zeroed sample (rec: the model's support records)"""
    per = np.diff(hits.offsets.astype(np.int64))
    read_of = np.repeat(np.arange(per.size), per)
    take = (np.asarray(counted, bool) & (rec["confident"] > 0))[read_of] & (hits.target > 1)
    d = np.bincount(hits.entry[take].astype(np.int64), minlength=int(n_entries))
    return np.minimum(d, DEPTH_MAX).astype(np.uint32)


def saturating_add(a, b):
    return np.minimum(np.asarray(a, np.uint64) + np.asarray(b, np.uint64), DEPTH_MAX).astype(np.uint32)


def spectrum_of(depth, entry_targets, ntar, bins):
    """-> (spectrum uint64[ntar, bins], ksum uint64[ntar], dmax uint32[ntar])"""
    assert 2 <= bins <= 4096
    depth = np.asarray(depth, np.uint32)
    t = np.asarray(entry_targets).astype(np.int64)
    assert depth.size == t.size
    spectrum = np.zeros((ntar, bins), np.uint64)
    np.add.at(spectrum, (t, np.minimum(depth.astype(np.int64), bins - 1)), 1)
    ksum = np.zeros(ntar, np.uint64)
    np.add.at(ksum, t, depth.astype(np.uint64))
    dmax = np.zeros(ntar, np.uint32)
    np.maximum.at(dmax, t, depth)
    return spectrum, ksum, dmax


def quartiles(row):
    """(distinct, q1, q2, q3) of one target's spectrum row (any number of bins; the last column is d = bins - 1)"""
    row = [int(x) for x in row]
    distinct = sum(row[1:])
    if distinct == 0:
        return 0, 0, 0, 0
    qs = []
    for p in (1, 2, 3):
        below = 0
        for d in range(1, len(row)):
            below += row[d]
            if 4 * below >= p * distinct:
                qs.append(d)
                break
    return (distinct,) + tuple(qs)


def depth_lines(spectrum, ksum, dmax):
    """the text of the depth file"""
    out = []
    for i in range(spectrum.shape[0]):
        distinct, q1, q2, q3 = quartiles(spectrum[i])
        out.append("%d,%d,%d,%d,%d,%d,%d\n" % (i, int(ksum[i]), distinct, q1, q2, q3, int(dmax[i])))
    return "".join(out)
