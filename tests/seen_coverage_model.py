"""The rule of kid_seen_coverage / kid_seen_coverage_bins, independent of the library, twice: `coverage` in vectorised
numpy and `coverage_literal` as a Python loop per entry into dicts with a loop over the sorted occupied bins for max_gap.
Bits are unpacked as in shared_kmers_model (bit o = bit o % 8 of byte o / 8), everything at or beyond n_entries is
dropped.  Also the lines kmer_coverage prints."""
import numpy as np

from shared_kmers_model import bits_of

FIELDS = ("n_probes", "n_seen", "span_bins", "bins", "bins_seen", "max_gap", "max_bin_seen", "max_bin")
DTYPE = np.dtype([(name, np.uint32) for name in FIELDS])
MAX_BINS = 1 << 28


def bins_model(org, pos, bitmaps, bin_width, n_orgs):
    """-> (bin_base uint64[n_orgs + 1], probes_per_bin uint32[B], seen_per_bin uint32[n, B])"""
    org, pos = np.asarray(org, np.int64), np.asarray(pos, np.int64)
    b = pos // bin_width
    span = np.zeros(n_orgs, np.int64)
    np.maximum.at(span, org, b + 1)
    base = np.concatenate([[0], np.cumsum(span)]).astype(np.uint64)
    B = int(base[-1])
    assert B <= MAX_BINS
    key = base[:-1].astype(np.int64)[org] + b
    probes = np.bincount(key, minlength=B).astype(np.uint32)
    seen = np.zeros((len(bitmaps), B), np.uint32)
    for i, bm in enumerate(bitmaps):
        seen[i] = np.bincount(key[bits_of(bm, org.size)], minlength=B)
    return base, probes, seen


def _longest_zero_run(zero):
    """the longest run of True in a bool array"""
    if zero.size == 0:
        return 0
    edges = np.diff(np.concatenate([[0], zero.astype(np.int8), [0]]))
    starts, ends = np.flatnonzero(edges == 1), np.flatnonzero(edges == -1)
    return int((ends - starts).max()) if starts.size else 0


def coverage(org, pos, bitmaps, bin_width, n_orgs):
    """-> DTYPE[n, n_orgs], vectorised per organism"""
    base, probes, seen = bins_model(org, pos, bitmaps, bin_width, n_orgs)
    out = np.zeros((len(bitmaps), n_orgs), DTYPE)
    for g in range(n_orgs):
        lo, hi = int(base[g]), int(base[g + 1])
        p = probes[lo:hi]
        occ = np.flatnonzero(p > 0)
        for i in range(len(bitmaps)):
            s = seen[i, lo:hi]
            r = out[i, g]
            r["n_probes"], r["n_seen"], r["span_bins"] = p.sum(), s.sum(), hi - lo
            r["bins"], r["bins_seen"] = occ.size, np.count_nonzero(s)
            r["max_gap"] = _longest_zero_run(s[occ] == 0)
            if s.sum() > 0:
                r["max_bin_seen"], r["max_bin"] = s.max(), int(np.argmax(s))  # argmax: the first, lowest, index
    return out


def coverage_literal(org, pos, bitmaps, bin_width, n_orgs):
    """-> DTYPE[n, n_orgs], one entry at a time"""
    n_entries = len(org)
    out = np.zeros((len(bitmaps), n_orgs), DTYPE)
    for i, bm in enumerate(bitmaps):
        bm = bytes(np.ascontiguousarray(bm, np.uint8))
        probes = [dict() for _ in range(n_orgs)]
        seen = [dict() for _ in range(n_orgs)]
        for o in range(n_entries):
            g, b = int(org[o]), int(pos[o]) // bin_width
            probes[g][b] = probes[g].get(b, 0) + 1
            if (bm[o >> 3] >> (o & 7)) & 1:
                seen[g][b] = seen[g].get(b, 0) + 1
        for g in range(n_orgs):
            if not probes[g]:
                continue
            run = gap = 0
            best, best_bin = 0, 0
            for b in sorted(probes[g]):
                s = seen[g].get(b, 0)
                run = run + 1 if s == 0 else 0
                gap = max(gap, run)
                if s > best:
                    best, best_bin = s, b
            out[i, g] = (sum(probes[g].values()), sum(seen[g].values()), max(probes[g]) + 1, len(probes[g]), len(seen[g]), gap, best,
                         best_bin)
    return out


def cli_lines(paths, records, min_seen=1):
    """what kmer_coverage prints for the files `paths` whose records are `records` [n, n_orgs]"""
    n, n_orgs = records.shape
    out = ["#%d\t%s\t%d\n" % (f, paths[f], int(records[f]["n_seen"].astype(np.int64).sum())) for f in range(n)]
    for f in range(n):
        for g in range(n_orgs):
            r = records[f, g]
            if int(r["n_seen"]) >= min_seen:
                out.append("%d,%d,%s\n" % (f, g, ",".join(str(int(r[name])) for name in FIELDS)))
    return "".join(out).encode()


def cli_bins_lines(paths, base, probes, seen, the_org):
    """what kmer_coverage --bins the_org prints"""
    n = len(paths)
    out = ["#%d\t%s\t%d\n" % (f, paths[f], int(seen[f].astype(np.int64).sum())) for f in range(n)]
    lo, hi = int(base[the_org]), int(base[the_org + 1])
    for f in range(n):
        for b in range(lo, hi):
            if probes[b] > 0:
                out.append("%d,%d,%d,%d,%d\n" % (f, the_org, b - lo, int(probes[b]), int(seen[f, b])))
    return "".join(out).encode()
