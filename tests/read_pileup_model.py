"""The rule of kid_pileup_* (include/kmer_id_amd.h), restated literally: placed reads piled up per genome bin.

Geometry, that of seen_coverage for the same bin width W: n_orgs = the largest org + 1; span_bins[g] = 1 + max(pos[o] // W)
over the entries of organism g, 0 when it has none; bin_base = the exclusive scan of span_bins; B their sum.

A record L (LOCUS_DTYPE of read_loci_model) is placed under (min_chain >= 1, min_margin >= 0) when
    L.n_chain >= min_chain,  (L.n_chain - L.n_other if L.n_chain >= L.n_other else 0) >= min_margin,  L.strand <= 1,
    L.entry_first < n_entries  and  L.org == org[L.entry_first];
otherwise it changes nothing.  A placed record, with a = pos[L.entry_first], d = L.pos_last - L.pos_first if L.pos_last >=
L.pos_first else 0 and k the k-mer length:
    forward (strand 0)  lo = a,              hi = a + d + k - 1
    reverse (strand 1)  lo = max(0, a - d),  hi = a + k - 1
    b_lo = min(lo // W, span_bins[g] - 1),  b_hi = min(hi // W, span_bins[g] - 1)  with g = L.org
adds 1 to starts[g][b_lo] and 1 to depth[g][b] for every b in b_lo..b_hi.  Counters are taken modulo 2^32.

Here every record walks its bins b_lo..b_hi into dictionaries keyed (g, b): there is no step array (steps() below is the
other form, for the tests that hold the two against each other).  Python integers throughout.
"""
import numpy as np

PILEUP_FIELDS = ("n_placed", "span_bins", "bins_covered", "max_gap", "max_depth", "max_depth_bin", "max_starts", "max_starts_bin", "reserved")
# nine uint32, four bytes of padding, depth_sum at offset 40: 48 bytes
PILEUP_DTYPE = np.dtype({"names": PILEUP_FIELDS + ("depth_sum",), "formats": [np.uint32] * 9 + [np.uint64],
                         "offsets": [4 * i for i in range(9)] + [40], "itemsize": 48})


def geometry(org, pos, W):
    """-> span_bins int64[n_orgs], bin_base uint64[n_orgs + 1]"""
    n_orgs = int(org.max()) + 1 if org.size else 0
    span = np.zeros(n_orgs, np.int64)
    np.maximum.at(span, org.astype(np.int64), pos.astype(np.int64) // W + 1)
    bin_base = np.zeros(n_orgs + 1, np.uint64)
    bin_base[1:] = np.cumsum(span)
    return span, bin_base


def placed(L, org, min_chain, min_margin):
    n_chain, n_other, e = int(L["n_chain"]), int(L["n_other"]), int(L["entry_first"])
    margin = n_chain - n_other if n_chain >= n_other else 0
    return n_chain >= min_chain and margin >= min_margin and int(L["strand"]) <= 1 and e < org.size and int(L["org"]) == int(org[e])


def interval(L, pos, k):
    """-> lo, hi of a placed record"""
    a = int(pos[int(L["entry_first"])])
    first, last = int(L["pos_first"]), int(L["pos_last"])
    d = last - first if last >= first else 0
    if int(L["strand"]) == 0:
        return a, a + d + k - 1
    return max(0, a - d), a + k - 1


def walk(loci, org, pos, k, W, span, min_chain, min_margin, starts=None, depth=None):
    """the records into the dictionaries starts and depth, keyed (g, b) -> starts, depth, the number placed"""
    starts = {} if starts is None else starts
    depth = {} if depth is None else depth
    n_placed = 0
    for L in loci:
        if not placed(L, org, min_chain, min_margin):
            continue
        n_placed += 1
        g = int(L["org"])
        lo, hi = interval(L, pos, k)
        b_lo, b_hi = min(lo // W, int(span[g]) - 1), min(hi // W, int(span[g]) - 1)
        starts[g, b_lo] = starts.get((g, b_lo), 0) + 1
        for b in range(b_lo, b_hi + 1):
            depth[g, b] = depth.get((g, b), 0) + 1
    return starts, depth, n_placed


def dense(d, span, bin_base):
    """a dictionary keyed (g, b) -> uint32[B] in the layout of bin_base"""
    out = np.zeros(int(bin_base[-1]), np.uint32)
    for (g, b), v in d.items():
        assert 0 <= b < int(span[g])
        out[int(bin_base[g]) + b] = v % 2 ** 32
    return out


def longest_zero_run(d):
    best = cur = 0
    for zero in (d == 0).tolist():
        cur = cur + 1 if zero else 0
        best = max(best, cur)
    return best


def records(span, bin_base, starts, depth):
    """starts, depth: uint32[B] -> PILEUP_DTYPE[n_orgs]"""
    out = np.zeros(span.size, PILEUP_DTYPE)
    for g in np.flatnonzero(span).tolist():
        a, n = int(bin_base[g]), int(span[g])
        s, d = starts[a:a + n], depth[a:a + n]
        r = out[g]
        r["n_placed"] = int(s.astype(np.uint64).sum()) % 2 ** 32
        r["span_bins"] = n
        r["bins_covered"] = int((d >= 1).sum())
        r["max_gap"] = longest_zero_run(d)
        r["max_depth"], r["max_depth_bin"] = int(d.max()), (int(d.argmax()) if d.max() else 0)  # (argmax: the lowest index)
        r["max_starts"], r["max_starts_bin"] = int(s.max()), (int(s.argmax()) if s.max() else 0)
        r["depth_sum"] = int(d.astype(np.uint64).sum())
    return out


def batch(loci, org, pos, k, W, min_chain, min_margin):
    """-> (bin_base uint64[n_orgs + 1], starts uint32[B], depth uint32[B], records PILEUP_DTYPE[n_orgs], n_placed)"""
    span, bin_base = geometry(org, pos, W)
    s, d, n_placed = walk(loci, org, pos, k, W, span, min_chain, min_margin)
    starts, depth = dense(s, span, bin_base), dense(d, span, bin_base)
    return bin_base, starts, depth, records(span, bin_base, starts, depth), n_placed


def steps(loci, org, pos, k, W, min_chain, min_margin):
    """The step-array form in numpy -> (starts uint32[B], steps uint32[B + n_orgs]): organism g owns the span_bins[g] + 1
    slots from bin_base[g] + g on, the last a sentinel; a placed record adds +1 at slot b_lo and -1 at slot b_hi + 1."""
    span, bin_base = geometry(org, pos, W)
    starts = np.zeros(int(bin_base[-1]), np.uint32)
    step = np.zeros(int(bin_base[-1]) + span.size, np.uint32)
    for L in loci:
        if not placed(L, org, min_chain, min_margin):
            continue
        g = int(L["org"])
        lo, hi = interval(L, pos, k)
        b_lo, b_hi = min(lo // W, int(span[g]) - 1), min(hi // W, int(span[g]) - 1)
        for a, i, by in ((starts, int(bin_base[g]) + b_lo, 1), (step, int(bin_base[g]) + g + b_lo, 1), (step, int(bin_base[g]) + g + b_hi + 1, -1)):
            a[i] = (int(a[i]) + by) % 2 ** 32  # (-1 as uint32 wrap-around)
    return starts, step


def depth_of_steps(step, span, bin_base):
    """one unsegmented inclusive scan over all slots, the sentinels dropped -> uint32[B]"""
    run = np.cumsum(step.astype(np.uint64)).astype(np.uint32)  # (modulo 2^32)
    slot = np.ones(step.size, bool)
    slot[(bin_base[1:].astype(np.int64) + np.arange(span.size))] = False  # organism g's sentinel: bin_base[g] + g + span[g]
    return run[slot]
