"""Independent model of kid_db_read_fragment_loci*: place a mate pair as one fragment by its colinear hits.

Plain Python over dictionaries -- nothing from the code under test (read_loci_model is imported by the tests for the
comparison with a single read alone, never here).  For one fragment with the hits (pos_i, entry_i) of mate 1 and of mate 2,
n = n_1 + n_2, the sites org[] / pos[] of the database's entries, the diagonal bin W >= 1, max_span >= 0 and the k-mer
length k:

  * participants of mate s: the first min(m_s, MAX_HITS) hits in list order whose entry < len(org)
  * a participant with g = org[entry], x = pos[entry], r = pos_i has the forward key (g, (x - r) // W) and the reverse key
    (g, (x + r) // W); F_s[key] and R_s[key] count the participants of mate s that have the key
  * paired placement (o, g, D, E): o = 0 takes (g, D) of F_1 and (g, E) of R_2, o = 1 takes F_2 and R_1; allowed when
    D <= E and (E - D) * W <= max_span; its score is the sum of the two counts
  * solo placement (s, t, g, d): one key of one mate, t = 0 forward or 1 reverse, its count the score
  * best: the highest score; a paired one before a solo one; paired by (o, g, D, E), solo by (t, g, d, s) ascending
  * the record (FRAGMENT_LOCUS_DTYPE), see record() below; without a participant all but n_hits and n_kmers is 0
"""
import bisect

import numpy as np

MAX_HITS = 4096
FIELDS = ("org", "orient", "mates", "n_chain", "n_chain_1", "n_chain_2", "n_org", "n_other", "n_hits", "n_kmers", "lo", "hi",
          "pos_first_1", "pos_last_1", "pos_first_2", "pos_last_2")
FRAGMENT_LOCUS_DTYPE = np.dtype([(name, np.uint32) for name in FIELDS])
U32 = 2 ** 32


def _mate(pos, entry, org, site_pos, w):
    """-> participants [(r, e, g, x, D, E)], F {(g, D): count}, R {(g, E): count}"""
    parts, F, R = [], {}, {}
    for i in range(min(len(pos), MAX_HITS)):
        e, r = int(entry[i]), int(pos[i])
        if e >= len(org):
            continue
        g, x = int(org[e]), int(site_pos[e])
        D, E = (x - r) // w, (x + r) // w
        F[g, D] = F.get((g, D), 0) + 1
        R[g, E] = R.get((g, E), 0) + 1
        parts.append((r, e, g, x, D, E))
    return parts, F, R


def placements(mates, w, max_span):
    """every placement as (score, rank, g, chosen) with rank the tie order (a smaller rank wins among equal scores) and
    chosen = {s: (t, diagonal)} for the mates s in it.  (The partners of a forward key are looked up in a sorted list per
    org, so that a fragment of thousands of hits does not cost the product of its keys.)"""
    (p1, F1, R1), (p2, F2, R2) = mates
    reach = max_span // w  # (E - D) * w <= max_span  <=>  E - D <= max_span // w, for integers E - D >= 0
    for o, (F, sf), (R, sr) in ((0, (F1, 1), (R2, 2)), (1, (F2, 2), (R1, 1))):
        by_org = {}
        for (g, E) in sorted(R):
            by_org.setdefault(g, []).append(E)
        for (g, D), cf in F.items():
            row = by_org.get(g, ())
            for E in row[bisect.bisect_left(row, D):bisect.bisect_right(row, D + reach)]:
                assert D <= E and (E - D) * w <= max_span
                yield (cf + R[g, E], (0, o, g, D, E), g, {sf: (0, D), sr: (1, E)})
    for s, (parts, F, R) in ((1, mates[0]), (2, mates[1])):
        for t, table in ((0, F), (1, R)):
            for (g, d), c in table.items():
                yield (c, (1, t, g, d, s), g, {s: (t, d)})


def record(pos1, entry1, pos2, entry2, n_kmers, org, site_pos, k, diag_bin=1, max_span=1000, want_unique=False):
    """one fragment -> its record, a dict over FIELDS (and whether no other placement reaches the best score)"""
    w = int(diag_bin)
    assert w >= 1 and max_span >= 0
    rec = dict.fromkeys(FIELDS, 0)
    rec["n_hits"] = (len(pos1) + len(pos2)) % U32
    rec["n_kmers"] = int(n_kmers) % U32
    mates = (_mate(pos1, entry1, org, site_pos, w), _mate(pos2, entry2, org, site_pos, w))
    best, ties, by_org = None, 0, {}
    for p in placements(mates, w, max_span):
        by_org[p[2]] = max(by_org.get(p[2], 0), p[0])
        if best is None or (-p[0], p[1]) < (-best[0], best[1]):
            ties = 1 if best is None or p[0] != best[0] else ties + 1
            best = p
        elif p[0] == best[0]:
            ties += 1
    if best is None:
        return (rec, True) if want_unique else rec
    score, rank, g, chosen = best
    unique = ties == 1
    rec["org"], rec["n_chain"] = g, score
    rec["mates"] = 3 if len(chosen) == 2 else next(iter(chosen))
    t1 = chosen[1][0] if 1 in chosen else 1 - chosen[2][0]
    rec["orient"] = t1  # 0: mate 1 reads forward
    rec["n_org"] = sum(1 for parts, F, R in mates for p in parts if p[2] == g)
    rec["n_other"] = max([c for g2, c in by_org.items() if g2 != g], default=0)
    lows, highs = [], []
    for s, (t, d) in chosen.items():
        chain = sorted((p[0], p[1], p[3]) for p in mates[s - 1][0] if p[2] == g and p[4 + t] == d)
        rec["n_chain_%d" % s] = len(chain)
        first, last, a = chain[0][0], chain[-1][0], chain[0][2]
        rec["pos_first_%d" % s], rec["pos_last_%d" % s] = first, last
        span = last - first
        if t == 0:
            lows.append(a)
            highs.append(a + span + k - 1)
        else:
            lows.append(max(0, a - span))
            highs.append(a + k - 1)
    assert rec["n_chain_1"] + rec["n_chain_2"] == score
    rec["lo"], rec["hi"] = min(lows), min(max(highs), U32 - 1)
    return (rec, unique) if want_unique else rec


def as_records(dicts):
    out = np.zeros(len(dicts), FRAGMENT_LOCUS_DTYPE)
    for i, d in enumerate(dicts):
        out[i] = tuple(d[f] for f in FIELDS)
    return out


def batch(hits, org, site_pos, k, diag_bin=1, max_span=1000):
    """hits: an interleaved CSR of 2 F reads with offsets, n_kmers, pos, entry -> FRAGMENT_LOCUS_DTYPE[F]"""
    n = hits.offsets.size - 1
    assert n % 2 == 0
    pos, entry = hits.pos.tolist(), hits.entry.tolist()
    org, site_pos = np.asarray(org).tolist(), np.asarray(site_pos).tolist()
    off = [int(v) for v in hits.offsets]
    out = []
    for f in range(n // 2):
        a, b, c = off[2 * f], off[2 * f + 1], off[2 * f + 2]
        nk = int(hits.n_kmers[2 * f]) + int(hits.n_kmers[2 * f + 1])
        out.append(record(pos[a:b], entry[a:b], pos[b:c], entry[b:c], nk, org, site_pos, k, diag_bin, max_span))
    return as_records(out)


def line(j, rec):
    """a line of a _fragment_loci.txt file, without its LF"""
    return "%d\t%d\t%d\t%d:%d:%d:%d:%d:%d:%d:%d:%d:%d" % (
        j, rec["n_kmers"], rec["n_hits"], rec["org"], rec["orient"], rec["mates"], rec["n_chain"], rec["n_chain_1"], rec["n_chain_2"],
        rec["n_org"], rec["n_other"], rec["lo"], rec["hi"])


# ---- the pileup of fragment records (kid_pileup_add_fragments): the rule restated over the dictionaries of read_pileup_model
def fragment_placed(L, span, min_chain, min_margin, paired_only):
    n_chain, n_other, g = int(L["n_chain"]), int(L["n_other"]), int(L["org"])
    margin = n_chain - n_other if n_chain >= n_other else 0
    return (1 <= int(L["mates"]) <= 3 and (not paired_only or int(L["mates"]) == 3) and n_chain >= min_chain and margin >= min_margin
            and g < len(span) and int(span[g]) >= 1 and int(L["lo"]) <= int(L["hi"]))


def fragment_walk(recs, W, span, min_chain, min_margin, paired_only, starts=None, depth=None):
    """the records into the dictionaries starts and depth, keyed (g, b) -> starts, depth, the number placed"""
    starts = {} if starts is None else starts
    depth = {} if depth is None else depth
    n_placed = 0
    for L in recs:
        if not fragment_placed(L, span, min_chain, min_margin, paired_only):
            continue
        n_placed += 1
        g = int(L["org"])
        b_lo, b_hi = min(int(L["lo"]) // W, int(span[g]) - 1), min(int(L["hi"]) // W, int(span[g]) - 1)
        starts[g, b_lo] = starts.get((g, b_lo), 0) + 1
        for b in range(b_lo, b_hi + 1):
            depth[g, b] = depth.get((g, b), 0) + 1
    return starts, depth, n_placed
