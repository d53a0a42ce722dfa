"""Independent model of kid_db_read_loci*: place a read on a genome by its colinear hits.

Plain Python over dictionaries -- nothing from the code under test.  For one read with hits (pos_i, entry_i), i < m, its
n_kmers = n, the sites org[] / pos[] of the database's entries and the diagonal bin width W >= 1:

  * participants: the first min(m, MAX_HITS) hits in list order whose entry < len(org)
  * a participant with g = org[entry], x = pos[entry], r = pos_i has the keys (g, 0, (x - r) // W) and (g, 1, (x + r) // W)
    (Python's // floors toward minus infinity, integers of any size); c[key] counts the participants that have it
  * the best key has the largest c; ties: strand 0, then the lowest g, then the lowest diagonal; the chain = the
    participants with the best key
  * the record (LOCUS_DTYPE): org, strand of the best key; n_chain = its c; n_org = participants with g = org; n_other =
    the largest c over keys with g != org (0: none); n_hits = m; n_kmers = n; pos_first / pos_last = the smallest and
    largest pos in the chain; entry_first = the lowest entry among the chain hits at pos_first
  * no participant: every field but n_hits and n_kmers is 0
"""
import numpy as np

MAX_HITS = 4096
MAX_ORGS = 1 << 24
FIELDS = ("org", "strand", "n_chain", "n_org", "n_other", "n_hits", "n_kmers", "pos_first", "pos_last", "entry_first")
LOCUS_DTYPE = np.dtype([(name, np.uint32) for name in FIELDS])


def locus(pos, entry, n_kmers, org, site_pos, diag_bin=1):
    """one read -> its record, a dict over FIELDS"""
    w = int(diag_bin)
    assert w >= 1 and len(pos) == len(entry)
    m = len(pos)
    rec = dict.fromkeys(FIELDS, 0)
    rec["n_hits"], rec["n_kmers"] = m, int(n_kmers)
    count, parts = {}, []
    for i in range(min(m, MAX_HITS)):
        e, r = int(entry[i]), int(pos[i])
        if e >= len(org):
            continue
        g, x = int(org[e]), int(site_pos[e])
        keys = ((g, 0, (x - r) // w), (g, 1, (x + r) // w))
        for key in keys:
            count[key] = count.get(key, 0) + 1
        parts.append((r, e, g, keys))
    if not parts:
        return rec
    best = min(count, key=lambda key: (-count[key], key[1], key[0], key[2]))
    chain = sorted((r, e) for r, e, g, keys in parts if keys[best[1]] == best)
    rec["org"], rec["strand"], rec["n_chain"] = best[0], best[1], count[best]
    rec["n_org"] = sum(1 for r, e, g, keys in parts if g == best[0])
    rec["n_other"] = max([c for key, c in count.items() if key[0] != best[0]], default=0)
    rec["pos_first"], rec["entry_first"] = chain[0]
    rec["pos_last"] = chain[-1][0]
    assert len(chain) == count[best]
    return rec


def as_records(dicts):
    out = np.zeros(len(dicts), LOCUS_DTYPE)
    for i, d in enumerate(dicts):
        out[i] = tuple(d[f] for f in FIELDS)
    return out


def batch(hits, org, site_pos, diag_bin=1):
    """hits: a CSR with offsets, n_kmers, pos, entry (read_hits_model.Hits) -> LOCUS_DTYPE[n]"""
    n = hits.offsets.size - 1
    pos, entry = hits.pos.tolist(), hits.entry.tolist()
    org, site_pos = np.asarray(org).tolist(), np.asarray(site_pos).tolist()
    out = []
    for r in range(n):
        a, b = int(hits.offsets[r]), int(hits.offsets[r + 1])
        out.append(locus(pos[a:b], entry[a:b], int(hits.n_kmers[r]), org, site_pos, diag_bin))
    return as_records(out)


def line(rec, site_pos):
    """the fourth field of a line of a _loci.txt file"""
    return "%d:%d:%d:%d:%d:%d:%d:%d" % (rec["org"], rec["strand"], rec["n_chain"], rec["n_org"], rec["n_other"], rec["pos_first"],
                                        rec["pos_last"], int(site_pos[int(rec["entry_first"])]))
