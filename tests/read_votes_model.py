"""Independent model of kid_db_read_votes*: reads called by root-path votes.

numpy only, on top of tests/read_hits_model.py (HitModel.batch gives the hits) and tests/read_support_model.py (S(c), the
rule and the climb, started from `call` instead of `final`).  For one read with hit targets t_1 .. t_m and n windows:

  w(c)       #{i : t_i = c}
  P(c)       #{i : t_i is c or an ancestor of c} = the sum of w over c's root path
  best       max_i P(t_i);  L = the distinct hit targets with P = best
  call       the lowest common ancestor of L (the deepest node on every member's root path); 0 when m = 0
  confident  the first node on call, parent(call), .., 1 that passes the rule; 0 if none does or call = 0

VoteModel.batch_literal follows the definition with Python integers: root paths by climbing parent[].
VoteModel.batch_anc is vectorised over the whole batch with SupportModel's anc table.
tests/test_read_votes_model.py holds the two against each other.
"""
from collections import Counter

import numpy as np

VOTE_DTYPE = np.dtype([("call", np.uint32), ("confident", np.uint32), ("n_kmers", np.uint32), ("n_hits", np.uint32),
                       ("p_best", np.uint32), ("n_best", np.uint32), ("s_call", np.uint32), ("s_confident", np.uint32)])


class VoteModel:
    def __init__(self, support_model):
        self.sm = support_model

    # ---- the definition, literally
    def root_path(self, c):
        """c, parent(c), .., 1"""
        path, c = [], int(c)
        while True:
            path.append(c)
            if c == 1:
                return path
            c = int(self.sm.parent[c])

    def call_literal(self, targets):
        """-> (call, p_best, n_best) of a read with these hit targets"""
        if len(targets) == 0:
            return 0, 0, 0
        w = Counter(int(t) for t in targets)
        p = {c: sum(w.get(a, 0) for a in self.root_path(c)) for c in w}
        best = max(p.values())
        members = [c for c in w if p[c] == best]
        common = set(self.root_path(members[0]))
        for c in members[1:]:
            common &= set(self.root_path(c))
        call = next(a for a in self.root_path(members[0]) if a in common)  # the deepest: the path runs upwards
        return call, best, len(members)

    def read_literal(self, targets, n, rule):
        call, best, n_best = self.call_literal(targets)
        _, conf, _, m, s_call, s_conf = self.sm.read_literal(targets, n, rule, call)
        return (call, conf, n, m, best, n_best, s_call, s_conf)

    def batch_literal(self, hits, rule):
        n = hits.offsets.size - 1
        out = np.zeros(n, VOTE_DTYPE)
        for r in range(n):
            out[r] = self.read_literal(hits.of(r)[1].tolist(), int(hits.n_kmers[r]), rule)
        return out

    # ---- all reads at once with the anc table
    def calls_anc(self, hits):
        """-> call, p_best, n_best per read"""
        anc = self.sm.anc
        n, nd, ntar = hits.offsets.size - 1, anc.shape[1], anc.shape[0]
        per = np.diff(hits.offsets.astype(np.int64))
        read_of = np.repeat(np.arange(n), per)
        tgt = hits.target.astype(np.int64)
        call, best, n_best = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
        if tgt.size == 0:
            return call, best, n_best
        ukey, w = np.unique(read_of * ntar + tgt, return_counts=True)  # w of every (read, node) with a hit
        paths = anc[tgt]  # [hit, d] = the node at depth d of the hit's root path, negative beyond its depth
        p = np.zeros(tgt.size, np.int64)
        for d in range(nd):
            on = paths[:, d] >= 0
            key = read_of[on] * ntar + paths[on, d]
            i = np.minimum(np.searchsorted(ukey, key), ukey.size - 1)
            p[on] += np.where(ukey[i] == key, w[i], 0)
        np.maximum.at(best, read_of, p)
        member = np.unique((read_of * ntar + tgt)[p == best[read_of]])  # distinct members of L, sorted by read
        m_read, m_paths = member // ntar, anc[member % ntar]
        n_best = np.bincount(m_read, minlength=n)
        first = np.flatnonzero(np.diff(np.concatenate(([-1], m_read))))  # where each read's members start
        has = m_read[first]
        lo = np.minimum.reduceat(m_paths, first, axis=0)
        hi = np.maximum.reduceat(m_paths, first, axis=0)
        depth = np.cumprod((lo == hi) & (lo >= 0), axis=1).sum(axis=1) - 1  # the common prefix of the members' root paths
        call[has] = lo[np.arange(has.size), depth]
        return call, best, n_best

    def batch_anc(self, hits, rule, calls=None):
        call, best, n_best = self.calls_anc(hits) if calls is None else calls
        s = self.sm.batch_identity(hits, rule, call.astype(np.uint32))
        out = np.zeros(call.size, VOTE_DTYPE)
        out["call"], out["confident"], out["n_kmers"], out["n_hits"] = call, s["confident"], s["n_kmers"], s["n_hits"]
        out["p_best"], out["n_best"], out["s_call"], out["s_confident"] = best, n_best, s["s_final"], s["s_confident"]
        return out
