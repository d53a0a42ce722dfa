"""Independent model of kid_db_read_support*: reads called by k-mer support.

numpy and the oracle binding only, on top of tests/read_hits_model.py (HitModel.batch gives the hits, HitModel.fold gives
`final`).  For one read with hit targets t_1 .. t_m (read-position order) and n windows looked up:

  final      the reference's left fold over the targets (0 when m = 0)
  S(c)       hits whose target is c or a descendant of c
  c passes   S(c) >= min_hits and 1000 * S(c) >= min_permille * n   (Python integers)
  confident  0 if final = 0, else the first node on final, parent(final), .., 1 that passes, 0 if none does

SupportModel.batch_literal computes S(c) by climbing the parent array from every hit, literally.
SupportModel.batch_identity is vectorised and uses the identity the kernel uses: with d_i = depth of the deepest common
node of t_i and final, the node at depth d of final's root path has S = #{i : d_i >= d}.
tests/test_read_support_model.py holds the two against each other and the (0, 0) tally against the oracle's counters.
"""
import numpy as np

SUPPORT_DTYPE = np.dtype([("final", np.uint32), ("confident", np.uint32), ("n_kmers", np.uint32), ("n_hits", np.uint32),
                          ("s_final", np.uint32), ("s_confident", np.uint32)])

RULES = [(0, 0), (1, 0), (2, 0), (3, 0), (0, 10), (0, 50), (2, 25), (0, 1000), (10 ** 6, 0)]


def passes(s, n, rule):
    return s >= rule[0] and 1000 * s >= rule[1] * n


class SupportModel:
    def __init__(self, hit_model, parent):
        self.hm = hit_model
        p = np.asarray(parent, np.int64).copy()
        p[0] = 1  # Tree1::get_parent: nodes 0 and 1 answer the root
        p[1] = 1
        self.parent = p
        depth = np.full(p.size, -1, np.int64)
        depth[1] = 0
        for i in range(p.size):
            path, z = [], i
            while depth[z] < 0:
                path.append(z)
                z = int(p[z])
            d = int(depth[z])
            for node in reversed(path):
                d += 1
                depth[node] = d
        self.depth = depth
        # anc[c, d] = the node at depth d of c's root path (-1 - c beyond its depth: never equal between two nodes)
        self.anc = -1 - np.repeat(np.arange(p.size)[:, None], int(depth.max()) + 1, axis=1)
        for c in range(p.size):
            z = c
            for d in range(int(depth[c]), -1, -1):
                self.anc[c, d] = z
                z = int(p[z])

    def finals(self, hits):
        return np.array([self.hm.fold(hits.of(r)[1]) for r in range(hits.offsets.size - 1)], np.uint32)

    # ---- the definition, literally
    def under(self, t, c):
        """is c the node t or an ancestor of it: climb parent[] from t"""
        t = int(t)
        while True:
            if t == c:
                return True
            if t == 1:
                return False
            t = int(self.parent[t])

    def read_literal(self, targets, n, rule, final):
        m = len(targets)
        if final == 0:
            return (0, 0, n, m, 0, 0)
        s_final = sum(self.under(t, final) for t in targets)
        c = int(final)
        while True:
            s = sum(self.under(t, c) for t in targets)
            if passes(s, n, rule):
                return (final, c, n, m, s_final, s)
            if c == 1:
                return (final, 0, n, m, s_final, 0)
            c = int(self.parent[c])

    def batch_literal(self, hits, rule, finals):
        n = hits.offsets.size - 1
        out = np.zeros(n, SUPPORT_DTYPE)
        for r in range(n):
            out[r] = self.read_literal(hits.of(r)[1].tolist(), int(hits.n_kmers[r]), rule, int(finals[r]))
        return out

    # ---- the identity, all reads at once
    def batch_identity(self, hits, rule, finals):
        n = hits.offsets.size - 1
        per = np.diff(hits.offsets.astype(np.int64))
        read_of = np.repeat(np.arange(n), per)
        fin = finals.astype(np.int64)
        a, b = self.anc[hits.target.astype(np.int64)], self.anc[fin[read_of]]
        d_i = np.cumprod(a == b, axis=1).sum(axis=1) - 1  # common prefix of the two root paths (depth 0 = the root, always common)
        nd = self.anc.shape[1]
        ge = np.zeros((n, nd), np.int64)  # ge[r, d] = #{i : d_i >= d}
        for d in range(nd):
            ge[:, d] = np.bincount(read_of[d_i >= d], minlength=n)
        out = np.zeros(n, SUPPORT_DTYPE)
        out["final"], out["n_kmers"], out["n_hits"] = finals, hits.n_kmers, per
        nk = hits.n_kmers.astype(np.int64)
        df = self.depth[fin]
        called = fin > 0
        out["s_final"] = np.where(called, ge[np.arange(n), np.where(called, df, 0)], 0)
        ok = (ge >= rule[0]) & (1000 * ge >= rule[1] * nk[:, None]) & (np.arange(nd)[None, :] <= df[:, None]) & called[:, None]
        deepest = nd - 1 - np.argmax(ok[:, ::-1], axis=1)  # the deepest depth that passes
        found = ok.any(axis=1)
        rows = np.flatnonzero(found)
        out["confident"][rows] = self.anc[fin[rows], deepest[rows]]
        out["s_confident"][rows] = ge[rows, deepest[rows]]
        return out

    # ---- a sample tallied with the records: gcount[confident]++ per counted read; the entries of the hits with target > 1
    # of counted reads with confident > 0 are seen, ucount[t] = seen entries of target t
    def tally(self, hits, rec, counted, entry_targets):
        ntar = self.parent.size
        g = np.bincount(rec["confident"][counted].astype(np.int64), minlength=ntar).astype(np.int64)
        per = np.diff(hits.offsets.astype(np.int64))
        read_of = np.repeat(np.arange(per.size), per)
        take = (counted & (rec["confident"] > 0))[read_of] & (hits.target > 1)
        seen = np.unique(hits.entry[take])
        u = np.bincount(np.asarray(entry_targets)[seen].astype(np.int64), minlength=ntar).astype(np.int64)
        return g, u


def result_text(g, u):
    """the result file's format: ntar lines of i,reads,unique_kmers"""
    return "".join("%d,%d,%d\n" % (i, int(g[i]), int(u[i])) for i in range(len(g)))
