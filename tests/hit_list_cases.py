"""Seeded trees and synthetic hit lists for the kernels that read a hit CSR -- kid_support_kernel, kid_fragment_kernel,
kid_vote_kernel, kid_vote_big_kernel -- through their *_from_hits_device entry points, and the models' records of them.
numpy and the oracle's msca only; no GPU, no test functions (tests/test_hit_list_cases.py holds the cases to what they
must decide, tests/test_gpu_hit_lists.py hands them to the kernels).

Trees: `parent` arrays over the nodes 0 .. ntar - 1, node 1 the root.  A spine 2 -> 3 -> .. makes the stated depth exact;
beside its last inner node stands a second node of that depth, and three more deepest-level leaves hang under each of the
two (seven deepest-level nodes under two parents whatever else is drawn); every other node hangs under a random earlier
node that is not at the deepest level.

  rows8       300 nodes, depth 8   the deepest tree the ancestor rows hold
  climb9      300 nodes, depth 9   the first tree that climbs parent[]
  flat        201 nodes, depth 1   every tie resolves at the root
  wide_rows   65536 nodes, depth 4 the largest ntar with rows: hit targets of 32768 and more, 65535 among them
  wide_climb  65537 nodes, depth 4 one past the rows' limit

Lists: 204 reads per tree.  The numbers of hits m run twelve times, each time in another seeded order, through M_VALUES
(the edges of the kernels' three work splits: L = KID_VOTE_LANE_HITS = KID_SUPPORT_LANE_HITS, 64 = a tile, W =
KID_VOTE_WAVE_HITS); every read draws one of six shapes (SHAPES) and its n_kmers from {m, m + 91, 0, 1, 4294968, 2^32 - 1}:
1000 * 4294968 is 704 modulo 2^32, so under the rule (0, 1000) a read of few hits with that n is not confident, and a
32-bit product says it is.  Reads 2i and 2i + 1 are the mates of fragment i.  pos and entry count up: nothing here tallies.
"""
import functools

import numpy as np

from helpers import oracle_db
from read_calls import header_constant
from read_fragments_model import FRAGMENT_DTYPE, fragment_csr
from read_hits_model import HitModel, Hits
from read_support_cases import random_keys
from read_support_model import SupportModel
from read_votes_model import VoteModel

LANE_HITS = header_constant("kid_votes.hip.h", "KID_VOTE_LANE_HITS")
WAVE_HITS = header_constant("kid_votes.hip.h", "KID_VOTE_WAVE_HITS")

TREES = {"rows8": (300, 8), "climb9": (300, 9), "flat": (201, 1), "wide_rows": (65536, 4), "wide_climb": (65537, 4)}
M_VALUES = [0, 1, 2, LANE_HITS - 1, LANE_HITS, LANE_HITS + 1, 63, 64, 65, 127, 128, 129, WAVE_HITS - 1, WAVE_HITS, WAVE_HITS + 1,
            2 * WAVE_HITS, 5000]
N_CYCLES = 12
N_READS = N_CYCLES * len(M_VALUES)
WRAP_N = 4294968  # 1000 * WRAP_N = 2^32 + 704
RULES = [(0, 0), (3, 0), (2, 25), (0, 1000), (0, 1), (2 ** 32 - 1, 0)]
SHAPES = ("uniform", "one_path", "two_nodes", "one_deepest", "distinct", "deepest_only")
SEEDS = {"rows8": 3, "climb9": 3, "flat": 2, "wide_rows": 1, "wide_climb": 1}  # the first that meet tests/test_hit_list_cases.py
K = 30


def tree(name, seed):
    """-> parent int32[ntar], depth int64[ntar] (the root 0; node 0, which is no node, -1)"""
    ntar, max_depth = TREES[name]
    rng = np.random.default_rng([seed, ntar, max_depth])
    parent = np.ones(ntar, np.int32)
    depth = np.zeros(ntar, np.int64)
    depth[0] = -1
    v = 2
    for d in range(1, max_depth + 1):  # the spine: node d + 1 at depth d
        parent[v], depth[v] = (1 if d == 1 else v - 1), d
        v += 1
    if max_depth >= 2:
        last_inner = max_depth  # the spine's node at depth max_depth - 1
        parent[v], depth[v] = parent[last_inner], max_depth - 1
        second = v
        v += 1
        for p in (last_inner, second):
            for _ in range(3):
                parent[v], depth[v] = p, max_depth
                v += 1
    draws = rng.random(ntar)
    for x in range(v, ntar):
        p = 1 + int(draws[x] * (x - 1))  # an earlier node; the parent of one at the deepest level stands in for it
        if depth[p] == max_depth:
            p = int(parent[p])
        parent[x], depth[x] = p, depth[p] + 1
    assert int(depth.max()) == max_depth and np.all(parent[2:] < np.arange(2, ntar)) and np.all(parent[2:] >= 1)
    return parent, depth


def root_path(parent, c):
    path = [int(c)]
    while path[-1] != 1:
        path.append(int(parent[path[-1]]))
    return path


def _targets(rng, shape, m, parent, depth, deepest):
    ntar = parent.size
    if m == 0:
        return np.empty(0, np.uint32)
    if shape == "uniform":
        t = rng.integers(1, ntar, m)
    elif shape == "one_path":
        t = rng.choice(root_path(parent, deepest[int(rng.integers(0, deepest.size))]), m)
    elif shape == "two_nodes":
        a = int(rng.integers(2, ntar))
        sibs = np.flatnonzero(parent == parent[a])
        sibs = sibs[(sibs != a) & (sibs > 1)]
        b = int(sibs[int(rng.integers(0, sibs.size))]) if sibs.size and rng.random() < 0.5 else int(rng.integers(2, ntar))
        t = rng.permutation(np.array([a, b] * (m // 2) + [1] * (m % 2)))
    elif shape == "one_deepest":
        t = np.full(m, deepest[int(rng.integers(0, deepest.size))])
    elif shape == "distinct":
        t = np.resize(rng.permutation(np.arange(1, ntar)), m)  # min(m, ntar - 1) distinct nodes, then round again
    else:
        t = deepest[rng.integers(0, deepest.size, m)]
    return np.asarray(t, np.uint32)


def lists(name, seed):
    """-> Hits of the tree's N_READS reads, the shape drawn for each"""
    parent, depth = tree(name, seed)
    rng = np.random.default_rng([seed, parent.size, 7])
    deepest = np.flatnonzero(depth == depth.max())
    ms = np.concatenate([rng.permutation(M_VALUES) for _ in range(N_CYCLES)]).astype(np.int64)
    shapes = [SHAPES[int(i)] for i in rng.integers(0, len(SHAPES), N_READS)]
    tg = [_targets(rng, shapes[r], int(ms[r]), parent, depth, deepest) for r in range(N_READS)]
    which = rng.integers(0, 6, N_READS)
    nk = np.choose(which, [ms, ms + 91, 0 * ms, 0 * ms + 1, 0 * ms + WRAP_N, 0 * ms + 2 ** 32 - 1]).astype(np.uint32)
    off = np.zeros(N_READS + 1, np.uint64)
    off[1:] = np.cumsum(ms)
    target = np.concatenate(tg)
    if name.startswith("wide"):  # the last node, and the first of the upper half of the 16-bit ids, whatever was drawn
        r = int(np.flatnonzero(ms == 5000)[0])
        target[int(off[r])], target[int(off[r]) + 1] = parent.size - 1, 32768
    count = np.arange(target.size, dtype=np.uint32)
    return Hits(off, nk, count, target, count.copy()), shapes


def out_of_range(hits, ntar, seed):
    """a copy with a seeded 2 % of the targets replaced by 0, ntar and 0xFFFFFFFF -> (the copy, what the model sees: 1 there)"""
    rng = np.random.default_rng([seed, ntar, 11])
    at = np.flatnonzero(rng.random(hits.target.size) < 0.02)
    raw, seen = hits.target.copy(), hits.target.copy()
    raw[at] = np.array([0, ntar, 0xFFFFFFFF], np.uint32)[rng.integers(0, 3, at.size)]
    seen[at] = 1
    return Hits(hits.offsets, hits.n_kmers, hits.pos, raw, hits.entry), Hits(hits.offsets, hits.n_kmers, hits.pos, seen, hits.entry)


def shuffled(hits, seed):
    """every read's hits in a seeded random order, everything else the same"""
    rng = np.random.default_rng([seed, 13])
    idx = np.concatenate([int(hits.offsets[r]) + rng.permutation(int(hits.offsets[r + 1] - hits.offsets[r]))
                          for r in range(hits.offsets.size - 1)] + [np.empty(0, np.int64)]).astype(np.int64)
    return Hits(hits.offsets, hits.n_kmers, hits.pos[idx], hits.target[idx], hits.entry[idx])


def raw_hits(hits):
    """the kid_hit[] of a Hits: uint32[total, 3] = pos, target, entry"""
    return np.ascontiguousarray(np.stack([hits.pos, hits.target, hits.entry], 1).astype(np.uint32))


class Models:
    """the three models over one tree.  The table behind them holds a few dozen random keys: only the tree matters, and
    the oracle's msca over it is the fold."""

    def __init__(self, parent, seed):
        rng = np.random.default_rng([seed, parent.size, 17])
        self.parent = parent
        self.keys = random_keys(rng, 48)
        self.targets = rng.integers(1, parent.size, 48).astype(np.uint32)
        self.hm = HitModel(oracle_db(parent, self.keys, self.targets, 10), self.keys, self.targets, K)
        self.sm = SupportModel(self.hm, parent)
        self.vm = VoteModel(self.sm)

    def finals(self, hits):
        """-> the fold of every read, and of every fragment: mate 1's fold carried on over mate 2's hits"""
        f = self.sm.finals(hits)
        ff = np.array([self.hm.fold(([int(f[2 * i])] if f[2 * i] else []) + hits.of(2 * i + 1)[1].tolist()) for i in range(f.size // 2)], np.uint32)
        return f, ff

    def support(self, hits, rule, finals):
        return self.sm.batch_identity(hits, rule, finals)

    def votes(self, hits, rule, calls=None):
        return self.vm.batch_anc(hits, rule, calls)

    def fragments(self, hits, rule, finals, fragment_finals):
        """the record of FragmentModel.fragment for every pair, all pairs at once.  n = n_1 + n_2 is taken as the record
        holds it, in 32 bits (read_fragments_model.fragment_csr)"""
        s = self.sm.batch_identity(fragment_csr(hits), rule, fragment_finals)
        out = np.zeros(s.size, FRAGMENT_DTYPE)
        for f in s.dtype.names:
            out[f] = s[f]
        out["final_1"], out["final_2"] = finals[0::2], finals[1::2]
        return out


class Expected:
    """the records of one hit list under the rules asked for, computed when first asked for and kept"""

    def __init__(self, models, hits):
        self.models, self.hits = models, hits
        self.finals, self.fragment_finals = models.finals(hits)
        self.calls = models.vm.calls_anc(hits)
        self._memo = {}

    def _get(self, family, rule, make):
        if (family, rule) not in self._memo:
            self._memo[family, rule] = make()
        return self._memo[family, rule]

    def support(self, rule):
        return self._get("support", rule, lambda: self.models.support(self.hits, rule, self.finals))

    def votes(self, rule):
        return self._get("votes", rule, lambda: self.models.votes(self.hits, rule, self.calls))

    def fragments(self, rule):
        return self._get("fragments", rule, lambda: self.models.fragments(self.hits, rule, self.finals, self.fragment_finals))


class Case:
    """one tree with its models, its lists and their three variants"""

    def __init__(self, name, seed):
        self.name, self.seed = name, seed
        self.parent, self.depth = tree(name, seed)
        self.ntar, self.max_depth = TREES[name]
        self.models = Models(self.parent, seed)
        self.hits, self.shapes = lists(name, seed)
        self.plain = Expected(self.models, self.hits)

    @functools.cached_property
    def out_of_range(self):
        """-> (the list as the kernels get it, Expected of the list as the model sees it)"""
        raw, seen = out_of_range(self.hits, self.ntar, self.seed)
        return raw, Expected(self.models, seen)

    @functools.cached_property
    def shuffled(self):
        h = shuffled(self.hits, self.seed)
        return h, Expected(self.models, h)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name, SEEDS[name])


def big_reads(case_, n=2000, seed=5):
    """list `A` of the two-stream test: n reads of W + 1 .. W + 90 hits, uniform over the tree's nodes"""
    rng = np.random.default_rng([seed, n])
    ms = WAVE_HITS + 1 + np.arange(n) % 90
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(ms)
    target = rng.integers(1, case_.ntar, int(off[-1])).astype(np.uint32)
    count = np.arange(target.size, dtype=np.uint32)
    return Hits(off, ms.astype(np.uint32), count, target, count.copy())
