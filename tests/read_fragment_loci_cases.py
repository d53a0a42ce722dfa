"""What the tests of kid_db_read_fragment_loci* share: synthetic interleaved hit lists over the site table of
read_loci_cases (three blocks of entries: A org 5 with pos 1000 + e, B org 2^24 - 1 with pos falling from 2^31 - 1, C org 0
with random pos), and the model's records of each under every rule.  numpy and the models only; no GPU, no test functions.

A fragment of the lists is (m_1, m_2, shape):
  proper        a forward chain in one mate and a reverse chain in the other on one org (A or B), E - D drawn from values
                around the rules' reach; one hit in ten is noise, uniform over the table
  two_orgs      the same on A and on B at once, half of each mate's hits on either: equal scores on two orgs when even
  uniform       read positions in [0, 300) or up to 2^32 - 1, entries uniform over the table
  one_chain     every hit of a mate on one forward diagonal of A; the mates' diagonals are unrelated
The pairs (m_1, m_2) cover 0, 1 and 2 hits, the edge of the lane regime +- 1 in either mate (every combination), 63 to 65,
a few hundred, 4095 to 4097 and 5000 against 1; the fragments of thousands of hits are proper chains (a chain of n hits
repeats its 1000 (pos, entry) pairs) or meet a small mate, so that the model stays quick.  HAND is a list of fragments
made by hand, each for one property (hand_made() says which); RULES the (W, max_span) the tests run under.
"""
import functools

import numpy as np

import read_fragment_loci_model as fm
import read_loci_cases as lc
from read_calls import header_constant
from read_hits_model import Hits
from read_support_cases import random_keys

LANE_HITS = header_constant("kid_fragment_loci.hip.h", "KID_FLOCI_LANE_HITS")
MAX_HITS = lc.MAX_HITS
assert MAX_HITS == fm.MAX_HITS == 4096 and 2 <= LANE_HITS < 60
K = lc.K
N_A, N_B, N_ENTRIES = lc.N_A, lc.N_B, lc.N_ENTRIES
ORG_A, ORG_B = lc.ORG_A, lc.ORG_B
R_MAX = 2 ** 32 - 1
X_B = 2 ** 31 - 1  # pos of B's first entry
BIG_W = 2 ** 31 - 1
RULES = [(1, 1000), (7, 1000), (1, 0), (7, 50), (BIG_W, BIG_W)]
CHAIN = 1000  # the distinct (pos, entry) pairs of a chain

_EDGE = [0, 1, 2, LANE_HITS - 1, LANE_HITS, LANE_HITS + 1]
SMALL = sorted({(a, b) for a in _EDGE for b in _EDGE})
MEDIUM = [(63, 64), (64, 65), (65, 3), (3, 65), (300, 200), (2 * LANE_HITS, 2 * LANE_HITS + 1), (0, 70), (70, 0)]
BIG = [(4095, 4096, "proper"), (4096, 4097, "proper"), (4097, 4095, "proper"), (4096, 4096, "two_orgs"), (5000, 1, "uniform"), (1, 5000, "uniform"),
       (4096, LANE_HITS + 2, "uniform"), (LANE_HITS + 2, 4097, "uniform"), (0, 4097, "one_chain"), (4096, 0, "one_chain"), (4095, 2, "proper")]
SHAPES = ("proper", "two_orgs", "uniform", "one_chain")
DELTAS = [0, 1, 7, 49, 50, 51, 56, 57, 300, 993, 994, 999, 1000, 1001, 1007, 5000]  # E - D of a proper pair, in bases


def _empty():
    return np.empty(0, np.int64), np.empty(0, np.int64)


def _cat(parts):
    return np.concatenate([p[0] for p in parts] + [np.empty(0, np.int64)]), np.concatenate([p[1] for p in parts] + [np.empty(0, np.int64)])


def chain(n, org, reverse, diag, r0):
    """n hits of one mate on the diagonal `diag` (x - r forward, x + r reverse) of org A or B, read positions from r0 on
    -> pos, entry; None when the table has no such entries"""
    if n == 0:
        return _empty()
    i = np.arange(n, dtype=np.int64) % CHAIN
    if org == ORG_A:  # x = 1000 + e
        r = r0 + (CHAIN - 1 - i if reverse else i)
        e = (diag - r if reverse else diag + r) - 1000
        lo, hi = 0, N_A
    else:  # x = X_B - (e - N_A)
        r = r0 + (i if reverse else CHAIN - 1 - i)
        e = N_A + X_B - (diag - r if reverse else diag + r)
        lo, hi = N_A, N_A + N_B
    if e.min() < lo or e.max() >= hi or r.min() < 0 or r.max() > R_MAX:
        return None
    return r, e


def noise(rng, n, far=False):
    return rng.integers(0, R_MAX + 1 if far else 300, n), rng.integers(0, N_ENTRIES, n)


def proper(rng, m1, m2, org):
    """a forward chain in mate 1 + o and a reverse chain in the other, E - D from DELTAS; a tenth of the hits noise"""
    for _ in range(100):
        o = int(rng.integers(0, 2))
        mf, mr = (m1, m2) if o == 0 else (m2, m1)
        nf, nr = mf - mf // 10, mr - mr // 10
        if org == ORG_A:
            D = int(rng.integers(1000, 1000 + N_A - 2 * CHAIN))
            rf = int(rng.integers(0, 50))
        else:
            D = int(rng.integers(X_B - 1550, X_B - 1050))
            rf = int(rng.integers(0, 50))
        E = D + int(DELTAS[int(rng.integers(0, len(DELTAS)))])
        f, r = chain(nf, org, False, D, rf), chain(nr, org, True, E, int(rng.integers(0, 50)))
        if f is None or r is None:
            continue
        f, r = _cat([f, noise(rng, mf - nf)]), _cat([r, noise(rng, mr - nr)])
        return (f, r) if o == 0 else (r, f)
    raise AssertionError("no proper pair of (%d, %d) hits on org %d" % (m1, m2, org))


def fragment(rng, m1, m2, shape):
    """-> (pos, entry) of mate 1, (pos, entry) of mate 2: int64 arrays of m1 and m2 elements, in a seeded order"""
    if shape == "proper":
        a, b = proper(rng, m1, m2, ORG_A if rng.integers(0, 2) else ORG_B)
    elif shape == "two_orgs":
        (a1, b1), (a2, b2) = proper(rng, m1 // 2, m2 // 2, ORG_A), proper(rng, m1 - m1 // 2, m2 - m2 // 2, ORG_B)
        a, b = _cat([a1, a2]), _cat([b1, b2])
    elif shape == "uniform":
        far = bool(rng.integers(0, 4) == 0)
        a, b = noise(rng, m1, far), noise(rng, m2, far)
    else:
        a = chain(m1, ORG_A, False, int(rng.integers(1000, 3000)), int(rng.integers(0, 20)))
        b = chain(m2, ORG_A, False, int(rng.integers(1000, 3000)), int(rng.integers(0, 20)))
    out = []
    for (r, e), m in ((a, m1), (b, m2)):
        assert r.size == m and e.size == m
        p = rng.permutation(m)
        out.append((r[p], e[p]))
    return out


def hand_made():
    """-> [(name, mate 1, mate 2)] with a mate a list of (pos, entry); entry e < N_A lies at 1000 + e on org 5"""
    b = lambda j: N_A + j  # noqa: E731  (entry j of B: pos X_B - j)
    c = lc.sites()[1]
    out = [
        # the worked case's shape: two forward hits of mate 1 on D = 1090, a hit on another org, mate 2 reverse at E = 1460 and far away
        ("worked", [(10, 100), (40, 130), (5, N_A + N_B + 3)], [(60, 400), (20, 4000)]),
        ("one_hit_each", [(10, 100)], [(60, 400)]),
        # D = 4000 forward in mate 1 above E = 2500 reverse in mate 2: D > E; the other orientation (D = 2440, E = 4060) is
        # 1620 bases apart, beyond every max_span here but the last rule's
        ("D_above_E", [(30, 3030)], [(30, 1470)]),
        # a paired and a solo placement of equal score: two hits on D = 4000 (no partner: every E is below), one on D = 1090
        # with mate 2's E = 1460
        ("pair_and_solo_tie", [(0, 3000), (1, 3001), (10, 100)], [(60, 400)]),
        # equal scores on two orgs: a pair on A and a pair on B
        ("two_orgs_tie", [(10, 100), (CHAIN, b(500))], [(60, 400), (30, b(300))]),
        # mate 2 alone, mate 1 alone, both without a participant
        ("absent_1", [], [(3, 200), (4, 201), (9, 700)]),
        ("absent_2", [(3, 200), (4, 201), (9, 700)], []),
        ("no_participant", [(3, N_ENTRIES), (4, 0xFFFFFFFF)], [(9, N_ENTRIES + 5)]),
        ("outside_and_inside", [(3, N_ENTRIES), (10, 100)], [(9, 0xFFFFFFFF), (60, 400)]),
        # the largest coordinates: org 2^24 - 1, sites 2^31 - 1 and 2^31 - 2, read positions 2^31 and 2^32 - 3.  Under W =
        # 2^31 - 1 both hits of mate 1 have the forward diagonal -1 and hi = 2^31 - 1 + 2^31 - 3 + k - 1 saturates
        ("saturate", [(2 ** 31, b(0)), (R_MAX - 2, b(1))], [(R_MAX, b(0))]),
        ("largest_pos", [(R_MAX, b(0)), (R_MAX, 0)], [(R_MAX, b(0)), (0, N_A + N_B + 1)]),
    ]
    assert int(c[N_A + N_B + 1]) == 2 ** 31 - 1
    # the partner exactly at max_span and one base beyond, for every rule: mate 1 forward at x = 1100, r = 10 (1090 in bases)
    for w, s in RULES[:4]:
        D = 1090 // w
        at, beyond = (D + s // w) * w + w - 1, (D + s // w + 1) * w  # the largest x + r with E = D + reach, the smallest behind it
        for name, total in (("at", at), ("beyond", beyond)):
            out.append(("%s_%d_%d" % (name, w, s), [(10, 100)], [(90, total - 90 - 1000)]))
            out.append(("%s_%d_%d_swapped" % (name, w, s), [(90, total - 90 - 1000)], [(10, 100)]))
    return out


def lists(seed=7):
    """-> Hits of the interleaved reads (2 per fragment), [(m1, m2, shape or the hand-made name)] per fragment"""
    rng = np.random.default_rng([seed, 2])
    what = [(a, b, SHAPES[int(rng.integers(0, len(SHAPES)))]) for a, b in SMALL for _ in range(2)]
    what += [(a, b, s) for a, b in MEDIUM for s in ("proper", "uniform")] + BIG
    what = [what[int(i)] for i in rng.permutation(len(what))]
    mates = [fragment(rng, a, b, s) for a, b, s in what]
    for name, h1, h2 in hand_made():
        what.append((len(h1), len(h2), name))
        mates.append([(np.array([h[0] for h in h], np.int64), np.array([h[1] for h in h], np.int64)) for h in (h1, h2)])
    ms = np.array([m for a, b, s in what for m in (a, b)], np.int64)
    nk = np.choose(rng.integers(0, 4, ms.size), [ms, ms + 91, 0 * ms, 0 * ms + 2 ** 32 - 1]).astype(np.uint32)
    off = np.zeros(ms.size + 1, np.uint64)
    off[1:] = np.cumsum(ms)
    pos = np.concatenate([m[0] for f in mates for m in f]).astype(np.uint32)
    entry = np.concatenate([m[1] for f in mates for m in f]).astype(np.uint32)
    target = (1 + np.arange(pos.size) % 7).astype(np.uint32)
    return Hits(off, nk, pos, target, entry), what


def big_fragments(n=300, seed=5):
    """list `A` of the two-stream test: n fragments, every one for the second kernel, uniform over the table"""
    rng = np.random.default_rng([seed, n])
    ms = np.stack([LANE_HITS + 1 + np.arange(n) % 40, np.arange(n) % 7], 1).reshape(-1)
    off = np.zeros(2 * n + 1, np.uint64)
    off[1:] = np.cumsum(ms)
    total = int(off[-1])
    return Hits(off, ms.astype(np.uint32), rng.integers(0, 300, total).astype(np.uint32), np.ones(total, np.uint32),
                rng.integers(0, N_ENTRIES, total).astype(np.uint32))


class Case:
    """the site table, the lists, their variants, and the model's records of each under every rule, made when first asked for"""

    def __init__(self, seed=7):
        self.org, self.pos = lc.sites()
        self.hits, self.what = lists(seed)
        self.n_fragments = len(self.what)
        self.keys = random_keys(np.random.default_rng([3, 17]), N_ENTRIES)  # the table behind the sites
        self.targets = (1 + np.arange(N_ENTRIES) % 7).astype(np.uint32)
        self._memo = {}

    def index(self, name):
        return [s for a, b, s in self.what].index(name)

    @functools.cached_property
    def shuffled(self):
        from hit_list_cases import shuffled
        return shuffled(self.hits, 3)

    @functools.cached_property
    def out_of_range(self):
        return lc.out_of_range(self.hits)

    @functools.cached_property
    def big(self):
        return big_fragments()

    def expected(self, variant, rule):
        if (variant, rule) not in self._memo:
            self._memo[variant, rule] = fm.batch(getattr(self, variant), self.org, self.pos, K, rule[0], rule[1])
        return self._memo[variant, rule]


@functools.lru_cache(maxsize=None)
def case():
    return Case()
