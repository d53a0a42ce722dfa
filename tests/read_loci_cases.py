"""What the tests of kid_db_read_loci* share: the genome world with its sites, and the synthetic hit lists with their site
table for kid_db_loci_from_hits_device.  numpy, the oracle and the models only; no GPU, no test functions.

The genome world (LociWorld): two random genomes of 3000 bases, every `every`-th window of each an entry of the database;
the sites are org = the genome's index and pos = the window's start.  SEED is the first seed whose genomes hold no
canonical 30-mer twice (LociWorld asserts it), so a stretch of a genome hits exactly its own windows.

The synthetic site table (SITES): three blocks of entries
  A  [0, 5200)      org 5          pos 1000 + e               a genome whose windows are consecutive entries
  B  [5200, 7800)   org 2^24 - 1   pos 2^31 - 1 - (e - 5200)  the largest org, the largest pos, descending
  C  [7800, 8192)   org 0          pos random, 0 and 2^31 - 1 among them
The lists (lists()): one read for every m of M_VALUES and every shape of SHAPES, in a seeded order; n_kmers from
{m, m + 91, 0, 2^32 - 1}; read positions up to 2^32 - 1.
"""
import functools

import numpy as np

import read_loci_model as lm
from helpers import concat_reads
from kmer_id_amd import synth
from read_calls import World, genome_world, header_constant, revcomp
from read_hits_model import Hits, windows
from read_support_cases import random_keys

LANE_HITS = header_constant("kid_loci.hip.h", "KID_LOCI_LANE_HITS")
WAVE_HITS = header_constant("kid_loci.hip.h", "KID_LOCI_WAVE_HITS")
MAX_HITS = header_constant("kid_loci.hip.h", "KID_LOCI_MAX_HITS")
assert MAX_HITS == lm.MAX_HITS == 4096 and LANE_HITS < 63 and 65 < WAVE_HITS < 4095

K = 30
SEED = 1
GENOME_LEN = 3000
WIDTHS = [1, 7, 2 ** 31 - 1]

# ------------------------------------------------------------------ the genome world


class LociWorld(World):
    """two genomes, the database of every `every`-th window of each, its sites, and reads cut from them:
    reads[i] = (kind, sequence, what the read is: (genome, a, L) or for a chimera ((gA, a, LA), (gB, b, LB)))"""

    def __init__(self, every, seed=SEED):
        parent, _ = synth.load_taxonomy("bact10")
        rng = np.random.default_rng([seed, 3000])
        self.every = every
        self.genomes, keys, targets, org, pos = [], [], [], [], []
        every_window = []
        for gi in range(2):
            g, _, _ = genome_world(rng, [8, 6, 5, 36, 35], GENOME_LEN, 1)
            k_all, p_all = windows(g, 0, GENOME_LEN - 1, K)
            assert np.array_equal(p_all, np.arange(GENOME_LEN - K + 1))
            every_window.append(k_all)
            self.genomes.append(g)
            keys.append(k_all[::every])
            targets.append(np.array([8, 6, 5, 36, 35], np.uint32)[rng.integers(0, 5, keys[-1].size)])
            org.append(np.full(keys[-1].size, gi, np.uint32))
            pos.append(p_all[::every].astype(np.uint32))
        # no canonical 30-mer twice, within a genome or between the two: a stretch hits its own windows and no other
        assert np.unique(np.concatenate(every_window)).size == 2 * (GENOME_LEN - K + 1), "pick another SEED"
        self.org, self.pos = np.concatenate(org), np.concatenate(pos)
        self.reads = self._reads(np.random.default_rng([seed, every, 5]))
        bases, off = concat_reads([r[1] for r in self.reads])
        World.__init__(self, parent, np.concatenate(keys), np.concatenate(targets), bases, off, 14)

    def _reads(self, rng):
        out = []
        cut = lambda gi, a, n: self.genomes[gi][a:a + n]  # noqa: E731
        for i in range(40):
            gi, n = int(rng.integers(0, 2)), int(rng.integers(60, 260))
            a = int(rng.integers(0, GENOME_LEN - n))
            out.append(("forward", cut(gi, a, n), (gi, a, n)))
            out.append(("reverse", revcomp(cut(gi, a, n)), (gi, a, n)))
        for i in range(20):
            na, nb = int(rng.integers(60, 140)), int(rng.integers(60, 140))
            a, b = int(rng.integers(0, GENOME_LEN - na)), int(rng.integers(0, GENOME_LEN - nb))
            ga = int(rng.integers(0, 2))
            out.append(("chimera", cut(ga, a, na) + cut(1 - ga, b, nb), ((ga, a, na), (1 - ga, b, nb))))
        for n in (0, 1, 29):
            out.append(("short", cut(0, 100, n), (0, 100, n)))
        out.append(("forward", cut(1, 0, 400), (1, 0, 400)))  # more than KID_LOCI_WAVE_HITS hits when every = 1
        out.append(("reverse", revcomp(cut(0, 2500, 500)), (0, 2500, 500)))
        order = rng.permutation(len(out))
        return [out[int(i)] for i in order]

    def own_windows(self, gi, a, n):
        """the database windows that lie in [a, a + n) of genome gi: their starts"""
        p = np.arange(0, GENOME_LEN - K + 1, self.every)
        return p[(p >= a) & (p + K <= a + n)]


@functools.lru_cache(maxsize=None)
def world(every):
    return LociWorld(every)


# ------------------------------------------------------------------ the synthetic lists
N_A, N_B, N_ENTRIES = 5200, 2600, 8192
ORG_A, ORG_B, ORG_C = 5, 2 ** 24 - 1, 0
M_VALUES = [0, 1, 2, LANE_HITS - 1, LANE_HITS, LANE_HITS + 1, 63, 64, 65, WAVE_HITS - 1, WAVE_HITS, WAVE_HITS + 1, 4095, 4096, 4097, 5000]
SHAPES = ("one_chain", "two_chains", "one_org_distinct", "uniform", "forward_reverse")
N_READS = len(M_VALUES) * len(SHAPES)
R_MAX = 2 ** 32 - 1


def sites(seed=3):
    """-> org, pos: uint32[N_ENTRIES]"""
    rng = np.random.default_rng([seed, N_ENTRIES])
    e = np.arange(N_ENTRIES, dtype=np.int64)
    org = np.where(e < N_A, ORG_A, np.where(e < N_A + N_B, ORG_B, ORG_C)).astype(np.uint32)
    pos = np.where(e < N_A, 1000 + e, 2 ** 31 - 1 - (e - N_A))
    c = rng.integers(0, 2 ** 31, N_ENTRIES - N_A - N_B)
    c[0], c[1] = 0, 2 ** 31 - 1
    pos[N_A + N_B:] = c
    assert pos.min() == 0 and pos.max() == 2 ** 31 - 1
    return org, pos.astype(np.uint32)


def _chain_a(rng, n, reverse=False):
    """n hits on one diagonal of org A: forward (x - r the same) or reverse (x + r the same); r up to 2^32 - 1 now and then"""
    if n == 0:
        return np.empty(0, np.int64), np.empty(0, np.int64)
    a = int(rng.integers(0, N_A - n + 1))
    i = np.arange(n, dtype=np.int64)
    r0 = int([0, 17, R_MAX - (n - 1)][int(rng.integers(0, 3))])
    return (r0 + n - 1 - i if reverse else r0 + i), a + i


def _chain_b(rng, n, reverse):
    """the same on org B, whose pos falls with the entry"""
    if n == 0:
        return np.empty(0, np.int64), np.empty(0, np.int64)
    n = min(n, N_B)
    b = int(rng.integers(0, N_B - n + 1))
    i = np.arange(n, dtype=np.int64)
    r0 = int([0, 1000, R_MAX - (n - 1)][int(rng.integers(0, 3))])
    return (r0 + i if reverse else r0 + n - 1 - i), N_A + b + i


def _read(rng, shape, m):
    """-> pos int64[m], entry int64[m]"""
    if shape == "one_chain":
        r, e = _chain_a(rng, m)
    elif shape == "two_chains":  # equal sizes on two orgs (B's chain as long as B allows), a hit on C when m is odd
        ra, ea = _chain_a(rng, m // 2)
        rb, eb = _chain_b(rng, m // 2, bool(rng.integers(0, 2)))
        rc, ec = (np.array([5]), np.array([N_A + N_B + 7])) if m % 2 else (np.empty(0, np.int64), np.empty(0, np.int64))
        r, e = np.concatenate([ra, rb, rc]), np.concatenate([ea, eb, ec])
        if r.size < m:  # (m // 2 > N_B: the rest once more on A)
            r2, e2 = _chain_a(rng, m - r.size)
            r, e = np.concatenate([r, r2]), np.concatenate([e, e2])
    elif shape == "one_org_distinct":  # x - r = 1000 + a - 2 i and x + r = 1000 + a + 4 i: no two hits share a diagonal
        i = np.arange(m, dtype=np.int64)
        a = int(rng.integers(0, N_A - m + 1)) if m <= N_A else 0
        r, e = 3 * i, a + i
    elif shape == "uniform":
        r, e = rng.integers(0, 300, m), rng.integers(0, N_ENTRIES, m)
    else:  # forward and reverse chains of equal size on A, the odd hit on the forward one
        rf, ef = _chain_a(rng, m - m // 2)
        rr, er = _chain_a(rng, m // 2, reverse=True)
        r, e = np.concatenate([rf, rr]), np.concatenate([ef, er])
    assert r.size == m and e.size == m and (m == 0 or (r.min() >= 0 and r.max() <= R_MAX))
    p = rng.permutation(m)  # (list order is not read-position order here: only the first 4096 of a list take part)
    return r[p], e[p]


def lists(seed=3):
    """-> Hits of the N_READS reads (target = 1 + a running number: it plays no role), the (m, shape) drawn for each"""
    rng = np.random.default_rng([seed, N_READS])
    what = [(m, s) for m in M_VALUES for s in SHAPES]
    what = [what[int(i)] for i in rng.permutation(len(what))]
    reads = [_read(rng, s, m) for m, s in what]
    ms = np.array([m for m, s in what], np.int64)
    nk = np.choose(rng.integers(0, 4, N_READS), [ms, ms + 91, 0 * ms, 0 * ms + 2 ** 32 - 1]).astype(np.uint32)
    off = np.zeros(N_READS + 1, np.uint64)
    off[1:] = np.cumsum(ms)
    pos = np.concatenate([r for r, e in reads]).astype(np.uint32)
    entry = np.concatenate([e for r, e in reads]).astype(np.uint32)
    target = (1 + np.arange(pos.size) % 7).astype(np.uint32)
    return Hits(off, nk, pos, target, entry), what


def out_of_range(hits, seed=3):
    """a copy with a seeded 2 % of the entries replaced by N_ENTRIES, N_ENTRIES + 5 and 0xFFFFFFFF"""
    rng = np.random.default_rng([seed, 11])
    at = np.flatnonzero(rng.random(hits.entry.size) < 0.02)
    entry = hits.entry.copy()
    entry[at] = np.array([N_ENTRIES, N_ENTRIES + 5, 0xFFFFFFFF], np.uint32)[rng.integers(0, 3, at.size)]
    return Hits(hits.offsets, hits.n_kmers, hits.pos, hits.target, entry)


def big_reads(n=600, seed=5):
    """list `A` of the two-stream test: n reads of WAVE_HITS + 1 .. WAVE_HITS + 90 hits, uniform over the table"""
    rng = np.random.default_rng([seed, n])
    ms = WAVE_HITS + 1 + np.arange(n) % 90
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(ms)
    total = int(off[-1])
    return Hits(off, ms.astype(np.uint32), rng.integers(0, 300, total).astype(np.uint32), np.ones(total, np.uint32),
                rng.integers(0, N_ENTRIES, total).astype(np.uint32))


class Case:
    """the site table, the lists, their variants, and the model's records of each under every width, made when first asked for"""

    def __init__(self, seed=3):
        self.org, self.pos = sites(seed)
        self.hits, self.what = lists(seed)
        self.keys = random_keys(np.random.default_rng([seed, 17]), N_ENTRIES)  # the table behind the sites: N_ENTRIES entries
        self.targets = (1 + np.arange(N_ENTRIES) % 7).astype(np.uint32)
        self._memo = {}

    @functools.cached_property
    def shuffled(self):
        from hit_list_cases import shuffled
        return shuffled(self.hits, 3)

    @functools.cached_property
    def out_of_range(self):
        return out_of_range(self.hits)

    @functools.cached_property
    def big(self):
        return big_reads()

    def expected(self, variant, w):
        if (variant, w) not in self._memo:
            self._memo[variant, w] = lm.batch(getattr(self, variant), self.org, self.pos, w)
        return self._memo[variant, w]


@functools.lru_cache(maxsize=None)
def case():
    return Case()
