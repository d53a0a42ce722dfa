"""What the tests of kid_pileup_* share: site tables, synthetic kid_locus records and the model's answers.  numpy and the
models only; no GPU, no test functions.

Tables
  big      the site table of read_loci_cases.sites(): orgs 0, 5 and 2^24 - 1 (n_orgs = 2^24, nearly all of them empty),
           positions up to 2^31 - 1; widths BIG_WIDTHS.  At W = 1 it has more than 2^28 bins.
  small(x) N_SMALL entries, four organisms: 0 and 1 with one entry each at position 0 (one bin each at every width: they
           are neighbours in the slot layout, a step that leaks past a sentinel shows in the other), 2 without an entry
           (span_bins 0), 3 with entries at 300 positions from 0 to x - 1 (span_bins x at W = 1).  small(300) is "the
           second table"; scan_table(n) is the small(x) whose B + n_orgs is n at W = 1.
Records (edge_records): every combination of what the rule looks at, drawn by a seeded generator and checked for coverage by
  tests/test_read_pileup_model.py; hot_spot and uniform are the two shapes of 100 000 records.
"""
import functools

import numpy as np

import read_loci_cases as lc
import read_loci_model as lm
import read_pileup_model as pm
from read_calls import header_constant

SCAN_TILE = header_constant("kid_pileup.hip.h", "KID_PILEUP_SCAN_TILE")
K = lc.K
BIG_WIDTHS = [4096, 65536, 2 ** 31 - 1]
SMALL_WIDTHS = [1, 7]
N_SMALL = 302
RULE = (3, 2)  # (min_chain, min_margin) of the edge records
U32 = 2 ** 32 - 1
SCAN_SLOTS = [SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, SCAN_TILE * SCAN_TILE + 1]
COUNTS = [0, 1, 63, 64, 65, 257]


@functools.lru_cache(maxsize=None)
def big():
    return lc.sites()


@functools.lru_cache(maxsize=None)
def small(x=300):
    """-> org, pos: uint32[N_SMALL]"""
    assert x >= 300
    p3 = np.unique(np.linspace(0, x - 1, 300).astype(np.int64))
    assert p3.size == 300 and p3[0] == 0 and p3[-1] == x - 1
    org = np.concatenate([[0, 1], np.full(300, 3)]).astype(np.uint32)
    pos = np.concatenate([[0, 0], p3]).astype(np.uint32)
    return org, pos


def scan_table(n_slots):
    """the small table with B + n_orgs = n_slots at W = 1: B = 1 + 1 + 0 + x, n_orgs = 4"""
    return small(n_slots - 6)


def locus(org, strand, n_chain, n_other, pos_first, pos_last, entry_first, n_org=None):
    r = np.zeros(1, lm.LOCUS_DTYPE)[0]
    r["org"], r["strand"], r["n_chain"], r["n_other"] = org, strand, n_chain, n_other
    r["n_org"] = n_chain if n_org is None else n_org
    r["n_hits"] = r["n_kmers"] = max(n_chain, 1)
    r["pos_first"], r["pos_last"], r["entry_first"] = pos_first, pos_last, entry_first
    return r


def edge_records(org, pos, n, seed, whole_span=4, d_max=20000):
    """n records over the table (org, pos), each field drawn from the values at which the rule changes its mind.  d beyond
    d_max (the model walks every bin of a record) only in 2 * whole_span records that span their organism's whole span."""
    rng = np.random.default_rng([seed, n, org.size])
    mc = RULE[0]
    ne = org.size
    out = np.zeros(n, lm.LOCUS_DTYPE)
    last_of = {int(g): int(np.flatnonzero(org == g)[np.argmax(pos[org == g])]) for g in np.unique(org)}
    first_of = {int(g): int(np.flatnonzero(org == g)[np.argmin(pos[org == g])]) for g in np.unique(org)}
    for i in range(n):
        n_chain = int(rng.choice([mc - 1, mc, mc + 1, mc + 1, 40, 40]))
        n_other = int(rng.choice([0, 0, n_chain - RULE[1] - 1, n_chain - RULE[1], n_chain - RULE[1] + 1, n_chain, n_chain + 1]))
        n_other = max(n_other, 0)
        strand = int(rng.choice([0, 0, 0, 1, 1, 1, 2]))
        e = int(rng.choice([int(rng.integers(0, ne)), int(rng.integers(0, ne)), int(rng.integers(0, ne)), ne - 1, 0, ne, U32]))
        g = int(org[e]) if e < ne else int(org[0])
        if rng.random() < 0.08:  # an org that disagrees with the entry's
            g = int(rng.choice([x for x in (0, 1, 2, 3, 5, int(org.max())) if x != g]))
        first = int(rng.choice([0, 0, 10, 17, U32 - 300, U32]))
        kind = int(rng.integers(0, 6))
        if kind == 0:
            last = first  # d = 0
        elif kind == 1:
            last = first - int(rng.integers(1, 50)) if first > 50 else first + 3  # pos_last < pos_first: d = 0
        elif kind == 2 and e < ne:  # on the reverse strand lo = 0 exactly, or below 0 before the max
            last = first + int(pos[e]) + int(rng.choice([0, 1, 5]))
        elif kind == 3 and e < ne:  # hi in the organism's last bin exactly, or past the span
            d = int(pos[last_of[g if g in last_of else int(org[e])]]) - int(pos[e]) - (K - 1) + int(rng.choice([0, 0, 1, 40]))
            last = first + max(d, 0)
        else:
            last = first + int(rng.integers(0, d_max))
        last = min(max(last, 0), U32)
        if last - first > d_max and kind not in (2, 3):
            last = first + d_max
        if last - first > d_max:  # (kinds 2 and 3 on a table with far-apart positions: keep the walk short)
            last = first + int(rng.integers(0, d_max))
        out[i] = locus(g, strand, n_chain, n_other, first, last, e)
    placed_orgs = [int(g) for g in np.unique(org)]
    j = 0
    for g in placed_orgs[-2:]:
        for w in range(whole_span):  # a chain that spans its organism's whole span: reverse from its last entry down to 0 (or below)
            out[(j * 37 + 5) % n] = locus(g, 1, 40, 0, 3, 3 + int(pos[last_of[g]]) + (0 if w % 2 == 0 else 77), last_of[g])
            j += 1
        # forward from its first entry with hi = its last entry's position: b_hi is exactly the organism's last bin, unclamped
        out[(j * 37 + 5) % n] = locus(g, 0, 40, 0, 0, max(int(pos[last_of[g]]) - int(pos[first_of[g]]) - (K - 1), 0), first_of[g])
        j += 1
    out[(j * 37 + 5) % n] = locus(int(org[0]), 0, 40, 0, 0, U32, 0)  # pos_first 0, pos_last 2^32 - 1: hi clamps
    out[((j + 1) * 37 + 5) % n] = locus(int(org[ne - 1]), 1, 40, 0, 0, U32, ne - 1)
    return out


def hot_spot(org, pos, n=100000, entry=150):
    """n records all in one bin of one organism (the bin of `entry`), a few that are not placed among them"""
    out = np.zeros(n, lm.LOCUS_DTYPE)
    out[:] = locus(int(org[entry]), 0, 9, 1, 5, 5, entry)
    out["strand"][::1000] = 2
    out["n_chain"][7::5000] = 1
    return out


def uniform(org, pos, n=100000, seed=9, d_max=40):
    """n records spread uniformly over the entries, both strands, short chains"""
    rng = np.random.default_rng([seed, n])
    out = np.zeros(n, lm.LOCUS_DTYPE)
    e = rng.integers(0, org.size, n)
    out["org"], out["entry_first"] = org[e], e
    out["strand"] = rng.integers(0, 2, n)
    out["n_chain"] = out["n_org"] = out["n_hits"] = out["n_kmers"] = rng.integers(2, 60, n)
    out["n_other"] = rng.integers(0, 3, n)
    out["pos_first"] = rng.integers(0, 100, n)
    out["pos_last"] = out["pos_first"] + rng.integers(0, d_max, n).astype(np.uint32)
    return out


class Expected:
    """the model's answer for a list of records on a table under a width and a rule, and the step form derived from it"""

    def __init__(self, loci, org, pos, w, rule=RULE):
        self.n_records = loci.size
        self.bin_base, self.starts, self.depth, self.records, self.n_placed = pm.batch(loci, org, pos, K, w, rule[0], rule[1])
        self.span = np.diff(self.bin_base.astype(np.int64))

    @functools.cached_property
    def steps(self):
        """the step array whose running sum is self.depth: per organism the differences of depth, the sentinel closing them"""
        n_orgs = self.span.size
        out = np.zeros(self.depth.size + n_orgs, np.uint32)
        for g in np.flatnonzero(self.span).tolist():
            a, n = int(self.bin_base[g]), int(self.span[g])
            d = np.concatenate([[0], self.depth[a:a + n].astype(np.int64), [0]])
            out[a + g:a + g + n + 1] = (np.diff(d) % 2 ** 32).astype(np.uint32)
        return out


@functools.lru_cache(maxsize=None)
def big_case(w):
    org, pos = big()
    loci = edge_records(org, pos, 400, 21, whole_span=2)
    return loci, Expected(loci, org, pos, w)


@functools.lru_cache(maxsize=None)
def small_case(w, x=300, n=400):
    org, pos = small(x)
    loci = edge_records(org, pos, n, 22, whole_span=4 if x <= 100000 else 1, d_max=min(2 * x, 20000))
    return loci, Expected(loci, org, pos, w)


@functools.lru_cache(maxsize=None)
def shape_case(shape, w):
    org, pos = small()
    loci = hot_spot(org, pos) if shape == "hot_spot" else uniform(org, pos)
    return loci, Expected(loci, org, pos, w, (2, 1))
