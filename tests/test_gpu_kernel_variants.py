"""Every instantiation of kid_classify_kernel<2, ROWS, HIST, MINLOC, KFIX, PAIRK> against the oracle, the dispatch limits
of kid_launch_classify at both sides, and the 16-bit workgroup histogram at the library's `span` cap.

Each case names the instantiation it is for and asserts that exactly that one ran (kid_sample_kernel_variants), so a
change of a limit or of the dispatch makes the case fail instead of quietly testing another kernel.  The axes:
  PAIRK   pair loop (1) for batches of <= 128 k-mers per read, duo loop (2) for <= 256, general loops (0) beyond;
          only the minimizer-localised table has the first two
  MINLOC  minimizer-localised table (k >= 24, GPU build, load <= 80 %) or the reference placement
  KFIX    30 for k = 30, else 0
  ROWS    ancestor rows (tree depth <= 8, ntar <= 65536) or the climb fallback
  HIST    gcount histogram in LDS (40 KiB per workgroup) or run-length + global atomics
Reads are cut from random genomes whose k-mers make the DB (targets walk one lineage, a few k-mers of a foreign one),
both strands, mutated copies and random reads in between; host batches put read starts on every byte offset mod 16."""
import numpy as np
import pytest

from kmer_id_amd import KID_FLAG_REF_GEOMETRY, KmerDB
from helpers import ob

pytestmark = pytest.mark.gpu

LOOPS = {1: "pair", 2: "duo", 0: "general"}
ML_VARIANTS = [(r, h, 1, kf, pk) for r in (1, 0) for h in (1, 0) for kf in (30, 0) for pk in (1, 2, 0)]
REF_VARIANTS = [(r, h, 0, kf, 0) for r in (1, 0) for h in (1, 0) for kf in (30, 0)]
ALL_VARIANTS = ML_VARIANTS + REF_VARIANTS
assert len(set(ALL_VARIANTS)) == 32
# k-mers per read for each loop (a host batch goes to the loop of its longest read)
NKS = {1: [1, 64, 65, 128], 2: [129, 256, 200], 0: [257, 961, 400], "ref": [1, 64, 128, 129, 256, 257, 961]}
# dispatch limits, derived from the LDS layout (KidWaveLds<>::total in kid_kernels.hip.h): (hist words + 8 waves *
# per-wave words) * 4 + 32 <= 40 KiB, hist words = ceil(ntar / 2) rounded up to 4 (two 16-bit counters) on the minimizer-localised table, ntar
# rounded up to 4 on the reference placement
PAIR_LDS_WORDS, GEN_ML_LDS_WORDS, WAVE_LDS_WORDS = 820, 792, 104
LIM_PAIR_HIST, LIM_GEN_ML_HIST, LIM_GEN_REF_HIST = 7344, 7792, 9400
LIM_UCOUNT_LDS, LIM_ROWS = 16384, 65536

ran = set()   # instantiations the matrix has seen, each matched against the oracle


def _words16(ntar):
    return ((ntar + 1) // 2 + 3) & ~3


def test_limits_follow_from_the_lds_layout():
    def fits(words):
        return words * 4 + 32 <= 40 * 1024
    for per_wave, lim, words in ((PAIR_LDS_WORDS, LIM_PAIR_HIST, _words16), (GEN_ML_LDS_WORDS, LIM_GEN_ML_HIST, _words16),
                                 (WAVE_LDS_WORDS, LIM_GEN_REF_HIST, lambda t: (t + 3) & ~3)):
        assert fits(words(lim) + 8 * per_wave) and not fits(words(lim + 1) + 8 * per_wave)
    assert LIM_UCOUNT_LDS * 4 <= 64 * 1024 < (LIM_UCOUNT_LDS + 1) * 4


# ------------------------------------------------------------------ synthetic DBs and reads
def taxonomy(ntar, deep, rng):
    """-> (parent, depth): a heap-shaped tree under root 1, fan-out 8 (depth <= 6 up to 65537 nodes: ancestor rows) or
    2 (depth > 8 from 512 nodes on: the climb fallback), its ids 2 .. ntar-1 shuffled (ancestors anywhere in the id
    range: ids >= 32768 in the 16-bit row fields)"""
    fan = 2 if deep else 8
    i = np.arange(ntar)
    hp = np.ones(ntar, np.int64)
    hp[2:] = (i[2:] - 2) // fan + 1
    depth = np.zeros(ntar, np.int64)
    for j in range(2, ntar):   # heap order: a parent comes before its children
        depth[j] = depth[hp[j]] + 1
    perm = np.arange(ntar)
    perm[2:] = 2 + rng.permutation(ntar - 2)
    parent = np.ones(ntar, np.int32)
    parent[perm[2:]] = perm[hp[2:]]
    d = np.zeros(ntar, np.int64)
    d[perm] = depth
    return parent, d


def genome_db(parent, depth, k, rng, n_genomes=48, genome_len=2400):
    """k-mers of random genomes.  Genome 0 carries target ntar-1 only (the last histogram counter); the others walk the
    lineage of a node at depth >= 3, with 2 % k-mers of foreign nodes (real LCAs)."""
    ntar = parent.size
    deep_nodes = np.flatnonzero(depth >= 3)
    nodes = np.flatnonzero(depth >= 1)
    code = np.zeros(256, np.uint64)
    for j, ch in enumerate(b"ACGT"):
        code[ch] = j
    genomes, keys, targets = [], [], []
    for g in range(n_genomes):
        seq = rng.choice(np.frombuffer(b"ACGT", np.uint8), genome_len)
        c = code[seq]
        nwin = genome_len - k + 1
        key = np.zeros(nwin, np.uint64)
        for j in range(k):
            key = (key << np.uint64(2)) | c[j:j + nwin]
        if g == 0:
            tg = np.full(nwin, ntar - 1, np.uint32)
        else:
            t0 = int(rng.choice(deep_nodes))
            lineage = [t0, int(parent[t0]), int(parent[int(parent[t0])])]
            tg = np.array(lineage, np.uint32)[rng.integers(0, 3, nwin)]
            foreign = rng.random(nwin) < 0.02
            tg[foreign] = rng.choice(nodes, int(foreign.sum())).astype(np.uint32)
        genomes.append(seq)
        keys.append(key)
        targets.append(tg)
    return genomes, np.concatenate(keys), np.concatenate(targets)


_COMP = np.zeros(256, np.uint8)
for _a, _b in zip(b"ACGTN", b"TGCAN"):
    _COMP[_a] = _b


def cut_reads(genomes, k, nks, n, rng):
    """n reads of nks[i % len(nks)] k-mers each: exact copies, reverse complements, copies with a substitution every
    ~25 bases, random reads; every eighth one from genome 0"""
    out = []
    acgt = np.frombuffer(b"ACGT", np.uint8)
    for i in range(n):
        L = nks[i % len(nks)] + k - 1
        kind = int(rng.integers(0, 4))
        if kind == 3:
            out.append(rng.choice(acgt, L))
            continue
        g = genomes[0 if i % 8 == 0 else int(rng.integers(0, len(genomes)))]
        p = int(rng.integers(0, g.size - L + 1))
        s = g[p:p + L].copy()
        if kind == 1:
            s = _COMP[s[::-1]]
        elif kind == 2:
            m = rng.random(L) < 0.04
            s[m] = rng.choice(acgt, int(m.sum()))
        out.append(s)
    return out


def ragged(reads, rng):
    """-> (bases, offsets): the reads back to back, with spacer reads of < 16 random bases (no k-mer) in between so
    that read i starts at byte offset 7 i mod 16"""
    acgt = np.frombuffer(b"ACGT", np.uint8)
    seqs, at = [], 0
    for i, r in enumerate(reads):
        pad = (7 * i - at) % 16
        if pad:
            seqs.append(rng.choice(acgt, pad))
            at += pad
        seqs.append(r)
        at += r.size
    data = np.concatenate(seqs)
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([s.size for s in seqs])
    return data, off


class Db:
    def __init__(self, k, flags, ntar, deep, seed):
        self.k, self.ntar = k, ntar
        self.rng = np.random.default_rng(seed)
        self.parent, depth = taxonomy(ntar, deep, self.rng)
        self.genomes, keys, targets = genome_db(self.parent, depth, k, self.rng)
        self.odb = ob.OracleDB(ntar, k, 18, parent=self.parent)
        self.odb.add(keys, targets)
        self.db = KmerDB(keys, targets, self.parent, k=k, log2_slots=18, flags=flags)
        info = self.db.info
        assert (info.tree_depth > 8) == deep and info.ntar == ntar

    def reads(self, nks, n):
        return cut_reads(self.genomes, self.k, nks, n, self.rng)

    def close(self):
        self.db.close()
        self.odb.close()


@pytest.fixture(scope="module")
def dbs():
    cache = {}

    def get(k, flags, ntar, deep):
        key = (k, flags, ntar, deep)
        if key not in cache:
            cache[key] = Db(k, flags, ntar, deep, seed=k * 1000003 + flags * 7919 + ntar * 2 + deep)
        return cache[key]
    yield get
    for d in cache.values():
        d.close()


def shape_of(r, h, m, kf):
    """(k, flags, ntar, deep) that selects ROWS r, HIST h, MINLOC m, KFIX kf"""
    if m:
        k, flags = (30, 0) if kf == 30 else ((31, 0) if r == h else (24, 0))
    else:
        k, flags = (30, KID_FLAG_REF_GEOMETRY) if kf == 30 else ((21, 0) if r == h else (31, KID_FLAG_REF_GEOMETRY))
    return k, flags, 3000 if h else 10000, not r


def oracle_run(d, data, off, os_=None):
    os_ = os_ or ob.OracleSample(d.odb)
    return os_, os_.classify(data, off)


def assert_counters(s, os_):
    g, u = s.end()
    eg, eu = os_.counts()
    assert np.array_equal(g, eg), "gcount differs from the oracle"
    assert np.array_equal(u, eu), "ucount differs from the oracle"
    st, est = s.stats(), os_.stats()
    assert st["lookups"] == est["lookups"] and st["hits"] == est["hits"], (st, est)
    return eg


def check_host_batch(d, nks, n, want):
    data, off = ragged(d.reads(nks, n), d.rng)
    os_, exp = oracle_run(d, data, off)
    s = d.db.sample()
    got = s.classify(data, off)
    assert s.kernel_variants() == want
    assert np.array_equal(got, exp), "final targets differ from the oracle in %d reads" % int((got != exp).sum())
    eg = assert_counters(s, os_)
    assert (exp > 1).sum() > n // 4 and os_.stats()["hits"] > n      # real hits and LCA folds
    s.close()
    return exp, eg


# ------------------------------------------------------------------ 1. the 32 instantiations
@pytest.mark.parametrize("variant", ALL_VARIANTS,
                         ids=["R%d-H%d-M%d-K%d-%s" % (r, h, m, kf, LOOPS[pk]) for r, h, m, kf, pk in ALL_VARIANTS])
def test_instantiation_vs_oracle(dbs, variant):
    r, h, m, kf, pk = variant
    k, flags, ntar, deep = shape_of(r, h, m, kf)
    d = dbs(k, flags, ntar, deep)
    assert d.db.info.geometry == m
    nks = NKS[pk] if m else NKS["ref"]
    check_host_batch(d, nks, 3000 if pk else 1500, {variant})
    ran.add(variant)


def test_union_of_the_matrix_is_every_instantiation():
    assert ran == set(ALL_VARIANTS), "instantiations not run (or failed): %s" % sorted(set(ALL_VARIANTS) - ran)


@pytest.mark.parametrize("rhk", [(r, h, kf) for r in (1, 0) for h in (1, 0) for kf in (30, 0)],
                         ids=lambda v: "R%d-H%d-K%d" % v)
def test_device_offsets_launch_all_three_loops(dbs, rhk):
    """classify_device (offsets the host never reads): the three loops of the configuration are launched, the device
    picks the one for the batch's longest read and the other two return at once.  Batches for each loop in turn on one
    sample, the last one of mixed lengths."""
    import torch
    r, h, kf = rhk
    d = dbs(*shape_of(r, h, 1, kf))
    s = d.db.sample()
    os_ = ob.OracleSample(d.odb)
    for nks, n in ((NKS[1], 2000), (NKS[2], 1000), ([1, 100, 129, 256, 257, 961, 30], 1400)):
        data, off = ragged(d.reads(nks, n), d.rng)
        _, exp = oracle_run(d, data, off, os_)
        d_b = torch.from_numpy(np.concatenate([data, np.zeros(64, np.uint8)])).cuda()
        d_o = torch.from_numpy(off.view(np.int64)).cuda()
        d_out = torch.full((off.size - 1,), -1, dtype=torch.int32, device="cuda")
        s.classify_device(d_b.data_ptr(), data.size, d_o.data_ptr(), off.size - 1, d_out=d_out.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(d_out.cpu().numpy().view(np.uint32), exp)
    assert s.kernel_variants() == {(r, h, 1, kf, pk) for pk in (0, 1, 2)}
    assert_counters(s, os_)
    s.close()


@pytest.mark.parametrize("pk", [1, 2, 0], ids=lambda v: LOOPS[v])
def test_fixed_layout_on_device_per_loop(dbs, pk):
    """classify_fixed_device: the host knows the one read length, only the loop for it is launched"""
    import torch
    d = dbs(*shape_of(1, 1, 1, 30))
    nk = {1: 128, 2: 129, 0: 257}[pk]
    n, L = 4000, nk + 29
    data = np.concatenate(d.reads([nk], n))
    os_, exp = oracle_run(d, data, np.arange(n + 1, dtype=np.uint64) * np.uint64(L))
    d_b = torch.from_numpy(np.concatenate([data, np.zeros(64, np.uint8)])).cuda()
    d_out = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    s = d.db.sample()
    s.classify_fixed_device(d_b.data_ptr(), L, n, d_out=d_out.data_ptr())
    torch.cuda.synchronize()
    assert s.kernel_variants() == {(1, 1, 1, 30, pk)}
    assert np.array_equal(d_out.cpu().numpy().view(np.uint32), exp)
    assert_counters(s, os_)
    assert (exp > 1).sum() > n // 4
    s.close()


# ------------------------------------------------------------------ 1b. the tapered shares at their edges
@pytest.mark.parametrize("n", [1, 7, 9, 17, 24, 65, 129, 1000])
@pytest.mark.parametrize("pk", [1, 2, 0], ids=lambda v: LOOPS[v])
def test_tapered_shares_at_their_edges(dbs, pk, n):
    """Batches of exactly n reads (no spacer reads) of one length per loop.  The grid has ceil(n / 8) workgroups, at most
    16 per CU: n = 1 .. 24 gives one, two and three of them, so the first half of the grid (the KID_TAPER shares) is
    empty or one workgroup and the grid is odd; an odd n ends a share of the pair loop on a phantom read; an n that is
    no multiple of 64 ends a wave on a partial block of results; 1000 reads leave waves at the end without any."""
    variant = (1, 1, 1, 30, pk)
    d = dbs(*shape_of(1, 1, 1, 30))
    nk = {1: 64, 2: 200, 0: 400}[pk]
    assert nk in NKS[pk]
    reads = d.reads([nk], n)
    data = np.concatenate(reads)                       # reads of nk + 29 bases: starts on every byte offset mod 16
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(nk + d.k - 1)
    os_, exp = oracle_run(d, data, off)
    s = d.db.sample()
    got = s.classify(data, off)
    assert s.kernel_variants() == {variant}
    assert got.size == n and np.array_equal(got, exp), "final targets differ from the oracle in %d reads" % int((got != exp).sum())
    assert_counters(s, os_)
    assert s.stats()["reads"] == n
    if n >= 17:
        assert os_.stats()["hits"] > n                 # real hits and LCA folds
    s.close()


# ------------------------------------------------------------------ 2. the dispatch limits, both sides
BOUNDARIES = [  # (name, last ntar inside, (k, flags), loops)
    ("pair_duo_hist", LIM_PAIR_HIST, (30, 0), (1, 2)),
    ("general_minloc_hist", LIM_GEN_ML_HIST, (30, 0), (0,)),
    ("general_refplace_hist", LIM_GEN_REF_HIST, (30, KID_FLAG_REF_GEOMETRY), (0,)),
    ("ucount_lds", LIM_UCOUNT_LDS, (30, 0), (1,)),
    ("rows", LIM_ROWS, (30, 0), (1,)),
]


@pytest.mark.parametrize("side", ["inside", "outside"])
@pytest.mark.parametrize("name,lim,kflags,loops", BOUNDARIES, ids=[b[0] for b in BOUNDARIES])
def test_dispatch_limit(dbs, name, lim, kflags, loops, side):
    """ntar at the last value a path takes and one above; reads hit ntar - 1 (at the histogram limits the odd last
    counter, the high half of the last 16-bit word) and, at the rows limit, ids >= 32768 in the 16-bit row fields"""
    ntar = lim if side == "inside" else lim + 1
    k, flags = kflags
    m = 0 if flags else 1
    d = dbs(k, flags, ntar, False)
    assert d.db.info.geometry == m
    for pk in loops:
        rows = name != "rows" or ntar <= LIM_ROWS
        if name == "pair_duo_hist":
            hist = ntar <= LIM_PAIR_HIST
        elif name == "general_minloc_hist":
            hist = ntar <= LIM_GEN_ML_HIST
        elif name == "general_refplace_hist":
            hist = ntar <= LIM_GEN_REF_HIST
        else:
            hist = False   # 16384 and more targets: above every histogram limit
        nks = NKS[pk] if m else NKS["ref"]
        exp, eg = check_host_batch(d, nks, 3000, {(int(rows), int(hist), m, 30, pk)})
        assert (exp == ntar - 1).sum() > 0 and eg[ntar - 1] > 0
        if name == "rows":
            assert eg[32768:].sum() > 300 and (exp >= 32768).sum() > 300


# ------------------------------------------------------------------ 3. the 16-bit histogram counters at the span cap
KID_TAPER, WPB = 6, 8


def span_cap(num_cu):
    """kid_launch_classify: a workgroup must stay below 65536 reads per launch.  The grid is 16 workgroups per CU; the
    first half of them take KID_TAPER units of reads per wave, the second half one, so the first ones get
    2 T / (T + 1) times the average share; the host caps a launch at grid * per_wg reads."""
    grid = num_cu * 16
    per_wg = (65535 - 2 * WPB - 64 * WPB) * (KID_TAPER + 1) // (2 * KID_TAPER)   # 37920
    return grid, grid * per_wg


def worst_workgroup(n, grid, pk):
    """reads of a workgroup of the first half (kid_classify_kernel: switch_block, the duo and general shares)"""
    half = grid // 2
    units = WPB * (KID_TAPER * half + (grid - half))
    unit = -(-n // units)
    if pk == 1:
        unit = (unit + 1) & ~1   # the pair loop takes an even number per unit
    return WPB * KID_TAPER * unit


@pytest.mark.parametrize("pk,read_len", [(1, 30), (2, 158), (0, 286)], ids=["pair", "duo", "general"])
def test_histogram_counters_at_the_span_cap(dbs, pk, read_len):
    """One device batch of `cap` reads puts ~65 000 reads into each of the first workgroups, within 450 of the 16-bit
    counter limit; cap + 1 and 1.5 cap take two launches.  All reads one template: (a) a miss, counted in the low half of
    hist[0] (a carry would land in target 1); (b) a read classified to the odd ntar - 1, the high half of the last word.
    The hit log overflows on the way: the seen bits of the later hits are set with atomics."""
    import torch
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    grid, cap = span_cap(num_cu)
    worst = worst_workgroup(cap, grid, pk)
    assert 65000 < worst < 65536, worst
    assert worst_workgroup(cap + cap // 2, grid, pk) >= 65536    # one launch of 1.5 cap would overflow
    n_max = cap + cap // 2
    need = n_max * (read_len + 4) + (4 << 30)
    if torch.cuda.mem_get_info()[0] < need:
        pytest.skip("needs %.0f GiB of free device memory" % (need / 2 ** 30))
    d = dbs(*shape_of(1, 1, 1, 30))
    ntar = d.ntar
    assert ntar % 2 == 0                                          # ntar - 1 is odd: the high half of its word
    acgt = np.frombuffer(b"ACGT", np.uint8)
    rng = np.random.default_rng(read_len)
    p = (read_len - 30) // 2
    templates = []
    for src in [None] + list(range(500, 600)):   # a miss; then a DB k-mer of target ntar - 1 in random bases
        t = rng.choice(acgt, read_len)
        if src is not None:
            t[p:p + 30] = d.genomes[0][src:src + 30]
        os_ = ob.OracleSample(d.odb)
        f = int(os_.classify(t, np.array([0, read_len], np.uint64))[0])
        if src is None or f == ntar - 1:
            eg, eu = os_.counts()
            templates.append((t, f, eu, os_.stats()))
        if len(templates) == 2:
            break
    assert templates[0][1] == 0 and templates[0][3]["hits"] == 0
    assert len(templates) == 2 and templates[1][1] == ntar - 1 and templates[1][3]["hits"] >= 1
    buf = torch.empty(n_max * read_len + 64, dtype=torch.uint8, device="cuda")
    out = torch.empty(n_max, dtype=torch.int32, device="cuda")
    s = d.db.sample()
    for t, f, eu, est in templates:
        buf[:n_max * read_len].view(n_max, read_len).copy_(torch.from_numpy(t).cuda().expand(n_max, read_len))
        for n in (cap, cap + 1, n_max):
            s.reset()
            out.fill_(-1)
            s.classify_fixed_device(buf.data_ptr(), read_len, n, d_out=out.data_ptr())
            torch.cuda.synchronize()
            assert s.kernel_variants() == {(1, 1, 1, 30, pk)}
            assert bool((out[:n] == f).all()), "n=%d: %d reads not classified to %d" % (n, int((out[:n] != f).sum()), f)
            g, u = s.end()
            assert g[f] == n and g.sum() == n, "n=%d: gcount[%d] = %d, total %d" % (n, f, g[f], g.sum())
            if f == 0:
                assert g[1] == 0
            assert np.array_equal(u, eu)
            st = s.stats()
            assert st["reads"] == n and st["lookups"] == n * est["lookups"] and st["hits"] == n * est["hits"], st
    s.close()
    del buf, out
    torch.cuda.empty_cache()
