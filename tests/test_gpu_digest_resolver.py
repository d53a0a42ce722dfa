"""The resolver of the DIGEST pair and duo loops settles a flagged lookup from the header of its table line: a lookup
that only the digest's 8-bit fingerprints flagged costs no cell load, and the results stay those of the oracle and of the
header kernels -- on a sparse table, where false flags outnumber everything else the resolver sees, and on a loaded one
with chained lines, keys stored past their home line and tombstones."""
import numpy as np
import pytest

from helpers import K
from kmer_id_amd import KID_OPT_LINE_DIGEST, KmerDB, synth
from oracle import binding as ob
from test_gpu_line_digest import ACGT, CODE, U64, canonical, digest_fp, key_fp, rev2

pytestmark = pytest.mark.gpu

LOG2_SLOTS = 18                      # 2^18 cells, 2^15 lines of 7 entries
LINES = 1 << (LOG2_SLOTS - 3)
LINE_SHIFT = 32 - (LOG2_SLOTS - 3)
W = 15                               # kid_min_window(30)
N_READS = 3000                       # per read length
LENGTHS = {150: 1, 250: 2}           # read length -> PAIRK: the pair loop and the duo loop


def line_of(keys):
    """test_gpu_line_digest.line_of for this table's number of lines"""
    g = np.full(keys.shape, 0xFFFFFFFF, U64)
    for j in range(W):
        f = (keys >> U64(2 * (W - 1 - j))) & U64(0xFFFFFFFF)
        r = (~rev2(f, 32)) & U64(0xFFFFFFFF)
        h = (np.minimum(f, r) * U64(0x9E3779B1)) & U64(0xFFFFFFFF)
        h ^= h >> U64(15)
        g = np.minimum(g, h)
    return ((g * U64(0xC2B2AE3D)) & U64(0xFFFFFFFF)) >> U64(LINE_SHIFT)


def random_keys(rng, n):
    """n distinct canonical 30-mers"""
    keys = np.unique(canonical(rng.integers(0, 1 << 60, 2 * n, dtype=np.uint64)))
    assert keys.size >= n
    return rng.permutation(keys)[:n]


def make_reads(rng, keys, n, length):
    """n ACGT reads as uint8 [n, length]: the odd ones random, the even ones random with one to four database k-mers"""
    reads = rng.choice(ACGT, (n, length))
    shifts = (2 * (K - 1 - np.arange(K))).astype(U64)
    for i in range(0, n, 2):
        for j, kk in enumerate(rng.choice(keys, int(rng.integers(1, 5)))):
            reads[i, j * K:(j + 1) * K] = ACGT[((kk >> shifts) & U64(3)).astype(np.int64)]
    return reads


def kmers_of(reads):
    """canonical keys of every k-mer of every read, in read and window order"""
    c = CODE[reads]
    n = reads.shape[1] - K + 1
    key = np.zeros((reads.shape[0], n), U64)
    for j in range(K):
        key = (key << U64(2)) | c[:, j:j + n]
    return canonical(key.ravel())


def table_parts(table):
    """-> header fingerprints [line, 7], count [line], entry keys [line, 7], used [line, 7], tombstone [line, 7]"""
    lines = table.reshape(-1, 8, 4).astype(U64)
    h = lines[:, 0, :]
    f = np.stack([h[:, 0] & U64(0xFFFF), h[:, 0] >> U64(16), h[:, 1] & U64(0xFFFF), h[:, 1] >> U64(16),
                  h[:, 2] & U64(0xFFFF), h[:, 2] >> U64(16), h[:, 3] & U64(0xFFFF)], axis=1)
    count = (h[:, 3] >> U64(16)) & U64(15)
    ekey = lines[:, 1:, 0] | (lines[:, 1:, 1] << U64(32))
    used = lines[:, 1:, 2] != 0
    tomb = lines[:, 1:, 1] == U64(0xFFFFFFFF)
    return f, count, ekey, used, tomb


class Database:
    """a GPU-built table, its oracle, reads of both lengths with the oracle's answers (computed once, never changed)"""

    def __init__(self, rng, parent, keys, targets):
        self.keys, self.targets = keys, targets
        self.db = KmerDB(keys, targets, parent, k=K, log2_slots=LOG2_SLOTS)
        assert self.db.info.geometry == 1
        self.table, self.digest = self.db.table_and_digest()
        assert self.digest is not None and self.table.shape[0] == 1 << LOG2_SLOTS
        self.odb = ob.OracleDB(parent.size, K, LOG2_SLOTS, parent=parent)
        self.odb.add(keys, targets)
        self.reads, self.kmers, self.expect = {}, {}, {}
        for L in LENGTHS:
            r = make_reads(rng, keys, N_READS, L)
            self.reads[L] = (r.ravel(), (np.arange(N_READS + 1, dtype=np.uint64) * np.uint64(L)))
            self.kmers[L] = kmers_of(r)
            os_ = ob.OracleSample(self.odb)
            final = os_.classify(*self.reads[L])
            self.expect[L] = (final,) + tuple(os_.counts()) + (os_.stats(), self.seen_model(self.kmers[L]))
            os_.close()

    def seen_model(self, kmers):
        """the bitmap the reads set: the first-insert ordinal of every database k-mer with target > 1 in a read"""
        order = np.argsort(self.keys, kind="stable")
        sk = self.keys[order]
        q = np.unique(kmers)
        at = np.searchsorted(sk, q)
        hit = (at < sk.size) & (sk[np.minimum(at, sk.size - 1)] == q)
        first = order[at[hit]]
        first = first[self.targets[first] > 1]
        bits = np.zeros(((self.keys.size + 127) // 128) * 16, np.uint8)
        np.bitwise_or.at(bits, first >> 3, (1 << (first & 7)).astype(np.uint8))
        return bits

    def close(self):
        self.db.close()
        self.odb.close()


@pytest.fixture(scope="module")
def parent():
    return synth.load_taxonomy("bact10")[0]


@pytest.fixture(scope="module")
def sparse(parent):
    """about 0.5 random keys per line: nearly every lookup the digest flags is a false flag of an 8-bit fingerprint"""
    rng = np.random.default_rng(20265)
    keys = random_keys(rng, LINES // 2)
    d = Database(rng, parent, keys, (2 + np.arange(keys.size) % 38).astype(np.uint32))
    yield d
    d.close()


@pytest.fixture(scope="module")
def loaded(parent):
    """about 2.5 cells per line: every key three times with different targets, so two of its three cells are tombstones"""
    rng = np.random.default_rng(20266)
    once = random_keys(rng, (5 * LINES // 2) // 3)
    t = (2 + np.arange(once.size) % 36).astype(np.uint32)
    d = Database(rng, parent, np.concatenate([once] * 3), np.concatenate([t, t + 1, t + 2]).astype(np.uint32))
    yield d
    d.close()


def flag_counts(d, length):
    """-> (H, C16, D8) over all k-mer instances of the reads of that length, from the downloaded table"""
    f, count, ekey, used, _ = table_parts(d.table)
    q = d.kmers[length]
    ln = line_of(q).astype(np.int64)
    fp = key_fp(q)
    H = int(np.isin(q, d.keys).sum())
    m16 = f[ln] == fp[:, None]                                   # (fp is never 0, an unused slot always)
    same = used[ln] & (ekey[ln] == q[:, None])
    C16 = int((m16 & ~same).sum())
    dbyte = np.where(f == 0, U64(0), digest_fp(f))
    m8 = dbyte[ln] == digest_fp(fp)[:, None]
    D8 = int((m8.any(axis=1) & ~m16.any(axis=1)).sum())
    return H, C16, D8


def run(d, length, option):
    """one sample over the reads of that length -> (final, gcount, ucount, seen bitmap, stats)"""
    s = d.db.sample()
    s.set_option(KID_OPT_LINE_DIGEST, option)
    final = s.classify(*d.reads[length])
    want = {(1, 1, 1, 30, LENGTHS[length])}
    assert s.kernel_variants(digest=bool(option)) == want and not s.kernel_variants(digest=not option), (option, s.kernel_variants())
    bits = s.seen_export(0, s.seen_bytes())
    g, u = s.end()
    st = s.stats()
    s.close()
    return final, g, u, bits, st


@pytest.mark.parametrize("length", sorted(LENGTHS))
def test_a_false_flag_of_the_digest_reads_no_cell(sparse, length):
    """stats: probes - lookups = cells read beyond the first load of a lookup.  Every stored key's cell is read (H); a
    16-bit fingerprint that matches another key costs its cell and, by the zero test of kid_hdr_cand, perhaps the slot
    above it (2 C16).  The D8 lookups that only an 8-bit fingerprint flagged must cost none: a resolver that trusts the
    digest reads about H + D8 cells."""
    _, count, _, _, _ = table_parts(sparse.table)
    assert int(count.max()) < 7, "a full line: the bound below would have to count chain walks"
    H, C16, D8 = flag_counts(sparse, length)
    print("length %d: H %d, C16 %d, D8 %d" % (length, H, C16, D8))
    assert D8 >= 200 and D8 >= 20 * (2 * C16 + 1), (H, C16, D8)
    final, g, u, bits, st = run(sparse, length, 1)
    print("length %d: lookups %d, probes %d: %d cells read" % (length, st["lookups"], st["probes"], st["probes"] - st["lookups"]))
    assert st["lookups"] == sparse.kmers[length].size
    assert H <= st["probes"] - st["lookups"] <= H + 2 * C16, (st, H, C16, D8)


def check_results(d, length):
    exp, eg, eu, est, ebits = d.expect[length]
    assert (exp > 1).sum() > 200 and (exp == 0).sum() > 200
    got = {option: run(d, length, option) for option in (0, 1)}
    for option, (final, g, u, bits, st) in got.items():
        assert np.array_equal(final, exp), "option %d: %d reads differ from the oracle" % (option, int((final != exp).sum()))
        assert np.array_equal(g, eg) and np.array_equal(u, eu), option
        assert st["lookups"] == est["lookups"] and st["hits"] == est["hits"], (option, st, est)
        assert np.array_equal(bits, ebits), option
    for a, b in zip(got[0][:4], got[1][:4]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("length", sorted(LENGTHS))
def test_results_on_the_sparse_table(sparse, length):
    check_results(sparse, length)


def test_loaded_table_holds_every_case(loaded):
    """chained lines, present keys stored past their home line, two tombstones per key; and a line where the digest's
    candidates and the header's differ for a k-mer of the reads"""
    f, count, ekey, used, tomb = table_parts(loaded.table)
    assert np.any(count == 8), "no chained line"
    assert int(tomb.sum()) == 2 * (loaded.keys.size // 3)
    live = used & ~tomb
    ln_of_entry = np.broadcast_to(np.arange(LINES, dtype=U64)[:, None], ekey.shape)
    home = line_of(ekey[live])
    away = home != ln_of_entry[live]
    assert np.any(away) and np.all(count[home[away].astype(np.int64)] == 8), "no present key stored past a chained line"
    differ = chained = 0
    for L in LENGTHS:
        q = loaded.kmers[L]
        ln = line_of(q).astype(np.int64)
        fp = key_fp(q)
        m16 = f[ln] == fp[:, None]
        m8 = np.where(f[ln] == 0, U64(0), digest_fp(f[ln])) == digest_fp(fp)[:, None]
        differ += int((m8 != m16).any(axis=1).sum())
        w3 = loaded.table.reshape(-1, 8, 4)[ln, 0, 3].astype(U64)
        chained += int(((count[ln] == 8) & (((w3 >> (U64(20) + ((fp * U64(12)) >> U64(16)))) & U64(1)) == 1)).sum())
    assert differ > 0, "no k-mer for which a digest-named slot and a header-named slot differ"
    assert chained > 0, "no k-mer whose header sends the resolver along the chain"


@pytest.mark.parametrize("length", sorted(LENGTHS))
def test_results_on_the_loaded_table(loaded, length):
    check_results(loaded, length)
