"""The digest plane of the minimizer-localised table and the DIGEST instantiations of the pair and duo loops
(KID_OPT_LINE_DIGEST): the plane equals its numpy model, both front halves give the oracle's answers on a table whose
lines fill up and chain, and the auto setting switches on the hit log's rate and back on a reset."""
import numpy as np
import pytest

from helpers import K
from kmer_id_amd import KID_OPT_LINE_DIGEST, KmerDB, synth
from oracle import binding as ob

pytestmark = pytest.mark.gpu

U64 = np.uint64
ACGT = np.frombuffer(b"ACGT", np.uint8)
CODE = np.zeros(256, U64)
for _j, _ch in enumerate(b"ACGT"):
    CODE[_ch] = _j
COMP = np.zeros(256, np.uint8)
for _a, _b in zip(b"ACGT", b"TGCA"):
    COMP[_a] = _b
LOG2_SLOTS = 16            # 8192 lines of 7 entries
LINE_SHIFT = 32 - (LOG2_SLOTS - 3)
W, M = 15, 16              # kid_min_window(30), kid_min_mlen(30)


# ------------------------------------------------------------------ kid_common.h in numpy
def rev2(x, bits):
    """reverse the order of the bits/2 two-bit groups of x (uint64 array)"""
    out = np.zeros_like(x)
    for j in range(bits // 2):
        out |= ((x >> U64(2 * j)) & U64(3)) << U64(bits - 2 - 2 * j)
    return out


def canonical(keyf, k=K):
    r = (~rev2(keyf, 64)) >> U64(64 - 2 * k)
    return np.minimum(keyf, r)


def key_fp(keys):
    lo, hi = keys & U64(0xFFFFFFFF), keys >> U64(32)
    rot = ((hi << U64(7)) | (hi >> U64(25))) & U64(0xFFFFFFFF)
    f = (((lo ^ rot) * U64(0x9E3779B1)) & U64(0xFFFFFFFF)) >> U64(16)
    return np.where(f == 0, U64(1), f)


def digest_fp(fp):
    return np.maximum(fp >> U64(8), U64(1))


def line_of(keys, k=K):
    """the line of a key's minimizer (kid_minimizer_of_key, kid_minloc_line)"""
    g = np.full(keys.shape, 0xFFFFFFFF, U64)
    for j in range(W):
        f = (keys >> U64(2 * (W - 1 - j))) & U64(0xFFFFFFFF)
        r = (~rev2(f, 32)) & U64(0xFFFFFFFF)
        h = (np.minimum(f, r) * U64(0x9E3779B1)) & U64(0xFFFFFFFF)
        h ^= h >> U64(15)
        g = np.minimum(g, h)
    return ((g * U64(0xC2B2AE3D)) & U64(0xFFFFFFFF)) >> U64(LINE_SHIFT)


def digest_model(table):
    """the plane from the table's headers: uint32 [lines, 2]"""
    h = table.reshape(-1, 8, 4)[:, 0, :].astype(U64)
    f = np.stack([h[:, 0] & U64(0xFFFF), h[:, 0] >> U64(16), h[:, 1] & U64(0xFFFF), h[:, 1] >> U64(16),
                  h[:, 2] & U64(0xFFFF), h[:, 2] >> U64(16), h[:, 3] & U64(0xFFFF)], axis=1)
    b = np.where(f == 0, U64(0), digest_fp(f))
    filt = h[:, 3] >> U64(20)
    nib = sum(((filt >> U64(3 * i)) & U64(7) != 0).astype(U64) << U64(i) for i in range(4))
    count = (h[:, 3] >> U64(16)) & U64(15)
    lo = b[:, 0] | (b[:, 1] << U64(8)) | (b[:, 2] << U64(16)) | (b[:, 3] << U64(24))
    hi = b[:, 4] | (b[:, 5] << U64(8)) | (b[:, 6] << U64(16)) | (count << U64(24)) | (nib << U64(28))
    return np.stack([lo, hi], axis=1).astype(np.uint32)


def windows(seq, k=K):
    """forward keys of all k-mers of an ACGT sequence (uint8 array)"""
    c = CODE[seq]
    n = seq.size - k + 1
    key = np.zeros(n, U64)
    for j in range(k):
        key = (key << U64(2)) | c[j:j + n]
    return key


# ------------------------------------------------------------------ the fixture
def genome_db(rng, n_genomes, genome_len, ntar):
    genomes, keys, targets = [], [], []
    for g in range(n_genomes):
        seq = rng.choice(ACGT, genome_len)
        key = canonical(windows(seq))
        genomes.append(seq)
        keys.append(key)
        targets.append(np.full(key.size, 2 + g % (ntar - 2), np.uint32))
    return genomes, np.concatenate(keys), np.concatenate(targets)


def make_reads(genomes, rng, n, length):
    """half cut from the genomes (every other one reverse-complemented, a substitution every ~40 bases in a quarter of
    them), half random"""
    out = []
    for i in range(n):
        if i & 1:
            out.append(rng.choice(ACGT, length))
            continue
        g = genomes[int(rng.integers(0, len(genomes)))]
        p = int(rng.integers(0, g.size - length + 1))
        s = g[p:p + length].copy()
        if i % 8 == 0:
            m = rng.random(length) < 0.025
            s[m] = rng.choice(ACGT, int(m.sum()))
        if i & 2:
            s = COMP[s[::-1]]
        out.append(s)
    return out


def pack(reads):
    data = np.concatenate(reads)
    off = np.zeros(len(reads) + 1, np.uint64)
    off[1:] = np.cumsum([r.size for r in reads])
    return data, off


class Fixture:
    def __init__(self, seed=20261):
        rng = np.random.default_rng(seed)
        parent, _ = synth.load_taxonomy("bact10")
        self.parent = parent
        self.genomes, self.keys, self.targets = genome_db(rng, 10, 3000, 40)
        self.db = KmerDB(self.keys, self.targets, parent, k=K, log2_slots=LOG2_SLOTS)
        assert self.db.info.geometry == 1
        self.odb = ob.OracleDB(parent.size, K, LOG2_SLOTS, parent=parent)
        self.odb.add(self.keys, self.targets)
        self.table, self.digest = self.db.table_and_digest()
        self.reads = {L: pack(make_reads(self.genomes, rng, 2000, L)) for L in (150, 250)}

    def close(self):
        self.db.close()
        self.odb.close()


@pytest.fixture(scope="module")
def fx():
    f = Fixture()
    yield f
    f.close()


def read_kmers(data, off):
    """canonical keys of every k-mer of every read (the reads are ACGT only), concatenated"""
    return np.concatenate([canonical(windows(data[int(off[i]):int(off[i + 1])])) for i in range(off.size - 1)])


def test_fixture_holds_every_case(fx):
    """on the CPU, from the downloaded table and the key list: the cases the two front halves must agree on are there"""
    lines = fx.table.reshape(-1, 8, 4).astype(U64)
    count = (lines[:, 0, 3] >> U64(16)) & U64(15)
    assert np.any(count == 7), "no line with 7 entries that is not chained"
    assert np.any(count == 8), "no chained line"
    ekey = lines[:, 1:, 0] | (lines[:, 1:, 1] << U64(32))            # [line, entry]
    used = lines[:, 1:, 2] != 0
    # a present key stored past its (chained) home line
    ln_of_entry = np.broadcast_to(np.arange(lines.shape[0], dtype=U64)[:, None], ekey.shape)
    live = used & (lines[:, 1:, 1] != U64(0xFFFFFFFF))
    home = line_of(ekey[live])
    away = home != ln_of_entry[live]
    assert np.any(away) and np.all(count[home[away].astype(np.int64)] == 8), "no present key stored past a chained line"
    # two entries of one line with equal digest bytes and different keys
    dbyte = np.where(used, digest_fp(key_fp(ekey)), U64(0))
    found = False
    for a in range(7):
        for b in range(a + 1, 7):
            found |= bool(np.any(used[:, a] & used[:, b] & (dbyte[:, a] == dbyte[:, b]) & (ekey[:, a] != ekey[:, b])))
    assert found, "no two entries of a line with equal digest bytes"
    # absent k-mers of the reads: one whose digest byte matches an entry of its line, one on a full line with its nibble bit set
    present = np.unique(fx.keys)
    match = nib = False
    for L, (data, off) in fx.reads.items():
        q = np.unique(read_kmers(data, off))
        q = q[~np.isin(q, present)]
        ln = line_of(q).astype(np.int64)
        fp = key_fp(q)
        match |= bool(np.any((dbyte[ln] == digest_fp(fp)[:, None]).any(axis=1)))
        hi = fx.digest[ln, 1].astype(U64)
        nib |= bool(np.any((((hi >> U64(24)) & U64(15)) == 8) & (((hi >> (U64(28) + (fp >> U64(14)))) & U64(1)) == 1)))
    assert match, "no absent k-mer whose digest byte matches a stored entry"
    assert nib, "no absent k-mer on a full line with its nibble bit set"


# ------------------------------------------------------------------ plane = model
def test_plane_equals_model_gpu_built_and_replica(fx):
    assert fx.digest is not None and fx.digest.shape == (1 << (LOG2_SLOTS - 3), 2)
    assert np.array_equal(fx.digest, digest_model(fx.table))
    rep = fx.db.replicate(0)
    t2, d2 = rep.table_and_digest()
    rep.close()
    assert np.array_equal(t2, fx.table) and np.array_equal(d2, fx.digest)


def test_plane_equals_model_with_tombstones(fx):
    """every key three times, with different targets: two of three cells become tombstones, their fingerprints stay"""
    keys = np.concatenate([fx.keys[:6000]] * 3)
    targets = np.concatenate([fx.targets[:6000], fx.targets[:6000] + 1, fx.targets[:6000] + 2]).astype(np.uint32)
    db = KmerDB(keys, targets, fx.parent, k=K, log2_slots=LOG2_SLOTS)
    table, digest = db.table_and_digest()
    db.close()
    assert int((table[:, 1] == 0xFFFFFFFF).sum()) == 12000
    assert np.array_equal(digest, digest_model(table))


def test_tables_without_a_plane(fx):
    from kmer_id_amd import KID_FLAG_HOST_BUILD, KID_FLAG_REF_GEOMETRY
    for flags in (KID_FLAG_REF_GEOMETRY, KID_FLAG_HOST_BUILD):
        db = KmerDB(fx.keys[:1000], fx.targets[:1000], fx.parent, k=K, log2_slots=LOG2_SLOTS, flags=flags)
        assert db.table_and_digest()[1] is None
        db.close()


# ------------------------------------------------------------------ both kernels, same answers
def expected_seen(fx, data, off, final):
    """the bitmap the reads set: the first-insert ordinal of every database k-mer with target > 1 in a read"""
    order = np.argsort(fx.keys, kind="stable")
    sk = fx.keys[order]
    q = np.unique(read_kmers(data, off))
    at = np.searchsorted(sk, q)
    hit = (at < sk.size) & (sk[np.minimum(at, sk.size - 1)] == q)
    first = order[at[hit]]                       # stable sort: the smallest ordinal of the key
    first = first[fx.targets[first] > 1]
    bits = np.zeros(((fx.keys.size + 127) // 128) * 16, np.uint8)
    np.bitwise_or.at(bits, first >> 3, (1 << (first & 7)).astype(np.uint8))
    return bits


@pytest.mark.parametrize("length,pairk", [(150, 1), (250, 2)])
def test_both_front_halves_equal_the_oracle(fx, length, pairk):
    data, off = fx.reads[length]
    os_ = ob.OracleSample(fx.odb)
    exp = os_.classify(data, off)
    eg, eu = os_.counts()
    est = os_.stats()
    assert (exp > 1).sum() > 500 and (exp == 0).sum() > 500
    want_bits = expected_seen(fx, data, off, exp)
    for option in (0, 1):
        s = fx.db.sample()
        s.set_option(KID_OPT_LINE_DIGEST, option)
        got = s.classify(data, off)
        assert s.kernel_variants(digest=bool(option)) == {(1, 1, 1, 30, pairk)} and not s.kernel_variants(digest=not option), option
        assert np.array_equal(got, exp), "option %d: %d reads differ from the oracle" % (option, int((got != exp).sum()))
        bits = s.seen_export(0, s.seen_bytes())
        g, u = s.end()
        assert np.array_equal(g, eg) and np.array_equal(u, eu), option
        st = s.stats()
        assert st["lookups"] == est["lookups"] and st["hits"] == est["hits"], (option, st, est)
        assert np.array_equal(bits, want_bits), option
        s.close()


def test_option_values(fx):
    from kmer_id_amd import KidError
    s = fx.db.sample()
    for bad in (-1, 3):
        with pytest.raises(KidError):
            s.set_option(KID_OPT_LINE_DIGEST, bad)
    s.close()


# ------------------------------------------------------------------ auto
def small_batches(s, os_, reads, n_batches, per):
    """n_batches host batches of `per` reads each, the oracle alongside -> all final targets equal"""
    for b in range(n_batches):
        data, off = pack(reads[(b * per) % len(reads):][:per])
        assert np.array_equal(s.classify(data, off), os_.classify(data, off))


def test_auto_switches_on_the_log_rate_and_back_on_reset():
    """A sparse database (random keys): reads of nine database k-mers each report ~9 log places per read -- above the
    threshold of 8 -- and random reads next to none.  A pass over the log comes with the 257th launch of a sample; the
    launch after it knows what the pass found."""
    rng = np.random.default_rng(77)
    parent, cnt = synth.load_taxonomy("bact10")
    cum = synth.cumulative(synth.scaled_counts(cnt, 2e-5))
    keys, targets = synth.db_keys(cum)
    db = KmerDB(keys, targets, parent, k=K, log2_slots=LOG2_SLOTS)
    odb = ob.OracleDB(parent.size, K, LOG2_SLOTS, parent=parent)
    odb.add(keys, targets)
    dense = []
    for i in range(64):
        s_ = rng.choice(ACGT, 275)
        for j, kk in enumerate(rng.choice(keys, 9)):
            s_[j * K:(j + 1) * K] = ACGT[((int(kk) >> (2 * (K - 1 - np.arange(K)))) & 3)]
        dense.append(s_)
    sparse = [rng.choice(ACGT, 275) for _ in range(64)]
    hdr, dig = {(1, 1, 1, 30, 2)}, {(1, 1, 1, 30, 2)}

    s, os_ = db.sample(), ob.OracleSample(odb)
    small_batches(s, os_, dense, 260, 16)
    assert s.log_state()["passes"] >= 1
    assert s.kernel_variants(digest=True) == dig and s.kernel_variants(digest=False) == hdr   # began on the plane, ended on the headers
    g, u = s.end()
    eg, eu = os_.counts()
    assert np.array_equal(g, eg) and np.array_equal(u, eu)
    assert s.stats()["hits"] == os_.stats()["hits"] and s.stats()["lookups"] == os_.stats()["lookups"]
    # the reset puts the digest back; a sample below the threshold stays on it through its passes
    s.reset()
    os_.reset()
    small_batches(s, os_, sparse, 260, 16)
    assert s.log_state()["passes"] >= 1
    assert s.kernel_variants(digest=True) == dig and not s.kernel_variants(digest=False)
    g, u = s.end()
    eg, eu = os_.counts()
    assert np.array_equal(g, eg) and np.array_equal(u, eu)
    s.close()
    db.close()
    odb.close()
