"""kid_db_read_fragment_loci and kid_db_read_fragment_loci_fastq against the model (tests/read_fragment_loci_model.py over
HitModel) on the genome world of tests/read_loci_cases.py: a few hundred fragments cut from the two genomes with a known
genome, orientation and insert -- lo, hi and orient are held against the implant itself, not only against the model --,
fragments with a mate absent, too short or from the other genome; the table kinds and a split into three calls; both mask
options on the FASTQ form; and every error status of the family in its documented order, a replica without sites included."""
import functools

import numpy as np
import pytest

import read_fragment_loci_model as fm
import read_loci_cases as lc
from base_quality_cases import mask_block
from helpers import concat_reads, fastq_block
from kmer_id_amd import FRAGMENT_LOCUS_DTYPE, KID_DB_OPT_LOW_COMPLEXITY, KID_DB_OPT_MIN_BASE_QUALITY
from low_complexity_model import mask_block as lowc_mask_block
from read_calls import KINDS, revcomp, same_records, status
from read_fragments_model import interleave
from read_hits_model import trim_ranges

pytestmark = pytest.mark.gpu

KID_ERR_ARG, KID_ERR_STATE = -1, -10
K = lc.K
N_FRAGMENTS = 300
RULES = [(1, 1000), (7, 400), (1, 0)]


@functools.lru_cache(maxsize=None)
def fragments(every):
    """-> the world, [(kind, mate 1, mate 2, what)]: `proper` is (genome, a, insert, o, len_1, len_2) -- the fragment covers
    [a, a + insert) of the genome; with o = 0 mate 1 is its first len_1 bases and mate 2 the reverse complement of its last
    len_2, with o = 1 the mates are exchanged"""
    w = lc.world(every)
    rng = np.random.default_rng([every, 77])
    out = []
    for i in range(N_FRAGMENTS):
        g, insert = int(rng.integers(0, 2)), int(rng.integers(60, 1300))
        a = int(rng.integers(0, lc.GENOME_LEN - insert))
        la, lb = (min(insert, int(rng.integers(40, 160))) for _ in range(2))
        head, tail = w.genomes[g][a:a + la], revcomp(w.genomes[g][a + insert - lb:a + insert])
        o = int(rng.integers(0, 2))
        kind = ("proper", "absent", "short", "other_genome")[0 if i % 5 else 1 + (i // 5) % 3]
        if kind == "absent":
            tail = b""
        elif kind == "short":
            tail = tail[:K - 1]
        elif kind == "other_genome":
            tail = revcomp(w.genomes[1 - g][a + insert - lb:a + insert])
        out.append((kind, head, tail, (g, a, insert, o, la, lb)) if o == 0 else (kind, tail, head, (g, a, insert, o, la, lb)))
    return w, out


@pytest.fixture(scope="module", params=[1, 7])
def world(request):
    w, frags = fragments(request.param)
    w.frags = frags
    w.fbases, w.foff = concat_reads(interleave([f[1] for f in frags], [f[2] for f in frags]))
    w.fhits = w.hm.batch(w.fbases, w.foff)
    return w


@pytest.fixture(scope="module")
def db(world):
    d = world.db()
    d.set_sites(world.org, world.pos)
    yield d
    d.close()


@pytest.mark.parametrize("rule", RULES, ids=lambda r: "W%d_S%d" % r)
def test_host_form_equals_the_model_and_the_implant(world, db, rule):
    got = db.read_fragment_loci(world.fbases, world.foff, diag_bin=rule[0], max_span=rule[1])
    same_records(got, fm.batch(world.fhits, world.org, world.pos, K, *rule), FRAGMENT_LOCUS_DTYPE, "every %d, %s" % (world.every, rule))
    if rule != (1, 1000):
        return
    seen = {"paired": 0, "solo": 0, "refused": 0}
    for r, (kind, m1, m2, (g, a, insert, o, la, lb)) in zip(got, world.frags):
        first, last = world.own_windows(g, a, la), world.own_windows(g, a + insert - lb, lb)  # the database windows of head and tail
        if kind != "proper" or first.size == 0 or last.size == 0 or first.size + last.size < 5:  # (fewer: a chance pair of two may tie)
            if kind in ("absent", "short") and first.size:  # the head alone: mate 1 + o, forward
                assert (int(r["mates"]), int(r["org"]), int(r["orient"])) == (1 + o, g, o)
                assert (int(r["lo"]), int(r["hi"])) == (int(first[0]), int(first[-1]) + K - 1) and int(r["n_chain"]) == first.size
                seen["solo"] += 1
            continue
        if insert - K > rule[1]:  # the two ends are further apart than max_span: no pair
            assert int(r["n_chain"]) < first.size + last.size
            seen["refused"] += 1
            continue
        assert (int(r["mates"]), int(r["org"]), int(r["orient"])) == (3, g, o)
        assert int(r["n_chain"]) == first.size + last.size == int(r["n_hits"]) and int(r["n_other"]) == 0
        assert (int(r["lo"]), int(r["hi"])) == (int(first[0]), int(last[-1]) + K - 1)
        assert int(r["n_chain_%d" % (1 + o)]) == first.size and int(r["n_chain_%d" % (2 - o)]) == last.size
        seen["paired"] += 1
    assert seen["paired"] >= 100 and seen["solo"] >= 20 and seen["refused"] >= 1, seen


def test_the_table_kinds_and_a_split_into_three_calls_give_the_same_bytes(world, db):
    whole = db.read_fragment_loci(world.fbases, world.foff, diag_bin=7, max_span=400)
    n = world.foff.size - 1
    for name, flags in KINDS.items():
        if flags == 0:
            continue
        other = world.db(flags)
        try:
            other.set_sites(world.org, world.pos)
            assert other.read_fragment_loci(world.fbases, world.foff, diag_bin=7, max_span=400).tobytes() == whole.tobytes(), name
        finally:
            other.close()
    cuts = [0, 2 * (n // 6), 2 * (n // 6) + 2, n]
    parts = [db.read_fragment_loci(world.fbases, world.foff[a:b + 1], diag_bin=7, max_span=400) for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.concatenate(parts).tobytes() == whole.tobytes()
    assert db.read_fragment_loci(world.fbases, world.foff[:1]).size == 0
    ms, calls, n_fragments = db.read_fragment_loci_time()
    assert ms > 0 and calls >= 4 and n_fragments >= n  # (the call without a read launched nothing)


def test_fastq_form_and_both_mask_options(world, db):
    mates = []
    for which in (1, 2):
        seqs = [f[which] for f in world.frags]
        quals = [b"I" * len(s) for s in seqs]
        for i in range(which, len(seqs), 4):  # low-quality bases inside reads that are kept
            if len(seqs[i]) > 100:
                row = bytearray(quals[i])
                row[40:44] = b"++++"
                row[90] = ord("2")
                quals[i] = bytes(row)
        for i in range(3 * which, len(seqs), 9):  # dropped by quality
            quals[i] = b"!" * len(seqs[i])
        for j in range(6):  # a stretch of a genome beside a homopolymer run
            s = world.genomes[j % 2][100 * j + which:100 * j + which + 60] + b"A" * 70
            seqs.append(s)
            quals.append(b"I" * len(s))
        start, stop, keep = trim_ranges(quals, [len(s) for s in seqs], K)
        assert 0 < int((~keep).sum()) and int(keep.sum()) > 80
        start[~keep], stop[~keep] = 0, -1  # a dropped record has no window and no hit
        text, recs = fastq_block(seqs, quals, eol=b"\r\n" if which == 1 else b"\n", blank_every=5 if which == 1 else 0)
        mates.append((seqs, start, stop, text, recs))
    n = len(mates[0][0])
    start, stop = np.zeros(2 * n, np.int32), np.zeros(2 * n, np.int32)
    start[0::2], start[1::2], stop[0::2], stop[1::2] = mates[0][1], mates[1][1], mates[0][2], mates[1][2]
    (t1, r1), (t2, r2) = mates[0][3:], mates[1][3:]

    def expect(seqs1, seqs2, rule):
        b, o = concat_reads(interleave(seqs1, seqs2))
        return fm.batch(world.hm.batch(b, o, start, stop), world.org, world.pos, K, *rule)

    for rule in ((1, 1000), (7, 400)):
        got = db.read_fragment_loci_fastq(t1, r1, t2, r2, diag_bin=rule[0], max_span=rule[1])
        same_records(got, expect(mates[0][0], mates[1][0], rule), FRAGMENT_LOCUS_DTYPE, "fastq, %s" % (rule,))
    plain = db.read_fragment_loci_fastq(t1, r1, t2, r2)
    assert int((plain["mates"] == 3).sum()) > 50
    # an absent mate is a record of two empty lines; the second half of a block is a block too
    absent = np.zeros_like(r2)
    half = db.read_fragment_loci_fastq(t1, r1[n // 2:], t2, absent[n // 2:])
    b, o = concat_reads(interleave(mates[0][0][n // 2:], [b""] * (n - n // 2)))
    st, sp = np.zeros(2 * (n - n // 2), np.int32), np.full(2 * (n - n // 2), -1, np.int32)
    st[0::2], sp[0::2] = mates[0][1][n // 2:], mates[0][2][n // 2:]
    same_records(half, fm.batch(world.hm.batch(b, o, st, sp), world.org, world.pos, K, 1, 1000), FRAGMENT_LOCUS_DTYPE, "absent mates")
    assert not (half["mates"] >= 2).any()
    for option, level, mask in [(KID_DB_OPT_MIN_BASE_QUALITY, 20, mask_block), (KID_DB_OPT_LOW_COMPLEXITY, 20, lowc_mask_block)]:
        (m1, n1), (m2, n2) = mask(t1, r1, level), mask(t2, r2, level)
        assert n1 > 0 and n2 > 0
        db.set_option(option, level)
        try:
            on = db.read_fragment_loci_fastq(t1, r1, t2, r2)
        finally:
            db.set_option(option, 0)
        ms1 = [m1[int(r[0]):int(r[0] + r[1])].tobytes() for r in r1]
        ms2 = [m2[int(r[0]):int(r[0] + r[1])].tobytes() for r in r2]
        same_records(on, expect(ms1, ms2, (1, 1000)), FRAGMENT_LOCUS_DTYPE, "masked %d" % option)
        assert on.tobytes() == db.read_fragment_loci_fastq(m1, r1, m2, r2).tobytes() and on.tobytes() != plain.tobytes(), option
    assert db.read_fragment_loci_fastq(t1, r1, t2, r2).tobytes() == plain.tobytes()


def test_errors_in_their_order(world):
    db = world.db()
    try:
        bases, off = world.fbases, world.foff[:9]  # eight reads
        text, recs = fastq_block([b"ACGT" * 10], [b"I" * 40])
        lib, h = db._lib, db._h
        out = np.zeros(4, FRAGMENT_LOCUS_DTYPE)
        p = lambda a: a.ctypes.data  # noqa: E731
        raw = lambda n, w, o: lib.kid_db_read_fragment_loci(h, p(bases), p(off), None, None, n, w, 1000, o)  # noqa: E731
        # without sites: what the fragments family refuses comes first, then diag_bin = 0, then the missing sites
        assert raw(7, 0, None) == KID_ERR_ARG and raw(7, 1, p(out)) == KID_ERR_ARG  # odd
        assert raw(8, 0, None) == KID_ERR_ARG and raw(8, 1, None) == KID_ERR_ARG  # out = NULL with reads
        assert raw(8, 0, p(out)) == KID_ERR_ARG  # diag_bin = 0
        assert raw(8, 1, p(out)) == KID_ERR_STATE and not out.view(np.uint32).any()
        assert status(lambda: db.read_fragment_loci(bases, world.foff[:8])) == KID_ERR_ARG
        assert status(lambda: db.read_fragment_loci(bases, off, diag_bin=0)) == KID_ERR_ARG
        assert status(lambda: db.read_fragment_loci(bases, off)) == KID_ERR_STATE
        assert status(lambda: db.read_fragment_loci_fastq(text, recs, text, recs, diag_bin=0)) == KID_ERR_ARG
        assert status(lambda: db.read_fragment_loci_fastq(text, recs, text, recs)) == KID_ERR_STATE
        assert status(lambda: db.fragment_loci_from_hits_device(0, 0, 0, 3, 0)) == KID_ERR_ARG
        assert status(lambda: db.fragment_loci_from_hits_device(0, 0, 0, 0, 0, diag_bin=0)) == KID_ERR_ARG
        assert status(lambda: db.fragment_loci_from_hits_device(0, 0, 0, 0, 0)) == KID_ERR_STATE
        assert db.read_fragment_loci_time()[1:] == (0, 0)  # nothing was launched
        # with sites
        db.set_sites(world.org, world.pos)
        good = db.read_fragment_loci(bases, off)
        assert good.size == 4 and db.read_fragment_loci(bases, off[:1]).size == 0
        db.fragment_loci_from_hits_device(0, 0, 0, 0, 0)  # no read: KID_OK, nothing launched
        assert status(lambda: db.read_fragment_loci(bases, off, diag_bin=0)) == KID_ERR_ARG
        assert status(lambda: db.fragment_loci_from_hits_device(0, 0, 0, 2, 0)) == KID_ERR_ARG  # null pointers with reads
        assert raw(8, 1, None) == KID_ERR_ARG
        assert lib.kid_db_read_fragment_loci(h, None, p(off), None, None, 8, 1, 1000, p(out)) == KID_ERR_ARG
        assert lib.kid_db_read_fragment_loci_fastq(h, p(text), text.size, None, p(text), text.size, p(recs), 1, 1, 1000, p(out)) == KID_ERR_ARG
        # a replica starts without sites
        rep = db.replicate(0)
        try:
            assert status(lambda: rep.read_fragment_loci(bases, off)) == KID_ERR_STATE
            rep.set_sites(world.org, world.pos)
            assert rep.read_fragment_loci(bases, off).tobytes() == good.tobytes()
        finally:
            rep.close()
        db.clear_sites()
        assert status(lambda: db.read_fragment_loci(bases, off)) == KID_ERR_STATE
        db.set_sites(world.org, world.pos)
        assert db.read_fragment_loci(bases, off).tobytes() == good.tobytes()
    finally:
        db.close()
