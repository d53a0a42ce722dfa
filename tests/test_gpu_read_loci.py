"""kid_db_read_loci and kid_db_read_loci_fastq against the model (tests/read_loci_model.py over HitModel) on the genome
world of tests/read_loci_cases.py: forward reads, reverse complements, chimeras and reads shorter than k; the three table
kinds; a batch split into three calls; both mask options on the FASTQ form; and the errors of the family: no sites, a
replica, diag_bin = 0, sites the library refuses."""
import numpy as np
import pytest

import read_loci_cases as lc
import read_loci_model as lm
from base_quality_cases import mask_block
from helpers import concat_reads, fastq_block
from kmer_id_amd import KID_DB_OPT_LOW_COMPLEXITY, KID_DB_OPT_MIN_BASE_QUALITY, LOCUS_DTYPE
from low_complexity_model import mask_block as lowc_mask_block
from read_calls import KINDS, same_records, status
from read_hits_model import trim_ranges

pytestmark = pytest.mark.gpu

KID_ERR_ARG, KID_ERR_STATE = -1, -10


@pytest.fixture(scope="module", params=[1, 7])
def world(request):
    w = lc.world(request.param)
    w.hits = w.hm.batch(w.bases, w.off)
    return w


@pytest.fixture(scope="module")
def db(world):
    d = world.db()
    d.set_sites(world.org, world.pos)
    yield d
    d.close()


@pytest.mark.parametrize("w", lc.WIDTHS)
def test_host_form_equals_the_model(world, db, w):
    got = db.read_loci(world.bases, world.off, diag_bin=w)
    same_records(got, lm.batch(world.hits, world.org, world.pos, w), LOCUS_DTYPE, "every %d, W = %d" % (world.every, w))
    if w == 1:  # what the rule promises, on the kernels' own records
        seen = {"forward": 0, "reverse": 0, "chimera": 0, "short": 0}
        for r, (kind, seq, what) in zip(got, world.reads):
            if kind == "short":
                assert r.tobytes() == np.zeros(1, LOCUS_DTYPE).tobytes()
            elif kind == "chimera":
                if r["n_other"] == 0:
                    continue
            elif r["n_hits"] < 2:
                continue
            elif kind == "forward":
                assert (int(r["org"]), int(r["strand"]), int(r["n_chain"])) == (what[0], 0, int(r["n_hits"]))
                assert int(world.pos[r["entry_first"]]) - int(r["pos_first"]) == what[1]
            else:
                assert (int(r["org"]), int(r["strand"]), int(r["n_chain"])) == (what[0], 1, int(r["n_hits"]))
                assert int(world.pos[r["entry_first"]]) + int(r["pos_first"]) == what[1] + what[2] - lc.K
            seen[kind] += 1
        assert min(seen.values()) >= 3, seen
        if world.every == 1:
            assert int(got["n_hits"].max()) > lc.WAVE_HITS and int((got["n_hits"] <= lc.LANE_HITS).sum()) >= 3


def test_the_table_kinds_and_a_split_into_three_calls_give_the_same_bytes(world, db):
    whole = db.read_loci(world.bases, world.off, diag_bin=7)
    n = world.off.size - 1
    for name, flags in KINDS.items():
        if flags == 0:
            continue
        other = world.db(flags)
        try:
            other.set_sites(world.org, world.pos)
            assert other.read_loci(world.bases, world.off, diag_bin=7).tobytes() == whole.tobytes(), name
        finally:
            other.close()
    cuts = [0, n // 3, n // 3 + 1, n]
    parts = [db.read_loci(world.bases, world.off[a:b + 1], diag_bin=7) for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.concatenate(parts).tobytes() == whole.tobytes()
    assert db.read_loci(world.bases, world.off[:1], diag_bin=7).size == 0


def test_ranges_are_honoured(world, db):
    n = world.off.size - 1
    lens = np.diff(world.off.astype(np.int64))
    start = np.minimum(5, np.maximum(lens - 1, 0)).astype(np.int32)
    stop = np.maximum(lens - 1 - 7, start).astype(np.int32)
    stop[lens == 0] = -1
    start[lens == 0] = 0
    got = db.read_loci(world.bases, world.off, start, stop, diag_bin=1)
    same_records(got, lm.batch(world.hm.batch(world.bases, world.off, start, stop), world.org, world.pos, 1), LOCUS_DTYPE, "ranges")
    assert n == got.size


def test_fastq_form_and_both_mask_options(world, db):
    seqs = [seq for kind, seq, what in world.reads]
    quals = [b"I" * len(s) for s in seqs]
    for i in range(0, len(seqs), 4):  # low-quality bases inside reads that are kept
        if len(seqs[i]) > 100:
            row = bytearray(quals[i])
            row[40:44] = b"++++"
            row[90] = ord("2")
            quals[i] = bytes(row)
    for i in range(1, len(seqs), 9):  # dropped by quality
        quals[i] = b"!" * len(seqs[i])
    for j in range(12):  # a stretch of a genome beside a homopolymer run
        s = world.genomes[j % 2][100 * j:100 * j + 60] + b"A" * 70
        seqs.append(s)
        quals.append(b"I" * len(s))
    start, stop, keep = trim_ranges(quals, [len(s) for s in seqs], lc.K)
    assert 0 < int((~keep).sum()) and int(keep.sum()) > 80
    start[~keep], stop[~keep] = 0, -1  # a dropped record has no window and no hit
    text, recs = fastq_block(seqs, quals, eol=b"\r\n", blank_every=5)

    def expect(the_seqs, w):
        b, o = concat_reads(the_seqs)
        return lm.batch(world.hm.batch(b, o, start, stop), world.org, world.pos, w)

    for w in (1, 7):
        same_records(db.read_loci_fastq(text, recs, diag_bin=w), expect(seqs, w), LOCUS_DTYPE, "fastq, W = %d" % w)
    plain = db.read_loci_fastq(text, recs)
    assert not plain["n_kmers"][~keep].any()
    for option, level, mask in [(KID_DB_OPT_MIN_BASE_QUALITY, 20, mask_block), (KID_DB_OPT_LOW_COMPLEXITY, 20, lowc_mask_block)]:
        masked, n_masked = mask(text, recs, level)
        assert n_masked > 0
        db.set_option(option, level)
        try:
            on = db.read_loci_fastq(text, recs)
        finally:
            db.set_option(option, 0)
        mseqs = [masked[int(r[0]):int(r[0] + r[1])].tobytes() for r in recs]
        same_records(on, expect(mseqs, 1), LOCUS_DTYPE, "masked %d" % option)
        assert on.tobytes() == db.read_loci_fastq(masked, recs).tobytes() and on.tobytes() != plain.tobytes(), option
    assert db.read_loci_fastq(text, recs).tobytes() == plain.tobytes()


def test_errors(world):
    db = world.db()
    try:
        bases, off = world.bases, world.off
        n_entries = world.org.size
        assert db.info.n_entries == n_entries
        # no sites
        assert status(lambda: db.read_loci(bases, off)) == KID_ERR_STATE
        text, recs = fastq_block([b"ACGT" * 10], [b"I" * 40])
        assert status(lambda: db.read_loci_fastq(text, recs)) == KID_ERR_STATE
        assert status(lambda: db.loci_from_hits_device(0, 0, 0, 0, 0)) == KID_ERR_STATE
        # sites the library refuses leave the old ones in force
        db.set_sites(world.org, world.pos)
        good = db.read_loci(bases, off)
        bad_org, bad_pos = world.org.copy(), world.pos.copy()
        bad_org[-1], bad_pos[0] = 2 ** 24, 2 ** 31
        assert status(lambda: db.set_sites(world.org[:-1], world.pos[:-1])) == KID_ERR_ARG
        assert status(lambda: db.set_sites(np.append(world.org, 0), np.append(world.pos, 0))) == KID_ERR_ARG
        assert status(lambda: db.set_sites(bad_org, world.pos)) == KID_ERR_ARG
        assert status(lambda: db.set_sites(world.org, bad_pos)) == KID_ERR_ARG
        assert db.read_loci(bases, off).tobytes() == good.tobytes()
        # diag_bin = 0
        assert status(lambda: db.read_loci(bases, off, diag_bin=0)) == KID_ERR_ARG
        assert status(lambda: db.read_loci_fastq(text, recs, diag_bin=0)) == KID_ERR_ARG
        assert status(lambda: db.loci_from_hits_device(0, 0, 0, 0, 0, diag_bin=0)) == KID_ERR_ARG
        # a replica starts without
        rep = db.replicate(0)
        try:
            assert status(lambda: rep.read_loci(bases, off)) == KID_ERR_STATE
            rep.set_sites(world.org, world.pos)
            assert rep.read_loci(bases, off).tobytes() == good.tobytes()
        finally:
            rep.close()
        # a second call replaces them; clearing and setting again works
        db.set_sites(world.org, (world.pos + 1).astype(np.uint32))
        moved = db.read_loci(bases, off)
        hit = good["n_chain"] > 0
        assert np.array_equal(moved["entry_first"], good["entry_first"]) and hit.sum() > 50
        db.clear_sites()
        assert status(lambda: db.read_loci(bases, off)) == KID_ERR_STATE
        db.clear_sites()
        db.set_sites(world.org, world.pos)
        assert db.read_loci(bases, off).tobytes() == good.tobytes()
        assert db.read_loci_time()[1] >= 4
    finally:
        db.close()
