"""read_loci -> Pileup.add end to end on the genome world of tests/read_loci_cases.py: the pileup of the kernels' own records
equals the model's on the same records; the depth of forward and reverse reads is what the rule claims it means -- the
number of reads that cover a base; and the statuses of the family in their order, a stale pileup after set_sites and
clear_sites, the orders of closing, a replica without sites."""
import numpy as np
import pytest

import read_loci_cases as lc
import read_pileup_model as pm
from helpers import concat_reads
from kmer_id_amd import PILEUP_DTYPE, Pileup
from read_calls import status

pytestmark = pytest.mark.gpu

KID_ERR_ARG, KID_ERR_STATE = -1, -10


@pytest.fixture(scope="module", params=[1, 7])
def world(request):
    return lc.world(request.param)


@pytest.fixture(scope="module")
def db(world):
    d = world.db()
    d.set_sites(world.org, world.pos)
    yield d
    d.close()


def same(p, exp, what):
    bin_base, starts, depth, records, n_placed = exp
    got = p.bins()
    assert np.array_equal(got[0], bin_base) and np.array_equal(got[1], starts) and np.array_equal(got[2], depth), what
    recs = p.summary()
    assert recs.dtype == PILEUP_DTYPE
    for f in PILEUP_DTYPE.names:
        assert np.array_equal(recs[f], records[f]), "%s: %s: got %s, the model %s" % (what, f, recs[f], records[f])
    assert recs.tobytes() == records.tobytes(), what
    return recs


@pytest.mark.parametrize("w, diag_bin, rule", [(1, 1, (2, 1)), (100, 1, (2, 1)), (1000, 7, (1, 0)), (2 ** 31 - 1, 1, (3, 5))])
def test_the_kernels_records_piled_up_equal_the_model(world, db, w, diag_bin, rule):
    loci = db.read_loci(world.bases, world.off, diag_bin=diag_bin)
    exp = pm.batch(loci, world.org, world.pos, lc.K, w, *rule)
    with db.pileup(w) as p:
        assert (p.n_orgs, p.bin_width) == (2, w)
        p.add(loci, *rule)
        recs = same(p, exp, "W = %d" % w)
        assert p.counts() == (loci.size, exp[4]) and int(recs["n_placed"].sum()) == exp[4] and 30 < exp[4] <= loci.size
        n = loci.size
        p.reset()
        for a, b in ((0, n // 3), (n // 3, n // 3 + 1), (n // 3 + 1, n)):
            p.add(loci[a:b], *rule)
        same(p, exp, "three calls")


@pytest.fixture(scope="module")
def every_window():
    world = lc.world(1)
    d = world.db()
    d.set_sites(world.org, world.pos)
    yield world, d
    d.close()


def test_depth_is_the_number_of_reads_that_cover_a_base(every_window):
    """every = 1, W = 1, min_chain = 2: depth[g][x] = #{forward and reverse reads (g, a, n) : a <= x < a + n}, clamped into
    the last bin (the last window starts at GENOME_LEN - K)"""
    world, db = every_window
    keep = [i for i, r in enumerate(world.reads) if r[0] in ("forward", "reverse")]
    bases, off = concat_reads([world.reads[i][1] for i in keep])
    loci = db.read_loci(bases, off, diag_bin=1)
    span = lc.GENOME_LEN - lc.K + 1
    want = np.zeros((2, span), np.int64)
    for i in keep:
        g, a, n = world.reads[i][2]
        lo, hi = min(a, span - 1), min(a + n - 1, span - 1)
        want[g, lo:hi + 1] += 1
    with db.pileup(1) as p:
        p.add(loci, min_chain=2, min_margin=1)
        base, starts, depth = p.bins()
        assert base.tolist() == [0, span, 2 * span] and p.counts() == (len(keep), len(keep))
        assert np.array_equal(depth.reshape(2, span), want)
        assert int(starts.sum()) == len(keep) and int(p.summary()["depth_sum"].sum()) == int(want.sum())


def test_statuses_in_their_order_and_a_stale_pileup(world):
    db = world.db()
    try:
        loci = np.zeros(3, lc.lm.LOCUS_DTYPE)
        assert status(lambda: db.pileup(0)) == KID_ERR_ARG       # bin_width = 0 comes before the missing sites
        assert status(lambda: db.pileup(100)) == KID_ERR_STATE   # no sites
        db.set_sites(world.org, world.pos)
        good = db.read_loci(world.bases, world.off)
        exp = pm.batch(good, world.org, world.pos, lc.K, 100, 2, 1)
        p = db.pileup(100)
        assert status(lambda: p.add(loci, min_chain=0)) == KID_ERR_ARG
        p.add(good)
        same(p, exp, "fresh")
        # a replica starts without sites
        rep = db.replicate(0)
        try:
            assert status(lambda: rep.pileup(100)) == KID_ERR_STATE
            rep.set_sites(world.org, world.pos)
            with rep.pileup(100) as q:
                q.add(good)
                same(q, exp, "replica")
        finally:
            rep.close()
        # the sites set again: the pileup is stale for add, and keeps answering from what it holds
        db.set_sites(world.org, (world.pos + 1).astype(np.uint32))
        assert status(lambda: p.add(good)) == KID_ERR_STATE
        assert status(lambda: p.add_device(0, 0)) == KID_ERR_STATE
        assert status(lambda: p.add(loci, min_chain=0)) == KID_ERR_ARG  # (the argument is looked at first)
        same(p, exp, "stale")
        assert p.counts() == (good.size, exp[4]) and p.export()[0].sum() == exp[4]
        p2 = db.pileup(100)
        db.clear_sites()
        assert status(lambda: p2.add(good)) == KID_ERR_STATE and status(lambda: db.pileup(100)) == KID_ERR_STATE
        assert p2.counts() == (0, 0) and not p2.bins()[2].any()
        p2.reset()
        p2.close()
        p2.close()  # (a second close does nothing)
        db.set_sites(world.org, world.pos)
        assert status(lambda: p.add(good)) == KID_ERR_STATE  # the same sites again are still another generation
        same(p, exp, "stale, the sites set a third time")
        # close orders: the pileup first, or the database first and the pileup only destroyed after it
        p.close()
        p3 = db.pileup(100)
        p3.add(good)
        assert isinstance(p3, Pileup)
    finally:
        db.close()
    p3.close()
