"""The second pass of the call kernels' unit loop.  A wave takes 64 consecutive units and strides on by gridDim.x * 256; the
launches cap the grid at num_cu * 8 workgroups, so the loop runs a second time only for more than
bound = num_cu * 8 * 256 units (524 288 on 256 compute units) -- more than any other test hands these kernels.

The five CSR kernels (kid_support_kernel, kid_fragment_kernel, kid_vote_kernel, kid_fragment_vote_kernel, kid_loci_kernel)
get bound + 65 units through their *_from_hits_device forms: a block of the rows8 reads of tests/hit_list_cases.py with
m in {0, 1, 2, L - 1, L, L + 1, 65} hits, tiled up to the bound (about 13 hits a read: under 100 MB of hits for reads, twice
that for fragments), and behind it a tail of 65 units with every edge of the work split, W + 1 and 5000 hits among them, so
that the list append happens in the second pass.  The one call's records are the bytes of the same list given in three
calls of fewer than bound units each (offsets left absolute); the first block and the tail equal the models' records, which
never see more than those; every tile's records are the first block's; the guard records behind the outputs stay untouched.
The two segment kernels get three long records whose segments at seg_len:seg_step = 64:1 exceed the bound, and a short
dense one behind them: the records equal those of one call per record, the last record's equal the model's."""
import functools

import numpy as np
import pytest

import hit_list_cases as hc
import read_loci_cases as lc
import read_loci_model as lm
import read_support_cases as sc
from helpers import DeviceCsr, concat_reads
from kmer_id_amd import FRAGMENT_DTYPE, FRAGMENT_VOTE_DTYPE, LOCUS_DTYPE, SEGMENT_DTYPE, SEGMENT_VOTE_DTYPE, VOTE_DTYPE, KmerDB, _lib
from kmer_id_amd.api import SUPPORT_DTYPE
from read_calls import same_records
from read_fragment_votes_model import FragmentVoteModel
from read_hits_model import Hits
from read_segment_votes_model import SegmentVoteModel
from read_segments_model import SegmentModel

pytestmark = pytest.mark.gpu

FAMILIES = {"support": (SUPPORT_DTYPE, 1), "fragments": (FRAGMENT_DTYPE, 2), "votes": (VOTE_DTYPE, 1),
            "fragment_votes": (FRAGMENT_VOTE_DTYPE, 2), "loci": (LOCUS_DTYPE, 1)}  # the record, reads per unit
RULES = [(0, 0), (2, 25)]
BLOCK_M = [0, 1, 2, hc.LANE_HITS - 1, hc.LANE_HITS, hc.LANE_HITS + 1, 65]
TAIL_UNITS = 65
DIAG_BIN = 7
SEG = (64, 1)


@functools.lru_cache(maxsize=None)
def bound():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256


def take(hits, reads):
    """-> Hits of the given reads of `hits`, in that order"""
    reads = np.asarray(reads, np.int64)
    ms = (hits.offsets[reads + 1] - hits.offsets[reads]).astype(np.int64)
    off = np.zeros(reads.size + 1, np.uint64)
    off[1:] = np.cumsum(ms)
    idx = np.repeat(hits.offsets[reads].astype(np.int64) - off[:-1].astype(np.int64), ms) + np.arange(int(off[-1]))
    return Hits(off, hits.n_kmers[reads], hits.pos[idx], hits.target[idx], hits.entry[idx])


def joined(parts):
    ends = np.cumsum([0] + [int(p.offsets[-1]) for p in parts])
    off = np.concatenate([parts[0].offsets[:1]] + [p.offsets[1:] + np.uint64(e) for p, e in zip(parts, ends)])
    return Hits(off, *(np.concatenate([getattr(p, f) for p in parts]) for f in ("n_kmers", "pos", "target", "entry")))


@functools.lru_cache(maxsize=None)
def big_list(unit):
    """-> (Hits of (bound + 65) * unit reads, the block, the tail, reads in the tiled part)"""
    c = hc.case("rows8")
    ms = np.diff(c.hits.offsets.astype(np.int64))
    block = take(c.hits, np.flatnonzero(np.isin(ms, BLOCK_M)))
    tail = take(c.hits, np.arange(TAIL_UNITS * unit))
    nb, n_tiled = block.offsets.size - 1, bound() * unit
    assert nb % 2 == 0 and set(BLOCK_M) == set(np.diff(block.offsets.astype(np.int64)).tolist())
    assert {hc.WAVE_HITS + 1, 5000} <= set(np.diff(tail.offsets.astype(np.int64)).tolist())
    tiles = take(block, np.arange(n_tiled) % nb)
    return joined([tiles, tail]), block, tail, n_tiled


def for_loci(hits):
    """the list with entries the site table of read_loci_cases has"""
    return Hits(hits.offsets, hits.n_kmers, hits.pos, hits.target, hits.entry % np.uint32(lc.N_ENTRIES))


@pytest.fixture(scope="module")
def tree_db():
    c = hc.case("rows8")
    d = KmerDB(c.models.keys, c.models.targets, c.parent, k=hc.K, log2_slots=10)
    yield d
    d.close()


@pytest.fixture(scope="module")
def loci_db():
    c = lc.case()
    d = KmerDB(c.keys, c.targets, np.ones(8, np.int32), k=lc.K, log2_slots=15)
    d.set_sites(c.org, c.pos)
    yield d
    d.close()


def model_of(family, hits):
    """-> rule -> the models' records of the list"""
    c = hc.case("rows8")
    if family == "loci":
        return lambda rule: lm.batch(hits, lc.case().org, lc.case().pos, DIAG_BIN)
    if family == "fragment_votes":
        return lambda rule: FragmentVoteModel(c.models.vm).batch_anc(hits, rule)
    return getattr(hc.Expected(c.models, hits), family)


def call(db, family, d, d_out, rule, first, n):
    """the device-form call over the reads [first, first + n): offsets stay absolute"""
    dtype, unit = FAMILIES[family]
    args = (d.d_ho.value + 8 * first, d.d_hits.value, d.d_nk.value + 4 * first, n, d_out.value + dtype.itemsize * (first // unit))
    if family == "loci":
        db.loci_from_hits_device(*args, diag_bin=DIAG_BIN)
    else:
        getattr(db, family + "_from_hits_device")(*args, min_hits=rule[0], min_permille=rule[1])


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_more_units_than_one_pass_of_the_grid_takes(tree_db, loci_db, family):
    dtype, unit = FAMILIES[family]
    hits, block, tail, n_tiled = big_list(unit)
    db = tree_db
    if family == "loci":
        hits, block, tail, db = for_loci(hits), for_loci(block), for_loci(tail), loci_db
    n_units, nb = bound() + TAIL_UNITS, (block.offsets.size - 1) // unit
    assert hits.offsets.size - 1 == n_units * unit and n_units > bound()
    cuts = [0, n_units // 3, 2 * (n_units // 3), n_units]
    assert max(b - a for a, b in zip(cuts[:-1], cuts[1:])) < bound()
    exp_block, exp_tail = model_of(family, block), model_of(family, tail)
    with DeviceCsr(hits.offsets, hc.raw_hits(hits), hits.n_kmers) as d:
        for rule in RULES[:1] if family == "loci" else RULES:
            d_one, d_parts = d.out(n_units, dtype), d.out(n_units, dtype)
            call(db, family, d, d_one, rule, 0, n_units * unit)
            for a, b in zip(cuts[:-1], cuts[1:]):
                call(db, family, d, d_parts, rule, a * unit, (b - a) * unit)
            _lib.check(d.lib.kid_dev_sync(0))
            one, parts = d.records(d_one, n_units, dtype), d.records(d_parts, n_units, dtype)
            what = "%s, rule %s" % (family, rule)
            assert one.tobytes() == parts.tobytes(), what
            same_records(one[:nb], exp_block(rule), dtype, what + ", first block")
            same_records(one[n_tiled // unit:], exp_tail(rule), dtype, what + ", tail")
            whole = (n_tiled // unit) // nb * nb
            assert one[:whole].tobytes() == np.tile(one[:nb], whole // nb).tobytes(), what + ", tiles"


@pytest.mark.parametrize("family", ["segments", "segment_votes"])
def test_more_segments_than_one_pass_of_the_grid_takes(tree_db, family):
    c, rng = hc.case("rows8"), np.random.default_rng(23)
    dtype, model = (SEGMENT_DTYPE, SegmentModel) if family == "segments" else (SEGMENT_VOTE_DTYPE, SegmentVoteModel)
    length = bound() // 3 + 5200
    dense = sc.implanted(rng, [sc.cases.key_seq(c.models.keys[j], hc.K) for j in rng.integers(0, c.models.keys.size, 40)], gap=1)
    seqs = [rng.choice(sc.ACGT, length).tobytes() for _ in range(3)] + [dense]
    read = getattr(tree_db, "read_" + family)
    for rule in RULES:
        kw = dict(seg_len=SEG[0], seg_step=SEG[1], min_hits=rule[0], min_permille=rule[1])
        bases, off = concat_reads(seqs)
        one = read(bases, off, **kw)
        n_seg = np.diff(one.offsets.astype(np.int64))
        assert int(n_seg.sum()) > bound() and int(n_seg[:3].max()) < bound() and int(one.offsets[3]) > bound() and n_seg[3] > 0
        alone = [read(*concat_reads([s]), **kw) for s in seqs]
        assert one.records.dtype == dtype and one.records.tobytes() == b"".join(a.records.tobytes() for a in alone), (family, rule)
        exp = model(c.models.sm, *concat_reads([dense])).direct(SEG[0], SEG[1], rule)
        assert int(exp[1]["n_hits"].max()) >= 2
        same_records(one.records[int(one.offsets[3]):], exp[1], dtype, "%s, rule %s, last record" % (family, rule))
