"""The read-hits model (tests/read_hits_model.py) against the oracle, before any GPU is involved: folding each read's
model hits left to right with the oracle's msca gives OracleSample.classify's final target, the windows add up to the
oracle's lookups and the hits to its hits.  The GPU tests then hold kid_db_read_hits* against this model."""
import numpy as np
import pytest

import read_hits_cases as cases
from helpers import ob, oracle_db
from kmer_id_amd import synth
from read_hits_model import HitModel, trim_ranges


def check_against_oracle(odb, model, bases, off, start=None, stop=None):
    hits = model.batch(bases, off, start, stop)
    smp = ob.OracleSample(odb)
    final = smp.classify(bases, off, start, stop)
    st = smp.stats()
    assert int(hits.n_kmers.sum()) == st["lookups"]
    assert int(hits.offsets[-1]) == st["hits"]
    bad = [r for r in range(off.size - 1) if model.fold(hits.of(r)[1]) != int(final[r])]
    assert not bad, "fold of the model's hits differs from process_read for reads %s" % bad[:10]
    for r in range(off.size - 1):  # position order, inside the classified range
        pos = hits.of(r)[0].astype(np.int64)
        assert np.all(np.diff(pos) > 0)
    return hits, final


def test_seeded_reads_fold_lookups_hits():
    parent, cum, keys, targets = cases.database(30, 2e-4)
    odb = oracle_db(parent, keys, targets, 20)
    bases, off = cases.synth_reads(cum, parent, 4000, 150)
    hits, final = check_against_oracle(odb, HitModel(odb, keys, targets, 30), bases, off)
    per_read = np.diff(hits.offsets.astype(np.int64))
    # the figures of this seeded set: they pin the generators the GPU tests share
    assert int(hits.n_kmers.sum()) == 482720 and int(hits.offsets[-1]) == 5100
    assert int((per_read > 0).sum()) == 1989 and int(per_read.max()) == 5
    assert np.all(keys[hits.entry] != 0) and np.array_equal(targets[hits.entry], hits.target)


@pytest.mark.parametrize("k", [15, 31])
def test_other_k(k):
    parent, cum, keys, targets = cases.database(k, 1e-4)
    odb = oracle_db(parent, keys, targets, 18, k=k)
    model = HitModel(odb, keys, targets, k)
    bases, off = cases.synth_reads(cum, parent, 600, 150, k=k)
    check_against_oracle(odb, model, bases, off)
    bases, off = cases.adversarial_reads(keys, k, seed=k)
    check_against_oracle(odb, model, bases, off)


def test_adversarial_bytes_and_duplicates_and_rolling_loop():
    parent, cum, keys, targets = cases.database(30, 1e-4, dup=True)
    odb = oracle_db(parent, keys, targets, 18)
    model = HitModel(odb, keys, targets, 30)
    bases, off = cases.adversarial_reads(keys, 30, seed=7)
    hits, final = check_against_oracle(odb, model, bases, off)
    assert int(hits.offsets[-1]) > 300
    # entry is the FIRST insert of the key
    for e, t in zip(hits.entry[:200].tolist(), hits.target[:200].tolist()):
        assert int(np.flatnonzero(keys == keys[e])[0]) == e and int(targets[e]) == t
    raw = bytes(bases)
    for r in range(0, off.size - 1, 5):  # the literal loop of the reference agrees with the vectorised windows
        seq = raw[int(off[r]):int(off[r + 1])]
        n, lst = model.read_rolling(seq, 0, len(seq) - 1)
        p, t, e = hits.of(r)
        assert n == int(hits.n_kmers[r]) and lst == list(zip(p.tolist(), t.tolist(), e.tolist()))


def test_u_is_t():
    parent, cum, keys, targets = cases.database(30, 1e-4)
    bases, off = cases.adversarial_reads(keys, 30, seed=11, u=True)
    assert b"U" in bytes(bases) and b"u" in bytes(bases)
    totals = []
    for flags in (0, ob.KO_FLAG_U_IS_T):
        odb = oracle_db(parent, keys, targets, 18, flags=flags)
        hits, _ = check_against_oracle(odb, HitModel(odb, keys, targets, 30, u_is_t=bool(flags)), bases, off)
        totals.append(int(hits.offsets[-1]))
    assert totals[1] > totals[0]  # implants written with U only count under the flag


def test_trimmed_ranges_from_process_qual():
    parent, cum, keys, targets = cases.database(30, 2e-4)
    odb = oracle_db(parent, keys, targets, 20)
    n, length = 1500, 150
    bases, off = cases.synth_reads(cum, parent, n, length)
    quals = synth.qualities(n, length)
    start, stop, keep = trim_ranges([q.tobytes() for q in quals], [length] * n, 30)
    assert 0 < int(keep.sum()) < n and int((start > 0).sum()) > 50 and int((stop < length - 1).sum()) > 50
    idx = np.flatnonzero(keep)
    b2 = bases.reshape(n, length)[idx].reshape(-1)
    o2 = synth.fixed_offsets(idx.size, length)
    hits, _ = check_against_oracle(odb, HitModel(odb, keys, targets, 30), b2, o2, start[idx], stop[idx])
    for r in range(idx.size):  # pos counts from the first byte of the read, not from start
        p = hits.of(r)[0]
        assert np.all(p >= start[idx][r]) and np.all(p + 29 <= stop[idx][r])


def test_probe_cap_of_m3():
    """a nearly full table with MAXREPROBE 16: keys that sit beyond the cap are no hits (the oracle answers 0)"""
    parent, cum, keys, targets = cases.database(30, 2e-4)
    keys, targets = keys[:15000], targets[:15000]
    capped = oracle_db(parent, keys, targets, 14, max_probes=16)
    free = oracle_db(parent, keys, targets, 14)
    bases, off = cases.adversarial_reads(keys, 30, seed=3, n=900)
    hc, _ = check_against_oracle(capped, HitModel(capped, keys, targets, 30), bases, off)
    hf, _ = check_against_oracle(free, HitModel(free, keys, targets, 30), bases, off)
    assert 0 < int(hc.offsets[-1]) < int(hf.offsets[-1])
