"""The tile edges of the kernels that cut a record into tiles of windows (kid_tile.hip.h): the long-record path at its
256-window tiles (kid_long.hip.h, reached at a small KID_OPT_LONG_RECORD_KMERS) and the read-hits path at its
64-window tiles (kid_hits.hip.h).  Records that end one window before, on and after a tile edge; database k-mers, an N
and a lower-case stretch on the windows either side of an edge.  Exact: the values are integers."""
import numpy as np
import pytest

import read_hits_cases as cases
from helpers import concat_reads, ob, oracle_db
from kmer_id_amd import KID_FLAG_REF_GEOMETRY, KmerDB, _lib
from read_hits_model import HitModel, windows
from test_gpu_read_hits import cross_check, same_hits

pytestmark = pytest.mark.gpu

KINDS = {"minloc": 0, "ref_geometry": KID_FLAG_REF_GEOMETRY}
ACGT = np.frombuffer(b"ACGT", np.uint8)


def lineage_targets(parent, odb):
    """x = the deepest node, p = its parent, y = a node whose deepest common node with x lies above p: the fold of
    [x, y, p] ends on p, the fold of [p, y, x] on x"""
    depth = np.zeros(parent.size, np.int64)
    for t in range(2, parent.size):
        d, u = 0, t
        while u != 1:
            u, d = int(parent[u]), d + 1
        depth[t] = d
    x = int(np.argmax(depth))
    p = int(parent[x])
    y = next(t for t in range(2, parent.size) if depth[odb.msca(t, x)] < depth[p])
    return x, y, p


def edge_case(k, sizes, plants, n_at, lower_at, short):
    """records of `sizes` windows with short reads in between and the last record last in the batch; the canonical
    k-mers of the windows `plants` of every record that has them go into the database under targets of one lineage and
    a foreign node in turn; the records named by n_at / lower_at get an N / a lower-case stretch there
    -> parent, keys, targets, odb, model, bases, off, the records' numbers in the batch"""
    rng = np.random.default_rng(1000 * k + sizes[0])
    parent, cum, keys0, targets0 = cases.database(k, 1e-4)
    x, y, p = lineage_targets(parent, oracle_db(parent, keys0[:1], targets0[:1], 10, k=k))
    turn = [x, y, p, y]
    sb, so = cases.synth_reads(cum, parent, 2 * len(sizes), short, k=k)
    shorts = [sb[int(so[i]):int(so[i + 1])].tobytes() for i in range(2 * len(sizes))]
    seqs, where, pkeys, ptargets = [], [], [], []
    for i, nwin in enumerate(sizes):
        rec = rng.choice(ACGT, nwin + k - 1)
        key, _ = windows(rec.tobytes(), 0, rec.size - 1, k)
        assert key.size == nwin
        for j, w in enumerate(w for w in plants if w < nwin and not (i in n_at and abs(w - n_at[i]) < k)):
            pkeys.append(key[w])
            ptargets.append(turn[j % 4])
        if i in n_at:
            rec[n_at[i]] = ord("N")  # the windows n_at - k + 1 .. n_at hold no k-mer
        if i in lower_at:
            rec[lower_at[i] - 10:lower_at[i] + k + 10] |= 0x20
        seqs += shorts[2 * i:2 * i + 2]
        where.append(len(seqs))
        seqs.append(rec.tobytes())
    keys = np.concatenate([keys0, np.array(pkeys, np.uint64)])
    targets = np.concatenate([targets0, np.array(ptargets, np.uint32)])
    odb = oracle_db(parent, keys, targets, 18, k=k)
    bases, off = concat_reads(seqs)
    return parent, keys, targets, odb, HitModel(odb, keys, targets, k), bases, off, where


@pytest.mark.parametrize("k", [30, 31])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_long_path_at_a_small_cut(kind, k):
    """KID_OPT_LONG_RECORD_KMERS = 256: records of 257, 511, 512, 513 and 769 windows take kid_long_plan / hits / fold
    (one, two, two, three and four tiles of 256), 150-base reads between them stay with the classify kernels.  Database
    k-mers at windows 255, 256, 511 and 512 (the last and first lane of a tile) under targets whose fold order matters,
    an N whose 30 / 31 windows without a k-mer lie across 255 | 256, lower case across 511 | 512.  Per-record results,
    gcount, ucount, lookups and hits are the oracle's, for host buffers and for a batch resident on the device."""
    parent, keys, targets, odb, model, bases, off, where = edge_case(
        k, [257, 511, 512, 513, 769], [255, 256, 511, 512], n_at={3: 270}, lower_at={2: 511, 4: 511}, short=150)
    assert where[-1] == off.size - 2
    hits = model.batch(bases, off)
    per = np.diff(hits.offsets.astype(np.int64))
    assert [int(per[r]) for r in where] == [2, 2, 3, 2, 4]
    assert any(model.fold(hits.of(r)[1]) != model.fold(hits.of(r)[1][::-1]) for r in where)  # the fold order matters
    assert {255, 256} <= set(range(270 - k + 1, 271)) and int(hits.n_kmers[where[3]]) == 513 - k
    os_ = ob.OracleSample(odb)
    exp = os_.classify(bases, off)
    eg, eu = os_.counts()
    est = os_.stats()
    assert len(set(exp[where].tolist())) > 1 and all(exp[where] > 0)
    db = KmerDB(keys, targets, parent, k=k, log2_slots=18, flags=KINDS[kind])
    for entry in ("host_buffers", "device_resident"):
        s = db.sample()
        s.set_option(_lib.KID_OPT_LONG_RECORD_KMERS, 256)
        if entry == "host_buffers":
            got = s.classify(bases, off)
        else:
            import torch
            pad = np.zeros(bases.size + 64, np.uint8)
            pad[:bases.size] = bases
            d_b, d_o = torch.from_numpy(pad).cuda(), torch.from_numpy(off.view(np.int64)).cuda()
            d_out = torch.full((off.size - 1,), -1, dtype=torch.int32, device="cuda")
            s.classify_device(d_b.data_ptr(), bases.size, d_o.data_ptr(), off.size - 1, d_out=d_out.data_ptr())
            torch.cuda.synchronize()
            got = d_out.cpu().numpy().view(np.uint32)
        assert np.array_equal(got, exp), entry
        g, u = s.end()
        assert np.array_equal(g, eg) and np.array_equal(u, eu), entry
        st = s.stats()
        assert st["lookups"] == est["lookups"] and st["hits"] == est["hits"] and st["reads"] == off.size - 1, entry
        s.close()
    db.close()


@pytest.mark.parametrize("k", [30, 31])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_hits_at_wave_tile_edges(kind, k):
    """reads of 63, 64, 65, 127, 128, 129 and 193 windows (one tile less one window .. three tiles and one window),
    database k-mers at windows 63, 64, 127 and 128, an N whose windows without a k-mer lie across 63 | 64: the hit
    lists are the model's and explain the classify path"""
    parent, keys, targets, odb, model, bases, off, where = edge_case(
        k, [63, 64, 65, 127, 128, 129, 193], [63, 64, 127, 128], n_at={5: 70}, lower_at={}, short=k + 20)
    exp = model.batch(bases, off)
    per = np.diff(exp.offsets.astype(np.int64))
    assert [int(per[r]) for r in where] == [0, 1, 2, 2, 3, 2, 4]
    assert {63, 64} <= set(range(70 - k + 1, 71)) and int(exp.n_kmers[where[5]]) == 129 - k
    for r, last in zip(where, [None, 63, 64, 64, 127, 128, 128]):
        assert (int(exp.of(r)[0][-1]) if last is not None else None) == last
    db = KmerDB(keys, targets, parent, k=k, log2_slots=18, flags=KINDS[kind])
    same_hits(db.read_hits(bases, off), exp, "%s k=%d" % (kind, k))
    cross_check(db, bases, off)
    db.close()
