"""Mask low-quality bases (kid_mask.hip.h; KID_OPT_MIN_BASE_QUALITY, KID_DB_OPT_MIN_BASE_QUALITY, kid_mask_batch*):
a base whose quality byte, read as signed char, is below Q + 33 is read as 'N'.  The defining property, checked
everywhere: a call with the option on equals the same call with the option off on a text that numpy masked
(seq[q.view(int8) < Q + 33] = 'N'), and both equal the oracle on that text."""
import numpy as np
import pytest

import kmer_id_amd
from kmer_id_amd import KID_DB_OPT_MIN_BASE_QUALITY, KID_FLAG_U_IS_T, KID_OPT_MIN_BASE_QUALITY, KmerDB
from base_quality_cases import block_records, build_block, kernel_case, mask_block, np_mask, records_of
from helpers import K, ob, oracle_db, small_db
from read_hits_model import HitModel
from test_gpu_fastq_blocks import oracle_fastq

pytestmark = pytest.mark.gpu

RULE = (2, 20)


@pytest.fixture(scope="module")
def dbs():
    parent, cum, keys, targets = small_db(1e-3)
    odb = oracle_db(parent, keys, targets, 20)
    db = KmerDB(keys, targets, parent, k=K, log2_slots=20)
    yield parent, cum, keys, targets, odb, db
    db.close()


@pytest.fixture(scope="module")
def block(dbs):
    """the records, their FASTQ block (CR LF lines, blank lines, every seq_off x qual_off alignment) and, per Q, the
    host-masked text with the oracle's answers on it; the unmasked answers under Q = 0"""
    parent, cum, keys, targets, odb, db = dbs
    records, aligns = block_records(odb, keys, targets, parent, cum)
    text, recs = build_block(records, aligns, crlf_every=5, blank_every=7)
    text.setflags(write=False)
    assert len({(int(r[0]) % 16, int(r[2]) % 16) for r in recs}) == 256
    seqs, quals = records_of(text, recs)
    exp = {}
    for q in (0, 2, 20, 40):
        masked, n = mask_block(text, recs, q)
        exp[q] = (masked, n, oracle_fastq(odb, records_of(masked, recs)[0], quals))
    return text, recs, quals, exp


def classify_block(db, text, recs, q=0):
    s = db.sample()
    if q is not None:
        s.set_option(KID_OPT_MIN_BASE_QUALITY, q)
    final, start, stop = s.classify_fastq(text, recs)
    n_masked = s.masked_bases()
    g, u = s.end()
    s.close()
    return final, start, stop, g, u, n_masked


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------ 1. the kernel alone
@pytest.fixture(scope="module")
def reads():
    return kernel_case()


@pytest.mark.parametrize("q", [1, 2, 20, 40, 93])
def test_mask_batch_equals_numpy_byte_for_byte(dbs, reads, q):
    db = dbs[-1]
    bases, quals, off = reads
    keep_b, keep_q = bases.copy(), quals.copy()
    exp, n = np_mask(bases, quals, q)
    assert 0 < n < bases.size
    got, got_n = db.mask_low_quality(bases, quals, off, q)
    assert np.array_equal(got, exp) and got_n == n
    assert np.array_equal(bases, keep_b) and np.array_equal(quals, keep_q)  # the caller's arrays are not written
    # a batch that starts inside the text: nothing in front of offsets[0] is touched
    a = int(off[40])
    got, got_n = db.mask_low_quality(bases, quals, off[40:], q)
    assert np.array_equal(got[:a], bases[:a]) and np.array_equal(got[a:], exp[a:])
    assert got_n == int((quals[a:].view(np.int8) < q + 33).sum())


def test_mask_batch_off_and_out_of_range(dbs, reads):
    db = dbs[-1]
    bases, quals, off = reads
    got, n = db.mask_low_quality(bases, quals, off, 0)
    assert np.array_equal(got, bases) and n == 0
    for bad in (-1, 94):
        with pytest.raises(kmer_id_amd.KidError) as e:
            db.mask_low_quality(bases, quals, off, bad)
        assert e.value.status == -1  # KID_ERR_ARG
        with pytest.raises(kmer_id_amd.KidError) as e:
            db.mask_low_quality_device(0, 0, 0, 1, bad)
        assert e.value.status == -1


@pytest.mark.parametrize("q", [2, 40])
def test_mask_batch_device_in_place_between_guards(dbs, reads, q):
    import torch
    db = dbs[-1]
    bases, quals, off = reads
    n = bases.size
    exp, cnt = np_mask(bases, quals, q)
    buf = torch.full((64 + n + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    buf[64:64 + n] = torch.from_numpy(bases).cuda()
    qbuf = torch.full((7 + n + 9,), 0x21, dtype=torch.uint8, device="cuda")  # (qualities at another alignment than the bases)
    qbuf[7:7 + n] = torch.from_numpy(quals).cuda()
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    counter = torch.full((1,), 5, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for calls in (1, 2):
        db.mask_low_quality_device(buf.data_ptr() + 64, qbuf.data_ptr() + 7, d_off.data_ptr(), off.size - 1, q, counter.data_ptr())
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert (got[:64] == 0x5A).all() and (got[64 + n:] == 0x5A).all()  # the guards
        assert np.array_equal(got[64:64 + n], exp)
        assert int(counter.item()) == 5 + calls * cnt  # added to, not reset
    assert (qbuf.cpu().numpy()[7:7 + n] == quals).all()
    db.mask_low_quality_device(buf.data_ptr() + 64, qbuf.data_ptr() + 7, d_off.data_ptr(), off.size - 1, 0)  # off: nothing runs
    db.mask_low_quality_device(buf.data_ptr() + 64, qbuf.data_ptr() + 7, d_off.data_ptr(), off.size - 1, q)  # no counter
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy()[64:64 + n], exp) and int(counter.item()) == 5 + 2 * cnt


# ------------------------------------------------------------------ 2. the FASTQ block forms
def test_the_inputs_decide_something(dbs, block):
    """on the CPU, through the oracle: masking at Q = 20 changes final targets and loses hits"""
    parent, cum, keys, targets, odb, db = dbs
    text, recs, quals, exp = block
    plain, masked = exp[0][2], exp[20][2]
    assert exp[0][1] == 0 and np.array_equal(exp[0][0], text)
    assert np.array_equal(plain[1], masked[1]) and np.array_equal(plain[2], masked[2])  # start / stop: the quality line alone
    assert int((plain[3] != masked[3]).sum()) >= 50
    hm = HitModel(odb, keys, targets, K)
    kept = np.flatnonzero(plain[0] == 1)
    count = []
    for t in (text, exp[20][0]):
        seqs = records_of(t, recs)[0]
        data = np.frombuffer(b"".join(seqs[i] for i in kept), np.uint8)
        off = np.zeros(kept.size + 1, np.uint64)
        off[1:] = np.cumsum([len(seqs[i]) for i in kept])
        h = hm.batch(data, off, plain[1][kept], plain[2][kept])
        count.append((int(h.offsets[-1]), int(h.n_kmers.sum())))
    assert count[1][0] < count[0][0] - 200 and count[1][1] < count[0][1]  # hits are lost, and windows


@pytest.mark.parametrize("q", [2, 20, 40])
def test_classify_fastq_option_equals_masked_text_and_oracle(dbs, block, q):
    db = dbs[-1]
    text, recs, quals, exp = block
    masked, n_masked, (called, start, stop, final, g, u) = exp[q]
    assert n_masked > 0
    on = classify_block(db, text, recs, q)
    off = classify_block(db, masked, recs, 0)
    assert same(on[:5], off[:5])
    assert on[5] == n_masked and off[5] == 0
    kept = called == 1
    assert np.array_equal(on[2] - on[1] >= K, kept)
    assert np.array_equal(on[1][kept], start[kept]) and np.array_equal(on[2][kept], stop[kept])
    assert np.array_equal(on[0], final) and np.array_equal(on[3], g) and np.array_equal(on[4], u)
    if q == 20:
        assert not np.array_equal(on[0], exp[0][2][3])  # (and it is not what the unmasked text gives)


@pytest.mark.parametrize("q", [2, 20, 40])
def test_read_hits_and_support_option_equal_masked_text(dbs, block, q):
    parent, cum, keys, targets, odb, db = dbs
    text, recs, quals, exp = block
    masked = exp[q][0]
    db.set_option(KID_DB_OPT_MIN_BASE_QUALITY, q)
    try:
        h_on = db.read_hits_fastq(text, recs)
        t_on = db.sample()
        s_on = db.read_support_fastq(text, recs, *RULE, tally=t_on)
    finally:
        db.set_option(KID_DB_OPT_MIN_BASE_QUALITY, 0)
    h_off = db.read_hits_fastq(masked, recs)
    t_off = db.sample()
    s_off = db.read_support_fastq(masked, recs, *RULE, tally=t_off)
    assert h_on.offsets.tobytes() == h_off.offsets.tobytes() and h_on.n_kmers.tobytes() == h_off.n_kmers.tobytes()
    for f in ("pos", "target", "entry"):
        assert getattr(h_on, f).tobytes() == getattr(h_off, f).tobytes(), f
    assert s_on.tobytes() == s_off.tobytes()
    assert same(t_on.end(), t_off.end())
    assert t_on.masked_bases() == 0  # (a tally is no FASTQ block of the sample's)
    t_on.close(); t_off.close()
    # ... and the oracle's hits on the masked text: pos counted from the first byte of the read, n_kmers smaller
    called, start, stop = exp[q][2][:3]
    kept = np.flatnonzero(called == 1)
    seqs = records_of(masked, recs)[0]
    data = np.frombuffer(b"".join(seqs[i] for i in kept), np.uint8)
    off = np.zeros(kept.size + 1, np.uint64)
    off[1:] = np.cumsum([len(seqs[i]) for i in kept])
    m = HitModel(odb, keys, targets, K).batch(data, off, start[kept], stop[kept])
    per_read = np.zeros(len(seqs), np.uint64)
    per_read[kept] = np.diff(m.offsets)
    nk = np.zeros(len(seqs), np.uint32)
    nk[kept] = m.n_kmers
    assert np.array_equal(np.diff(h_on.offsets), per_read) and np.array_equal(h_on.n_kmers, nk)
    assert np.array_equal(h_on.pos, m.pos) and np.array_equal(h_on.target, m.target) and np.array_equal(h_on.entry, m.entry)
    assert np.array_equal(s_on["n_kmers"], nk) and np.array_equal(s_on["final"], exp[q][2][3])
    if q == 20:
        plain = db.read_hits_fastq(text, recs)
        assert int(plain.offsets[-1]) > int(h_on.offsets[-1]) and int(plain.n_kmers.sum()) > int(nk.sum())


def test_u_is_t_database(dbs, block):
    parent, cum, keys, targets, odb, db = dbs
    text, recs, quals, exp = block
    masked, n_masked = exp[20][0], exp[20][1]
    udb = KmerDB(keys, targets, parent, k=K, log2_slots=20, flags=KID_FLAG_U_IS_T)
    uodb = oracle_db(parent, keys, targets, 20, flags=ob.KO_FLAG_U_IS_T)
    called, start, stop, final, g, u = oracle_fastq(uodb, records_of(masked, recs)[0], quals)
    on = classify_block(udb, text, recs, 20)
    assert same(on[:5], classify_block(udb, masked, recs, 0)[:5]) and on[5] == n_masked
    assert np.array_equal(on[0], final) and np.array_equal(on[3], g) and np.array_equal(on[4], u)
    assert not np.array_equal(final, exp[20][2][3])  # the U records count here
    udb.set_option(KID_DB_OPT_MIN_BASE_QUALITY, 20)
    h_on = udb.read_hits_fastq(text, recs)
    rep = udb.replicate(0)  # the option is not copied
    h_rep = rep.read_hits_fastq(masked, recs)
    assert h_on.offsets.tobytes() == h_rep.offsets.tobytes() and h_on.pos.tobytes() == h_rep.pos.tobytes()
    assert rep.read_hits_fastq(text, recs).offsets.tobytes() != h_on.offsets.tobytes()
    rep.close(); udb.close()


# ------------------------------------------------------------------ 3. splits and state
def test_one_call_and_three_calls(dbs, block):
    db = dbs[-1]
    text, recs, quals, exp = block
    keep = text.copy()
    one = classify_block(db, text, recs, 20)
    s = db.sample()
    s.set_option(KID_OPT_MIN_BASE_QUALITY, 20)
    n = recs.shape[0]
    parts = [s.classify_fastq(text, recs[a:b]) for a, b in ((0, 700), (700, 701), (701, n))]
    assert all(np.array_equal(np.concatenate([p[i] for p in parts]), one[i]) for i in range(3))
    assert s.masked_bases() == one[5] == exp[20][1]
    assert same(s.end(), one[3:5])
    s.close()
    db.set_option(KID_DB_OPT_MIN_BASE_QUALITY, 20)
    whole = db.read_support_fastq(text, recs, *RULE)
    pieces = [db.read_support_fastq(text, recs[a:b], *RULE) for a, b in ((0, 1), (1, 2900), (2900, n))]
    db.set_option(KID_DB_OPT_MIN_BASE_QUALITY, 0)
    assert np.concatenate(pieces).tobytes() == whole.tobytes()
    assert np.array_equal(text, keep)


def test_five_blocks_on_one_sample_and_the_option_switched_off(dbs, block):
    parent, cum, keys, targets, odb, db = dbs
    text, recs, quals, exp = block
    seqs = records_of(text, recs)[0]
    n = len(seqs)
    cuts = [(0, 900), (900, 1000), (1000, 2500), (2500, 3300), (3300, n)]
    blocks = [build_block(list(zip(seqs[a:b], quals[a:b])), crlf_every=3 + i, blank_every=4 + i) for i, (a, b) in enumerate(cuts)]
    s, ref = db.sample(), db.sample()
    s.set_option(KID_OPT_MIN_BASE_QUALITY, 20)
    total = 0
    for t, r in blocks:
        keep = t.copy()
        masked, cnt = mask_block(t, r, 20)
        total += cnt
        assert same(s.classify_fastq(t, r), ref.classify_fastq(masked, r))
        assert np.array_equal(t, keep)
    assert s.masked_bases() == total and ref.masked_bases() == 0
    assert same(s.end(), ref.end())
    # reset: the counter starts again, the option stays; set to 0: the unmasked results again
    s.reset(); ref.reset()
    assert s.masked_bases() == 0
    t, r = blocks[1]
    assert same(s.classify_fastq(t, r), ref.classify_fastq(mask_block(t, r, 20)[0], r)) and s.masked_bases() == mask_block(t, r, 20)[1]
    assert same(s.gcount(), ref.gcount())
    s.reset(); ref.reset()
    s.set_option(KID_OPT_MIN_BASE_QUALITY, 0)
    assert same(s.classify_fastq(t, r), ref.classify_fastq(t, r)) and s.masked_bases() == 0
    assert same(s.end(), ref.end())
    for bad in (-1, 94):
        with pytest.raises(kmer_id_amd.KidError) as e:
            s.set_option(KID_OPT_MIN_BASE_QUALITY, bad)
        assert e.value.status == -1
        with pytest.raises(kmer_id_amd.KidError) as e:
            db.set_option(KID_DB_OPT_MIN_BASE_QUALITY, bad)
        assert e.value.status == -1
    with pytest.raises(kmer_id_amd.KidError):
        db.set_option(77, 1)
    s.close(); ref.close()


def test_lines_out_of_order_are_refused_under_the_option_only(dbs):
    db = dbs[-1]
    seq = b"ACGTTGCAAGGCTTAACCGGTTAACGTACGTAGCTAGCTAACGT"
    text = np.frombuffer(b"@a\n" + seq + b"\n+\n" + b"I" * len(seq) + b"\n@b\n" + seq + b"\n+\n" + b"I" * len(seq) + b"\n", np.uint8)
    so, L = 3, len(seq)
    qo = so + L + 3
    so2 = qo + L + 4
    qo2 = so2 + L + 3
    good = np.array([[so, L, qo, L], [so2, L, qo2, L]], np.uint32)
    cases = {"quality inside its sequence": np.array([[so, L, so + 10, L]], np.uint32),
             "quality in front of its sequence": np.array([[qo, L, so, L]], np.uint32),
             "records in descending order": good[::-1].copy(),
             "the next sequence inside a quality line": np.array([[so, L, qo, L], [qo + 5, L, qo2, L]], np.uint32)}
    s = db.sample()
    s.classify_fastq(text, good)
    for name, recs in cases.items():
        s.classify_fastq(text, recs)  # option off: accepted as ever
        db.read_hits_fastq(text, recs)
    s.set_option(KID_OPT_MIN_BASE_QUALITY, 20)
    db.set_option(KID_DB_OPT_MIN_BASE_QUALITY, 20)
    try:
        s.classify_fastq(text, good)
        db.read_hits_fastq(text, good)
        for name, recs in cases.items():
            for call in (lambda: s.classify_fastq(text, recs), lambda: db.read_hits_fastq(text, recs),
                         lambda: db.read_support_fastq(text, recs, *RULE)):
                with pytest.raises(kmer_id_amd.KidError) as e:
                    call()
                assert e.value.status == -1, name
    finally:
        db.set_option(KID_DB_OPT_MIN_BASE_QUALITY, 0)
    s.end()
    s.close()
