"""Mask low-complexity sequence (kid_lowc.hip.h; KID_OPT_LOW_COMPLEXITY, KID_DB_OPT_LOW_COMPLEXITY, kid_lowc_batch*)
against the Python model (low_complexity_model.py): the kernels alone with the WHOLE text compared, so that a stray
store shows, and the FASTQ forms, where a call with the option on equals the same call with the option off on text the
model masked."""
import numpy as np
import pytest

import kmer_id_amd
from kmer_id_amd import (KID_DB_OPT_LOW_COMPLEXITY, KID_DB_OPT_MIN_BASE_QUALITY, KID_FLAG_U_IS_T, KID_OPT_LOW_COMPLEXITY,
                         KID_OPT_MIN_BASE_QUALITY, KmerDB)
from base_quality_cases import build_block, hit_reads, records_of
from base_quality_cases import mask_block as quality_mask_block
from helpers import K, oracle_db, small_db, synth
from low_complexity_model import mask_block, mask_reads
from test_gpu_fastq_blocks import oracle_fastq

pytestmark = pytest.mark.gpu

CHUNK = 512  # KID_LOWC_CHUNK: positions a lane decides of a line that is split
LENGTHS = [0, 1, 2, 3, 4, 31, 32, 33, 63, 64, 65, 150, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1]
LONG = 20000
THRESHOLDS = [1, 20, 310, 1000]
RULE = (2, 20)
PERIODS = [b"A", b"CA", b"GAT", b"t", b"gC", b"U", b"AU"]


def plant(rng, s, at, run, per):
    for j in range(max(0, at), min(len(s), at + run)):
        s[j] = per[(j - at) % len(per)]


def kernel_case(seed=19):
    """reads back to back without a gap -> (bases, offsets): every length of LENGTHS at every start alignment mod 16 (a
    read of 0..15 bases in front of every repetition moves it there), random text over a dirty alphabet with runs of
    period 1, 2 and 3 planted -- N, lower case, other bytes and U among them -- then one record of LONG bases at an odd
    address with a run across every chunk edge."""
    rng = np.random.default_rng(seed)
    lens, total = [], 0
    for a in range(16):
        pad = (a - total) % 16
        lens += [pad] + LENGTHS
        total += pad + sum(LENGTHS)
    lens += [(5 - total) % 16, LONG]
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    bases = rng.choice(np.frombuffer(b"ACGTACGTACGTACGTacgtNU", np.uint8), int(off[-1]))
    for i, ln in enumerate(lens[:-1]):
        a = int(off[i])
        for _ in range(int(rng.integers(0, 3)) if ln >= 7 else 0):
            plant(rng, bases[a:a + ln], int(rng.integers(-10, ln)), int(rng.integers(5, 90)), PERIODS[int(rng.integers(len(PERIODS)))])
        if ln >= 40 and i % 3 == 0:  # ... and something else inside a run
            bases[a + ln // 2] = rng.choice(np.frombuffer(b"N-\x00\xc1", np.uint8))
    long_rec = bases[int(off[-2]):]
    for e in range(CHUNK, LONG, CHUNK):  # across every chunk edge, at every phase of the run against it
        c = e // CHUNK
        plant(rng, long_rec, e - 20 - c % 37, 45 + c % 23, PERIODS[c % 3])
    long_rec[7 * CHUNK] = ord("N")
    long_rec[9 * CHUNK - 1] = ord("a")
    long_rec[11 * CHUNK + 1] = ord("-")
    starts = {(int(off[i]) % 16, lens[i]) for i in range(len(lens))}
    assert all((a, ln) in starts for a in range(16) for ln in LENGTHS if ln) and int(off[-2]) % 2 == 1
    bases.setflags(write=False)
    return bases, off


@pytest.fixture(scope="module")
def dbs():
    parent, cum, keys, targets = small_db(1e-3)
    odb = oracle_db(parent, keys, targets, 20)
    db = KmerDB(keys, targets, parent, k=K, log2_slots=20)
    udb = KmerDB(keys, targets, parent, k=K, log2_slots=20, flags=KID_FLAG_U_IS_T)
    yield parent, cum, keys, targets, odb, udb, db
    udb.close()
    db.close()


@pytest.fixture(scope="module")
def reads():
    """the kernel case and the model's answer per (T, u_is_t), computed once"""
    bases, off = kernel_case()
    exp = {(t, u): mask_reads(bases, off, t, u) for t in THRESHOLDS for u in (False, True) if not u or t == 20}
    for v in exp.values():
        v[0].setflags(write=False)
    return bases, off, exp


# ------------------------------------------------------------------ 1. the kernels alone
@pytest.mark.parametrize("t", THRESHOLDS)
def test_batch_equals_the_model_byte_for_byte(dbs, reads, t):
    db = dbs[-1]
    bases, off, exp = reads
    want, n = exp[(t, False)]
    assert (0 < n < bases.size) if t < 310 else n == 0  # (62 equal triplets: 10 * 1891 = 310 * 61 -- nothing is low from 310 on)
    got, got_n = db.mask_low_complexity(bases, off, t)
    assert np.array_equal(got, want) and got_n == n
    again, again_n = db.mask_low_complexity(bases, off, t)
    assert again.tobytes() == got.tobytes() and again_n == got_n  # two runs byte-identical
    # reads of up to CHUNK bases alone: no line is split and the kernel writes in place -- the same bytes
    z = int(off[15])
    assert int(np.diff(off[:16].astype(np.int64)).max()) == CHUNK
    got, got_n = db.mask_low_complexity(bases, off[:16], t)
    assert np.array_equal(got[:z], want[:z]) and np.array_equal(got[z:], bases[z:]) and got_n == int((want[:z] != bases[:z]).sum())
    # a batch that starts inside the text: nothing in front of offsets[0] or behind offsets[n] is touched
    a = int(off[40])
    got, got_n = db.mask_low_complexity(bases, off[40:-1], t)
    assert np.array_equal(got[:a], bases[:a]) and np.array_equal(got[a:int(off[-2])], want[a:int(off[-2])])
    assert np.array_equal(got[int(off[-2]):], bases[int(off[-2]):])
    assert got_n == int((want[a:int(off[-2])] != bases[a:int(off[-2])]).sum())


def test_u_counts_as_a_base_under_the_flag_alone(dbs, reads):
    udb, db = dbs[-2], dbs[-1]
    bases, off, exp = reads
    want, n = exp[(20, True)]
    assert not np.array_equal(want, exp[(20, False)][0])
    got, got_n = udb.mask_low_complexity(bases, off, 20)
    assert np.array_equal(got, want) and got_n == n
    line = np.frombuffer(b"UUUUUUUUUU", np.uint8)
    assert bytes(udb.mask_low_complexity(line, [0, 10], 20)[0]) == b"N" * 10
    assert bytes(db.mask_low_complexity(line, [0, 10], 20)[0]) == bytes(line)


def test_hand_cases_and_lines_back_to_back(dbs):
    db = dbs[-1]
    for line, want in ((b"AAAAAA", b"AAAAAA"), (b"AAAAAAA", b"NNNNNNN"), (b"NNNNAAAAAAANNNN", b"NNNNNNNNNNNNNNN")):
        got, n = db.mask_low_complexity(np.frombuffer(line, np.uint8), [0, len(line)], 20)
        assert bytes(got) == want and n == sum(a != b for a, b in zip(line, want))
    a40 = np.frombuffer(b"A" * 40, np.uint8)
    assert db.mask_low_complexity(a40, [0, 40], 100)[1] == 40
    got, n = db.mask_low_complexity(a40, [0, 20, 40], 100)  # two lines of 20: neither sees the other (the model's test says why 100)
    assert n == 0 and bytes(got) == bytes(a40)
    assert db.mask_low_complexity(a40, [0, 6, 12, 18, 24, 30, 36, 40], 20)[1] == 0
    assert db.mask_low_complexity(a40, [0, 0, 0, 40, 40], 20)[1] == 40  # empty reads around


def test_off_and_out_of_range(dbs, reads):
    db = dbs[-1]
    bases, off, exp = reads
    got, n = db.mask_low_complexity(bases, off, 0)
    assert np.array_equal(got, bases) and n == 0
    for bad in (-1, 1001):
        with pytest.raises(kmer_id_amd.KidError) as e:
            db.mask_low_complexity(bases, off, bad)
        assert e.value.status == -1  # KID_ERR_ARG
        with pytest.raises(kmer_id_amd.KidError) as e:
            db.mask_low_complexity_device(0, 0, 1, bad)
        assert e.value.status == -1
        with pytest.raises(kmer_id_amd.KidError) as e:
            db.set_option(KID_DB_OPT_LOW_COMPLEXITY, bad)
        assert e.value.status == -1
        s = db.sample()
        with pytest.raises(kmer_id_amd.KidError) as e:
            s.set_option(KID_OPT_LOW_COMPLEXITY, bad)
        assert e.value.status == -1
        s.close()


@pytest.mark.parametrize("t", [1, 20])
def test_device_form_in_place_between_guards(dbs, reads, t):
    """(the device form does not split the long record: one lane walks all of it -- the same bytes as the split host form)"""
    import torch
    db = dbs[-1]
    bases, off, exp = reads
    n = bases.size
    want, cnt = exp[(t, False)]
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    counter = torch.full((1,), 5, dtype=torch.int64, device="cuda")
    first = None
    for calls, lead in ((1, 64), (2, 67)):  # (the text at two alignments)
        buf = torch.full((lead + n + 64,), 0x41, dtype=torch.uint8, device="cuda")  # guards of 'A': bases, if anything read them
        buf[lead:lead + n] = torch.from_numpy(np.array(bases)).cuda()
        torch.cuda.synchronize()
        db.mask_low_complexity_device(buf.data_ptr() + lead, d_off.data_ptr(), off.size - 1, t, counter.data_ptr())
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert (got[:lead] == 0x41).all() and (got[lead + n:] == 0x41).all()
        assert np.array_equal(got[lead:lead + n], want)
        assert int(counter.item()) == 5 + calls * cnt  # added to, not reset
        first = got[lead:lead + n].tobytes() if first is None else first
        assert got[lead:lead + n].tobytes() == first
    keep = buf.clone()
    db.mask_low_complexity_device(buf.data_ptr() + 67, d_off.data_ptr(), off.size - 1, 0, counter.data_ptr())  # off: nothing runs
    db.mask_low_complexity_device(buf.data_ptr() + 67, d_off.data_ptr(), 0, t, counter.data_ptr())  # no reads
    torch.cuda.synchronize()
    assert torch.equal(buf, keep) and int(counter.item()) == 5 + 2 * cnt


# ------------------------------------------------------------------ 2. the FASTQ block forms
T = 20
Q = 20


@pytest.fixture(scope="module")
def block(dbs):
    """reads with hits per the oracle, a repeat planted into each (the mask takes the run and the bases around it, and
    hits with them), records of the kernel's lengths, one LONG record with runs across its chunk edges, U records; with
    mixed qualities -> text, recs, and the model's masked texts: by complexity, by quality, by quality then complexity"""
    parent, cum, keys, targets, odb, udb, db = dbs
    rng = np.random.default_rng(23)
    L = 150
    records = []
    for i, (s, q) in enumerate(hit_reads(odb, keys, targets, parent, cum, 150, r0=90000)):
        s = np.frombuffer(s, np.uint8).copy()
        if i % 5:
            plant(rng, s, int(rng.integers(0, 110)), 20 + 5 * (i % 6), PERIODS[i % 3])
        records.append((s.tobytes(), q))
    b = synth.reads(cum, parent, 200, L, K, r0=777).reshape(200, L)
    ql = synth.qualities(200, L, r0=777)
    for i in range(200):
        s = b[i].copy()
        if i % 2:
            plant(rng, s, int(rng.integers(0, 120)), int(rng.integers(8, 60)), PERIODS[int(rng.integers(len(PERIODS)))])
        if i % 7 == 0:
            s = np.frombuffer(s.tobytes().lower(), np.uint8)
        records.append((s.tobytes(), ql[i].tobytes()))
    pool = synth.reads(cum, parent, 160, L, K, r0=120000).copy()
    for e in range(CHUNK, pool.size, CHUNK):
        plant(rng, pool, e - 20 - (e // CHUNK) % 37, 45 + (e // CHUNK) % 23, PERIODS[(e // CHUNK) % 3])
    mixed = np.frombuffer(b"IIIIIIIIIIIIJH52#!\"", np.uint8)
    at = 0
    for ln in LENGTHS + [LONG]:
        records.append((pool[at:at + ln].tobytes(), rng.choice(mixed, ln).tobytes()))
        at = (at + ln) % 1000
    aligns = [None] * len(records)
    for i in range(32):  # seq_off at every alignment, twice
        s = b[i].copy()
        plant(rng, s, 10 + 3 * i, 40, PERIODS[i % 3])
        records.append((s.tobytes(), ql[i].tobytes()))
        aligns.append((i % 16, (5 * i) % 16))
    text, recs = build_block(records, aligns, crlf_every=5, blank_every=7)
    text.setflags(write=False)
    by_t, n_t = mask_block(text, recs, T)
    by_q, n_q = quality_mask_block(text, recs, Q)
    by_qt, n_qt = mask_block(by_q, recs, T)
    for m in (by_t, by_q, by_qt):  # quality lines, headers, line ends: nothing but bases of sequence lines differs
        assert all(np.array_equal(m[qo:qo + qn], text[qo:qo + qn]) for so, sl, qo, qn in recs.tolist())
    assert n_t > 2000 and n_q > 100 and n_qt > 1000 and not np.array_equal(by_qt, by_t)
    return text, recs, records_of(text, recs)[1], {"t": (by_t, n_t), "q": (by_q, n_q), "qt": (by_qt, n_qt)}


def classify_block(db, text, recs, t=0, q=0):
    s = db.sample()
    if t is not None:
        s.set_option(KID_OPT_LOW_COMPLEXITY, t)
        s.set_option(KID_OPT_MIN_BASE_QUALITY, q)
    final, start, stop = s.classify_fastq(text, recs)
    counts = (s.low_complexity_bases(), s.masked_bases())
    g, u = s.end()
    s.close()
    return final, start, stop, g, u, counts


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_classify_fastq_option_equals_masked_text_and_oracle(dbs, block):
    parent, cum, keys, targets, odb, udb, db = dbs
    text, recs, quals, exp = block
    keep = text.copy()
    masked, n = exp["t"]
    plain = classify_block(db, text, recs, None)  # no option ever set: what the parent computes
    on = classify_block(db, text, recs, T)
    off = classify_block(db, masked, recs, 0)
    assert same(on[:5], off[:5]) and on[5] == (n, 0) and off[5] == (0, 0) and plain[5] == (0, 0)
    assert same(plain[:5], classify_block(db, text, recs, 0)[:5])
    assert np.array_equal(on[1], plain[1]) and np.array_equal(on[2], plain[2])  # start / stop: the quality line alone
    assert int((on[0] != plain[0]).sum()) >= 20  # ... and it is not what the unmasked text gives
    called, start, stop, final, g, u = oracle_fastq(odb, records_of(masked, recs)[0], quals)
    assert np.array_equal(on[0], final) and np.array_equal(on[3], g) and np.array_equal(on[4], u)
    assert np.array_equal(text, keep)


def test_both_masks_are_quality_then_complexity(dbs, block):
    db = dbs[-1]
    text, recs, quals, exp = block
    (by_q, n_q), (by_qt, n_qt) = exp["q"], exp["qt"]
    on = classify_block(db, text, recs, T, Q)
    assert same(on[:5], classify_block(db, by_qt, recs, 0)[:5]) and on[5] == (n_qt, n_q)
    assert not same(on[:5], classify_block(db, exp["t"][0], recs, 0)[:5])
    db.set_option(KID_DB_OPT_MIN_BASE_QUALITY, Q)
    db.set_option(KID_DB_OPT_LOW_COMPLEXITY, T)
    try:
        h_on = db.read_hits_fastq(text, recs)
    finally:
        db.set_option(KID_DB_OPT_MIN_BASE_QUALITY, 0)
        db.set_option(KID_DB_OPT_LOW_COMPLEXITY, 0)
    h_off = db.read_hits_fastq(by_qt, recs)
    for f in ("offsets", "n_kmers", "pos", "target", "entry"):
        assert getattr(h_on, f).tobytes() == getattr(h_off, f).tobytes(), f


def test_read_hits_and_support_option_equal_masked_text(dbs, block):
    parent, cum, keys, targets, odb, udb, db = dbs
    text, recs, quals, exp = block
    masked = exp["t"][0]
    plain = db.read_hits_fastq(text, recs)
    s_plain = db.read_support_fastq(text, recs, *RULE)
    db.set_option(KID_DB_OPT_LOW_COMPLEXITY, T)
    try:
        h_on = db.read_hits_fastq(text, recs)
        t_on = db.sample()
        s_on = db.read_support_fastq(text, recs, *RULE, tally=t_on)
        rep = db.replicate(0)  # a replica starts off
        h_rep = rep.read_hits_fastq(text, recs)
        rep.close()
    finally:
        db.set_option(KID_DB_OPT_LOW_COMPLEXITY, 0)
    h_off = db.read_hits_fastq(masked, recs)
    t_off = db.sample()
    s_off = db.read_support_fastq(masked, recs, *RULE, tally=t_off)
    for f in ("offsets", "n_kmers", "pos", "target", "entry"):
        assert getattr(h_on, f).tobytes() == getattr(h_off, f).tobytes(), f
        assert getattr(h_rep, f).tobytes() == getattr(plain, f).tobytes(), f
    assert s_on.tobytes() == s_off.tobytes() and s_on.tobytes() != s_plain.tobytes()
    assert same(t_on.end(), t_off.end()) and t_on.low_complexity_bases() == 0  # (a tally is no FASTQ block of the sample's)
    t_on.close(); t_off.close()
    assert int(plain.offsets[-1]) > int(h_on.offsets[-1]) and int(plain.n_kmers.sum()) > int(h_on.n_kmers.sum())
    # the option off again: byte for byte what it was
    again = db.read_hits_fastq(text, recs)
    for f in ("offsets", "n_kmers", "pos", "target", "entry"):
        assert getattr(again, f).tobytes() == getattr(plain, f).tobytes(), f
    assert db.read_support_fastq(text, recs, *RULE).tobytes() == s_plain.tobytes()


def test_segments_fragments_and_votes_forms_equal_masked_text(dbs, block):
    """the other forms that kid_hits_stage_fastq stages; the fragment call has two blocks and an interleaved index (the
    second block holds the LONG record: the staged text takes the two passes)"""
    db = dbs[-1]
    text, recs, quals, exp = block
    masked = exp["t"][0]
    n = recs.shape[0] // 2
    r1, r2 = recs[:n], recs[n:2 * n]
    assert int(r2[:, 1].max()) == LONG

    def calls(t):
        seg = db.read_segments_fastq(t, recs, 100, 50, *RULE)
        return (seg.offsets.tobytes(), seg.records.tobytes(), db.read_fragments_fastq(t, r1, t, r2, *RULE).tobytes(),
                db.read_votes_fastq(t, recs, *RULE).tobytes())

    plain = calls(text)
    db.set_option(KID_DB_OPT_LOW_COMPLEXITY, T)
    try:
        on = calls(text)
    finally:
        db.set_option(KID_DB_OPT_LOW_COMPLEXITY, 0)
    off = calls(masked)
    assert on == off and all(a != b for a, b in zip(on[1:], plain[1:]))
    assert calls(text) == plain


def test_u_is_t_database_on_a_block(dbs, block):
    parent, cum, keys, targets, odb, udb, db = dbs
    text, recs, quals, exp = block
    masked, n = mask_block(text, recs, T, u_is_t=True)
    assert n > exp["t"][1]  # the U runs count here
    on = classify_block(udb, text, recs, T)
    assert same(on[:5], classify_block(udb, masked, recs, 0)[:5]) and on[5] == (n, 0)


def test_pieces_reset_and_switching_off(dbs, block):
    db = dbs[-1]
    text, recs, quals, exp = block
    one = classify_block(db, text, recs, T)
    s = db.sample()
    s.set_option(KID_OPT_LOW_COMPLEXITY, T)
    n = recs.shape[0]
    parts = [s.classify_fastq(text, recs[a:b]) for a, b in ((0, 100), (100, 101), (101, n))]
    assert all(np.array_equal(np.concatenate([p[i] for p in parts]), one[i]) for i in range(3))
    assert s.low_complexity_bases() == one[5][0] == exp["t"][1] and s.masked_bases() == 0
    assert same(s.end(), one[3:5])
    s.reset()
    assert s.low_complexity_bases() == 0  # reset: the counter starts again, the option stays
    ref = db.sample()
    head = recs[:120]
    assert same(s.classify_fastq(text, head), ref.classify_fastq(exp["t"][0], head))
    assert s.low_complexity_bases() == mask_block(text, head, T)[1] and same(s.gcount(), ref.gcount())
    s.reset(); ref.reset()
    s.set_option(KID_OPT_LOW_COMPLEXITY, 0)
    assert same(s.classify_fastq(text, head), ref.classify_fastq(text, head)) and s.low_complexity_bases() == 0
    assert same(s.end(), ref.end())
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
             "records in descending order": good[::-1].copy(),
             "the next sequence inside a quality line": np.array([[so, L, qo, L], [qo + 5, L, qo2, L]], np.uint32)}
    s = db.sample()
    for recs in cases.values():
        s.classify_fastq(text, recs)  # option off: accepted as ever
        db.read_hits_fastq(text, recs)
    s.set_option(KID_OPT_LOW_COMPLEXITY, T)
    db.set_option(KID_DB_OPT_LOW_COMPLEXITY, T)
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
        db.set_option(KID_DB_OPT_LOW_COMPLEXITY, 0)
    s.end()
    s.close()
