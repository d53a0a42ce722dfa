"""Closing a sample (kid_sample_end / _gcount / _ucount_range / _end_merged): whatever the sample still has in flight, on
whichever stream, the counters handed back are the oracle's.  Exact: integers."""
import numpy as np
import pytest
import torch

import short_sample_cases as sc
from kmer_id_amd import KidError, end_merged

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def db():
    d = sc.new_db()
    yield d
    d.close()


@pytest.fixture(scope="module")
def dev_reads():
    _, _, _, bases, off = sc.world()
    d_bases = torch.zeros(bases.size + 64, dtype=torch.uint8, device="cuda:0")
    d_bases[:bases.size] = torch.from_numpy(bases.copy()).to("cuda:0")
    d_off = torch.from_numpy(off.astype(np.int64)).to("cuda:0")
    torch.cuda.synchronize()
    return d_bases, d_off


def test_close_without_a_launch(db):
    s = db.sample()
    g, u = s.end()
    assert not g.any() and not u.any()
    s.close()


def test_close_after_one_launch(db, dev_reads):
    d_bases, _ = dev_reads
    s = db.sample()
    out = torch.zeros(sc.N_READS, dtype=torch.int32, device="cuda:0")
    st = torch.cuda.Stream(device="cuda:0")
    s.classify_fixed_device(d_bases.data_ptr(), sc.READ_LEN, sc.N_READS, d_out=out.data_ptr(), stream=st.cuda_stream)
    got = s.end()  # (no synchronise of ours in front of it)
    finals, g, u = sc.expected(1)
    assert sc.same(got, (g, u))
    assert np.array_equal(out.cpu().numpy().view(np.uint32), finals)  # the launch is through when the close returns
    s.close()


def test_close_after_launches_on_two_caller_streams(db, dev_reads):
    d_bases, _ = dev_reads
    s = db.sample()
    outs = [torch.zeros(sc.N_READS, dtype=torch.int32, device="cuda:0") for _ in range(2)]
    streams = [torch.cuda.Stream(device="cuda:0") for _ in range(2)]
    for out, st in zip(outs, streams):
        s.classify_fixed_device(d_bases.data_ptr(), sc.READ_LEN, sc.N_READS, d_out=out.data_ptr(), stream=st.cuda_stream)
    got = s.end()
    finals, g, u = sc.expected(2)
    assert sc.same(got, (g, u))
    for out in outs:
        assert np.array_equal(out.cpu().numpy().view(np.uint32), finals)
    s.close()


def test_close_while_a_host_buffer_batch_is_in_flight(db):
    _, _, _, bases, off = sc.world()
    s = db.sample()
    b, o = bases.copy(), off.copy()
    out = np.full(sc.N_READS, 0xFFFFFFFF, np.uint32)
    ticket = s.classify_async(b, o, out=out)
    got = s.end()  # no wait(ticket) in front of it
    finals, g, u = sc.expected(1)
    assert sc.same(got, (g, u))
    assert np.array_equal(out, finals)  # the batch's results are in the caller's array when the close returns
    s.wait(ticket)
    s.close()


def test_close_after_the_log_was_switched_off(db):
    bases, off = sc.key_reads(1024, 10)  # 300 bases of ten database keys each: more than 8 hits per read
    o = sc.Oracle()
    s = db.sample()
    assert s.log_state()["has_log"]
    for _ in range(2):  # the pass of the first read-out finds the rate and takes the log away; the second batch goes without
        assert np.array_equal(s.classify(bases, off), o.classify(bases, off))
        g = s.gcount()
        half = (s.seen_bytes() * 8 // 2) // 128 * 128
        u = s.ucount_range(0, half) + s.ucount_range(half, s.seen_bytes() * 8)
        assert sc.same((g, u), o.counts())
    assert not s.log_state()["logging"]
    assert np.array_equal(s.classify(bases, off), o.classify(bases, off))
    assert sc.same(s.end(), o.counts())
    s.close()


def test_end_reset_classify_end_again(db):
    _, _, _, bases, off = sc.world()
    s = db.sample()
    finals, g, u = sc.expected(1)
    for _ in range(2):
        assert np.array_equal(s.classify(bases, off), finals)
        assert sc.same(s.end(), (g, u))
        with pytest.raises(KidError) as e:
            s.classify(bases, off)
        assert e.value.status == -10  # KID_ERR_STATE: ended
        s.reset()
    assert sc.same(s.end(), (np.zeros_like(g), np.zeros_like(u)))
    s.close()


def test_gcount_alone_then_ucount_over_two_halves(db):
    _, _, _, bases, off = sc.world()
    s = db.sample()
    s.classify(bases, off, want_final=False)
    _, g, u = sc.expected(1)
    assert np.array_equal(s.gcount(), g)
    bits = s.seen_bytes() * 8
    half = (bits // 2) // 128 * 128
    assert 0 < half < bits
    lo, hi = s.ucount_range(0, half), s.ucount_range(half, bits)
    assert lo.any() and hi.any() and np.array_equal(lo + hi, u)
    assert np.array_equal(s.ucount_range(0, bits), u) and not s.ucount_range(half, half).any()
    s.classify(bases, off, want_final=False)  # the sample is still open
    assert sc.same(s.end(), sc.expected(2)[1:])
    s.close()


def test_end_merged_over_two_samples_on_one_device(db):
    _, _, _, bases, off = sc.world()
    a, b = db.sample(), db.sample()
    h = off[sc.N_READS // 2]
    a.classify(bases[:h], off[:sc.N_READS // 2 + 1], want_final=False)
    b.classify(bases[h:], off[sc.N_READS // 2:] - h, want_final=False)
    assert sc.same(end_merged([a, b]), sc.expected(1)[1:])
    a.close(), b.close()


def test_error_words_surface_at_the_close(db, dev_reads):
    d_bases, d_off = dev_reads
    n = 64
    start = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    stop = torch.full((n,), sc.READ_LEN - 1, dtype=torch.int32, device="cuda:0")
    stop[5] = sc.READ_LEN  # one past the read: only the device sees it
    torch.cuda.synchronize()
    s = db.sample()
    s.classify_device(d_bases.data_ptr(), n * sc.READ_LEN, d_off.data_ptr(), n, d_start=start.data_ptr(), d_stop=stop.data_ptr())
    for call in (s.gcount, s.end):
        with pytest.raises(KidError) as e:
            call()
        assert e.value.status == -1 and "outside the read" in str(e.value)  # KID_ERR_ARG, as before
    s.close()
