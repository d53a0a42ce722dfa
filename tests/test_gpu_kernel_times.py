"""kid_sample_kernel_times: the HIP-event time of every timed batch, beside the sum kid_sample_kernel_time gives."""
import numpy as np
import pytest

import short_sample_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sample():
    db = sc.new_db()
    s = db.sample()
    s.set_timing(True)
    yield s
    s.close()
    db.close()


def launches(s, n):
    _, _, _, bases, off = sc.world()
    for _ in range(n):
        s.classify(bases, off, want_final=False)


def test_n_launches_give_n_positive_values_that_add_up(sample):
    sample.kernel_time(), sample.kernel_times()
    launches(sample, 5)
    total, n = sample.kernel_time()
    ms, m = sample.kernel_times()
    assert n == 5 and m == 5 and ms.size == 5 and (ms > 0).all()
    assert abs(float(ms.sum()) - total) <= 1e-9 * total  # the same float32 event times, added up in float64 twice
    assert sample.kernel_time() == (0.0, 0)


def test_a_cap_below_n_reports_n_and_fills_cap(sample):
    sample.kernel_times()
    launches(sample, 4)
    ms, n = sample.kernel_times(cap=3)
    assert n == 4 and ms.size == 3 and (ms > 0).all()
    ms, n = sample.kernel_times(cap=0)  # (all four counted as reported)
    assert n == 0 and ms.size == 0


def test_a_second_query_gives_none(sample):
    sample.kernel_time(), sample.kernel_times()  # (the sample is shared: what the tests before left)
    launches(sample, 2)
    assert sample.kernel_times()[1] == 2
    ms, n = sample.kernel_times()
    assert n == 0 and ms.size == 0
    assert sample.kernel_time()[1] == 2  # the sum's own query is not taken from
