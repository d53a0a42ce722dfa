"""kid_ucount_kernel on bitmaps that are not almost empty: the bitmap is set through kid_sample_seen_or and ucount compared
with numpy.bincount over the targets of the set bits, on the real taxonomy (LDS histogram) and on a flat one of 20 000
leaves (no histogram: ntar * 4 > 64 KiB).  Exact: integers."""
import numpy as np
import pytest

import short_sample_cases as sc

pytestmark = pytest.mark.gpu


def patterns(nbytes):
    words = nbytes // 4
    z = np.zeros(words, np.uint32)
    one_bit = np.left_shift(np.uint32(1), (np.arange(words, dtype=np.uint32) * 7) % 32).astype(np.uint32)
    alt = z.copy(); alt[::2] = 0xFFFFFFFF
    last = z.copy(); last[-4:] = (0x80000001, 0, 0xFFFFFFFF, 0x00010000)
    return {"all_zero": z, "all_one": np.full(words, 0xFFFFFFFF, np.uint32), "one_bit_per_word": one_bit,
            "alternating_words": alt, "last_partial_group": last}


def flat_world():
    _, keys, _, _, _ = sc.world()
    ntar = 20002
    parent = np.ones(ntar, np.int32)  # 20 000 leaves under the root
    targets = (2 + (np.arange(keys.size, dtype=np.uint64) * 7919) % 20000).astype(np.uint32)  # neighbours differ
    return parent, keys, targets


@pytest.fixture(scope="module", params=["real", "flat"])
def case(request):
    if request.param == "real":
        parent, keys, targets, _, _ = sc.world()
    else:
        parent, keys, targets = flat_world()
    assert (parent.size * 4 > 64 * 1024) == (request.param == "flat")
    db = sc.new_db(parent, keys, targets)
    s = db.sample()
    yield s, parent.size, np.asarray(targets)
    s.close()
    db.close()


@pytest.mark.parametrize("name", ["all_zero", "all_one", "one_bit_per_word", "alternating_words", "last_partial_group"])
def test_ucount_equals_bincount(case, name):
    s, ntar, targets = case
    nbytes = s.seen_bytes()
    assert nbytes * 8 >= targets.size and nbytes % 16 == 0 and targets.size % 128 != 0  # the last group is a partial one
    bitmap = patterns(nbytes)[name]
    s.reset()
    s.seen_or(0, bitmap.view(np.uint8))
    bits = np.flatnonzero(np.unpackbits(bitmap.view(np.uint8), bitorder="little"))
    ord_target = np.zeros(nbytes * 8, np.int64)  # (entries past the last: target 0, as the library pads them)
    ord_target[:targets.size] = targets
    exp = np.bincount(ord_target[bits], minlength=ntar)
    assert np.array_equal(s.ucount_range(0, nbytes * 8), exp)
    half = (nbytes * 4) // 128 * 128
    assert np.array_equal(s.ucount_range(0, half) + s.ucount_range(half, nbytes * 8), exp)
