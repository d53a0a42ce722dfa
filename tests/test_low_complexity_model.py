"""The low-complexity rule as the Python model states it (low_complexity_model.py): its two forms agree, and the hand
cases of the rule come out as worked out by hand.  No GPU."""
import random

import pytest

from low_complexity_model import low_direct, low_sliding, mask_line, mask_reads, score_direct, codes_of

T = 20


def rnd(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n)).encode()


def seeded_lines(seed=3, n=40):
    """random lines of many lengths over a dirty alphabet, with planted runs of period 1, 2 and 3"""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        ln = rng.choice([5, 31, 32, 33, 63, 64, 65, 66, 100, 150, 257])
        s = bytearray(rnd(rng, ln, "ACGTacgtNUu-"))
        for _ in range(rng.randrange(4)):
            a, per, run = rng.randrange(ln), rng.choice([b"A", b"CA", b"GAT", b"g", b"ct"]), rng.randrange(5, 80)
            for j in range(a, min(ln, a + run)):
                s[j] = per[(j - a) % len(per)]
        out.append(bytes(s))
    return out


@pytest.mark.parametrize("t", [1, 20, 309, 310, 1000])
@pytest.mark.parametrize("u_is_t", [False, True])
def test_the_two_forms_agree_on_seeded_lines(t, u_is_t):
    some = 0
    for line in seeded_lines():
        a, b = low_direct(line, t, u_is_t), low_sliding(line, t, u_is_t)
        assert a == b, line
        some += sum(a)
    assert (some > 0) == (t < 310)  # a window of 62 equal triplets: 10 * 1891 = 310 * 61


def test_threshold_zero_is_off():
    assert not any(low_direct(b"A" * 100, 0)) and not any(low_sliding(b"A" * 100, 0))
    assert mask_line(b"A" * 100, 0) == (b"A" * 100, 0)


def test_hand_cases():
    assert score_direct(codes_of(b"AAAAAA"), 0) == (4, 6)  # 60 > 60 is false
    assert mask_line(b"AAAAAA", T) == (b"AAAAAA", 0)
    assert score_direct(codes_of(b"AAAAAAA"), 3) == (5, 10)
    assert mask_line(b"AAAAAAA", T) == (b"NNNNNNN", 7)
    assert mask_line(b"NNNNAAAAAAANNNN", T) == (b"NNNNNNNNNNNNNNN", 7)
    assert mask_line(b"NNNNAAAAAAANNNN", T, low=low_direct) == (b"NNNNNNNNNNNNNNN", 7)
    # 'U' is a base under the flag alone: without it, it breaks the run into pieces too short to score
    assert mask_line(b"AAAUAAAUAAA", T) == (b"AAAUAAAUAAA", 0)
    assert mask_line(b"UUUUUUU", T, u_is_t=True) == (b"NNNNNNN", 7) and mask_line(b"UUUUUUU", T) == (b"UUUUUUU", 0)
    assert mask_line(b"aaaAAAa", T) == (b"NNNNNNN", 7)  # case-blind


def test_a_run_of_40_takes_its_flanks_and_a_run_of_15_is_left():
    """(seeded: 15 A hold 13 equal triplets, S = 78 of the 122 a full window needs at T = 20, and the flanks add their own
    chance repeats -- in about a third of random 150-mers they tip some position over; this one is of the other kind)"""
    rng = random.Random(7)
    left, right = rnd(rng, 60), rnd(rng, 50)
    masked, n = mask_line(left + b"A" * 40 + right, T)
    assert masked == mask_line(left + b"A" * 40 + right, T, low=low_direct)[0]
    ns = [i for i, c in enumerate(masked) if c == ord("N")]
    assert ns == list(range(ns[0], ns[-1] + 1)) and n == len(ns)  # one stretch
    assert 10 <= 60 - ns[0] <= 22 and 10 <= ns[-1] - 99 <= 22  # the run and about 16 bases on each side
    line = rnd(rng, 70) + b"A" * 15 + rnd(rng, 65)
    assert mask_line(line, T) == (line, 0)


def test_uniform_random_reads_are_left_alone():
    rng = random.Random(2024)
    for _ in range(300):
        line = rnd(rng, 150)
        assert mask_line(line, T) == (line, 0)


def test_one_repeated_base_at_lengths_0_to_70():
    for ln in range(71):
        line = b"A" * ln
        assert low_direct(line, T) == low_sliding(line, T)
        # l = ln - 2 triplets (at most 62 in a window), all equal: 10 l (l - 1) / 2 > 20 (l - 1) <=> l > 4
        assert mask_line(line, T) == ((b"N" * ln, ln) if ln >= 7 else (line, 0)), ln


def test_lines_back_to_back_share_no_window():
    """Two 20-A lines back to back, neither masked, where the 40 A as one line are.  (A line of n equal bases has
    l = n - 2 and S = l (l - 1) / 2, so it is low iff 5 l > T: 20 A alone are low below T = 90, 40 A below T = 190.  At
    T = 100 the two lines stay only if neither sees the other's bases; at T = 20 six bases a line show the same.)"""
    import numpy as np
    bases = np.frombuffer(b"A" * 40, np.uint8)
    for low in (low_direct, low_sliding):
        assert mask_line(bytes(bases), 100, low=low) == (b"N" * 40, 40)
        assert mask_line(bytes(bases[:20]), 100, low=low) == (b"A" * 20, 0)
    assert mask_reads(bases, [0, 40], 100)[1] == 40
    masked, n = mask_reads(bases, [0, 20, 40], 100)
    assert n == 0 and bytes(masked) == bytes(bases)
    masked, n = mask_reads(bases, [0, 6, 12, 18, 24, 30, 36, 40], T)
    assert n == 0 and bytes(masked) == bytes(bases)
    assert mask_reads(bases, [0, 20, 40], T)[1] == 40  # (at T = 20 each is low on its own)
