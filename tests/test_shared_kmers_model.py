"""The shared-k-mers rule on a case small enough to count by hand, and the seen file: write / read round trip, bad magic,
truncation.  No GPU."""
import struct

import numpy as np
import pytest

import shared_kmers_model as sm
from kmer_id_amd import read_seen_file, write_seen_file

# 40 entries, 3 targets: entries 0..9 -> 2, 10..24 -> 1, 25..39 -> 2, except entry 30 -> 0
T = np.array([2] * 10 + [1] * 15 + [2] * 15, np.uint32)
T[30] = 0
A = [0, 1, 2, 10, 11, 30, 39]          # 2: {0, 1, 2, 39}   1: {10, 11}   0: {30}
B = [1, 2, 3, 11, 12, 13, 30, 38, 39]  # 2: {1, 2, 3, 38, 39}   1: {11, 12, 13}   0: {30}
C = [5, 24, 25]                        # 2: {5, 25}   1: {24}


def bitmap(entries, pad_ones=False):
    bits = np.zeros(40, bool)
    bits[entries] = True
    return sm.pack(bits, pad_ones=pad_ones)


def test_layout_of_a_bitmap():
    b = bitmap(A)
    assert b.size == 16 == sm.seen_bytes(40) and sm.seen_bytes(0) == 16 and sm.seen_bytes(128) == 16 and sm.seen_bytes(129) == 32
    words = b.view("<u4")
    assert words[0] == (1 << 0 | 1 << 1 | 1 << 2 | 1 << 10 | 1 << 11 | 1 << 30) and words[1] == 1 << (39 - 32) and not words[2:].any()


def test_the_rule_on_a_hand_written_case():
    expected = np.array([[[1, 2, 4], [1, 1, 3], [0, 0, 0]],
                         [[1, 1, 3], [1, 3, 5], [0, 0, 0]],
                         [[0, 0, 0], [0, 0, 0], [0, 1, 2]]], np.int64)
    got = sm.shared(T, 3, [bitmap(A), bitmap(B), bitmap(C)])
    assert got.dtype == np.int64 and np.array_equal(got, expected)
    # the padding bits (entries 40 .. 127) are ignored whatever they hold; a bitmap may be named twice
    padded = sm.shared(T, 3, [bitmap(A, True), bitmap(B, True), bitmap(C), bitmap(A)])
    assert np.array_equal(padded[:3, :3], expected) and np.array_equal(padded[3], padded[0]) and np.array_equal(padded[0, 3], expected[0, 0])
    assert np.array_equal(padded, padded.transpose(1, 0, 2))


def test_the_lines_of_kmer_shared():
    m = sm.shared(T, 3, [bitmap(A), bitmap(B), bitmap(C)])
    assert sm.cli_lines(["a", "b", "c"], m) == (b"#0\ta\t7\n#1\tb\t9\n#2\tc\t3\n0,1,0,1,1,1\n0,1,1,2,3,1\n0,1,2,4,5,3\n"
                                                  b"0,2,1,2,1,0\n0,2,2,4,2,0\n1,2,1,3,1,0\n1,2,2,5,2,0\n")
    assert sm.cli_lines(["a", "b", "c"], m, 2) == b"#0\ta\t7\n#1\tb\t9\n#2\tc\t3\n0,1,2,4,5,3\n"


def test_seen_file_round_trip(tmp_path):
    path = str(tmp_path / "x_seen.bin")
    b = bitmap(B, pad_ones=True)
    write_seen_file(path, b, 40, 3, 30)
    raw = open(path, "rb").read()
    assert len(raw) == 32 + 16 and raw[:8] == b"KIDSEEN1" and struct.unpack("<QiiQ", raw[8:32]) == (40, 3, 30, 16) and raw[32:] == b.tobytes()
    got, n_entries, ntar, k = read_seen_file(path)
    assert got.dtype == np.uint8 and np.array_equal(got, b) and (n_entries, ntar, k) == (40, 3, 30)


@pytest.mark.parametrize("damage", ["magic", "short-header", "short-bitmap", "long", "size"])
def test_seen_file_that_is_not_one(tmp_path, damage):
    path = str(tmp_path / "x_seen.bin")
    write_seen_file(path, bitmap(A), 40, 3, 30)
    raw = open(path, "rb").read()
    bad = {"magic": b"KIDSEEN2" + raw[8:], "short-header": raw[:20], "short-bitmap": raw[:-1], "long": raw + b"\0",
           "size": raw[:8] + struct.pack("<QiiQ", 400, 3, 30, 16) + raw[32:]}[damage]
    open(path, "wb").write(bad)
    with pytest.raises(ValueError):
        read_seen_file(path)
