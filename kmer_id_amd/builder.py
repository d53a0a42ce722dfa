"""ctypes wrapper of the probe-database builder (kid_builder_* of include/kmer_id_amd.h): the GPU table of
kmer_build_vf6 and its three phases.  Text is ACGTN bytes (anything but A, C, G, T breaks a k-mer)."""
import ctypes as C

import numpy as np

from ._lib import check, load

CAND_DTYPE = np.dtype([("key", "<u8"), ("gpos", "<i8"), ("target", "<i4"), ("count", "<u2"), ("strand_r", "u1"), ("flags", "u1")])


def device_mem_info(device=0):
    """(free, total) bytes of the device's memory"""
    lib = load()
    f, t = C.c_uint64(0), C.c_uint64(0)
    check(lib.kid_device_mem_info(device, C.byref(f), C.byref(t)))
    return f.value, t.value


def _text(seq):
    if isinstance(seq, str):
        seq = seq.encode("ascii")
    a = np.frombuffer(seq, np.uint8) if isinstance(seq, (bytes, bytearray)) else np.ascontiguousarray(seq, np.uint8)
    return a, a.ctypes.data_as(C.c_void_p), a.size


class ProbeBuilder:
    """2^log2_cells uint32 cells on `device`; parent[ntar] is the taxonomy after the tree file's edges."""

    def __init__(self, parent, log2_cells=35, device=0, batch_bases=0):
        self._lib = load()
        self.parent = np.ascontiguousarray(parent, np.int32)
        self.log2_cells = log2_cells
        h = C.c_void_p()
        check(self._lib.kid_builder_create(device, log2_cells, self.parent.ctypes.data_as(C.c_void_p), self.parent.size,
                                           batch_bases, C.byref(h)))
        self._h = h

    def close(self):
        if self._h:
            self._lib.kid_builder_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def add(self, seq, target):
        """phase 1: every 30-mer of an ingroup genome of `target`"""
        a, p, n = _text(seq)
        check(self._lib.kid_builder_add(self._h, p, n, int(target)))

    def remove(self, seq):
        """phase 2: every 30-mer of an outgroup genome spoils its cell"""
        a, p, n = _text(seq)
        check(self._lib.kid_builder_remove(self._h, p, n))

    def set_minct(self, minct):
        m = np.ascontiguousarray(minct, np.int32)
        check(self._lib.kid_builder_set_minct(self._h, m.ctypes.data_as(C.c_void_p), m.size))

    def claim(self, seq, gpos_base=0):
        """phase 3 for one sequence: the candidates (first occurrences of live cells with count >= minct), gpos order"""
        a, p, n = _text(seq)
        out = np.zeros(max(n - 29, 1), CAND_DTYPE)
        nc = C.c_uint64(0)
        check(self._lib.kid_builder_claim(self._h, p, n, int(gpos_base), out.ctypes.data_as(C.c_void_p), out.size, C.byref(nc)))
        return out[:nc.value]

    def size(self):
        v = C.c_uint64(0)
        check(self._lib.kid_builder_size(self._h, C.byref(v)))
        return v.value

    def export(self, first=0, n=None):
        if n is None:
            n = (1 << self.log2_cells) - first
        out = np.zeros(n, np.uint32)
        check(self._lib.kid_builder_export(self._h, first, n, out.ctypes.data_as(C.c_void_p)))
        return out

    def entropy(self, keys):
        """the device's check_entropy flags: bit 0 passes, bit 1 "bad" """
        k = np.ascontiguousarray(keys, np.uint64)
        out = np.zeros(k.size, np.uint8)
        check(self._lib.kid_builder_entropy(self._h, k.ctypes.data_as(C.c_void_p), k.size, out.ctypes.data_as(C.c_void_p)))
        return out

    def stats(self):
        """({add, remove, claim} device ms, bases handed over)"""
        ms = (C.c_double * 3)()
        nb = (C.c_uint64 * 3)()
        check(self._lib.kid_builder_stats(self._h, ms, nb))
        return list(ms), list(nb)
