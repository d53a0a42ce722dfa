"""The entry points of the short-sample work are declared, exported and bound (no GPU)."""
import ctypes as C
import os
import re

import kmer_id_amd
from kmer_id_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("kid_sample_kernel_times",)


def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "kmer_id_amd.h")).read()
    lib = kmer_id_amd.load()
    for name in NEW:
        assert re.search(r"^int %s\(" % name, header, re.M), name + " is not declared"
        assert hasattr(lib, name), name + " is not exported"
        assert name in _lib.PROTOTYPES, "no ctypes prototype for " + name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(_lib.PROTOTYPES[name][1])
    assert callable(api.Sample.kernel_times)


def test_null_handles_are_refused():
    lib = kmer_id_amd.load()
    n = C.c_uint64(7)
    assert lib.kid_sample_kernel_times(None, None, 0, C.byref(n)) == -1  # KID_ERR_ARG
