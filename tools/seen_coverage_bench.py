#!/usr/bin/env python3
"""What kid_seen_coverage costs: the device time of its count pass (the kernel that runs once per bitmap) and of all the
kernels of a call, for entries in (org, position) order and for the same entries shuffled, beside the time the same
device needs to stream the bytes each of them reads.

The database is bact10-synth at --scale (0.25: 27.1 M entries).  The sites are synthetic: org = o // 20000, positions
ascending within an organism with a seeded step of 1 .. 99 bases (about 1 M bases and, at the default width of 1000,
1000 bins of 20 entries per organism).  Bitmap 0 is the seen-bitmap of a sample that classified --reads reads of the
metric workload, the others are random at its bit density (seeded).  Everything is handed to the call in host memory, as
the C ABI asks; the device times come from HIP events inside the call (kid_seen_coverage_time for all kernels,
kid_bench_coverage_count_time for the count kernels over the bitmaps) and hold no copy.  The yardsticks are plain
device-to-device copies, in the same process between two HIP events, of
    count pass:  n * (B + 8 * n_entries) bytes        (B: bytes of a bitmap; org and pos are read once per bitmap)
    whole call:  (n + 2) * 8 * n_entries + n * B + (12 * n + 4) * bins bytes
                 (the span stage and the probes-per-bin pass read org and pos once each; per bitmap the counters are
                  cleared, and the reduce kernel reads them and the probes per bin)
Every figure is the median of --runs calls after --warmup.  The records of the shuffled call must be the bytes of the
ordered one."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402
from kmer_id_amd import COVERAGE_DTYPE, _lib  # noqa: E402
from kmer_id_amd.api import seen_coverage_time  # noqa: E402
from read_hits_bench import READ_LEN  # noqa: E402
from shared_kmers_bench import copy_ms  # noqa: E402

PER_ORG = 20000


def sites(n_entries, seed):
    rng = np.random.default_rng(seed)
    o = np.arange(n_entries, dtype=np.int64)
    org = (o // PER_ORG).astype(np.uint32)
    at = np.cumsum(rng.integers(1, 100, n_entries, dtype=np.int64))
    pos = (at - at[o // PER_ORG * PER_ORG]).astype(np.uint32)  # from 0 in every organism
    return org, pos


def pack(bits, nbytes):
    out = np.zeros(nbytes, np.uint8)
    packed = np.packbits(bits, bitorder="little")
    out[:packed.size] = packed
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=0.25)
    ap.add_argument("--log2-slots", type=int, default=28)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--bin-width", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--n", type=int, nargs="+", default=[1, 8])
    a = ap.parse_args()
    device = torch.device("cuda", 0)
    lib = _lib.load()
    db, parent, cum, build_s, _, _ = bench.build_db(device, a.scale, a.log2_slots, False)
    d = bench.gen_reads(device, cum, parent, 0, a.reads)
    bases = d.cpu().numpy()[:a.reads * READ_LEN].copy()
    del d
    s = db.sample()
    s.classify(bases, np.arange(a.reads + 1, dtype=np.uint64) * np.uint64(READ_LEN), want_final=False)
    g, u = s.end()
    n_entries, nbytes = db.info.n_entries, s.seen_bytes()
    first = s.seen_export(0, nbytes)
    s.close(), db.close()
    density = int(u.sum()) / n_entries
    rng = np.random.default_rng(1000)
    bits = [np.unpackbits(first, bitorder="little")[:n_entries].astype(bool)]
    for i in range(1, max(a.n)):
        bits.append(rng.random(n_entries, dtype=np.float32) < density)
    org, pos = sites(n_entries, 7)
    n_orgs = int(org[-1]) + 1
    perm = np.random.default_rng(11).permutation(n_entries)
    orders = {"in (org, pos) order": (org, pos, [pack(b, nbytes) for b in bits]),
              "shuffled": (org[perm], pos[perm], [pack(b[perm], nbytes) for b in bits])}
    print("database: %d entries in %d organisms, a bitmap of %d bytes; the metric sample (%d reads) has %d bits = %.4f of the entries; "
          "the other bitmaps are random at that density; bin width %d" % (n_entries, n_orgs, nbytes, a.reads, int(u.sum()), density, a.bin_width))
    for n in a.n:
        records, figures = {}, {}
        for name, (o_, p_, maps) in orders.items():
            ptrs = (C.c_void_p * n)(*[m.ctypes.data for m in maps[:n]])
            out = np.zeros((n, n_orgs), COVERAGE_DTYPE)
            count, whole, wall = [], [], []
            for i in range(a.warmup + a.runs):
                seen_coverage_time()
                lib.kid_bench_coverage_count_time(None)
                t0 = time.perf_counter()
                _lib.check(lib.kid_seen_coverage(0, o_.ctypes.data_as(C.c_void_p), p_.ctypes.data_as(C.c_void_p), n_entries, n_orgs, a.bin_width,
                                                 ptrs, n, out.ctypes.data_as(C.c_void_p)))
                w = (time.perf_counter() - t0) * 1e3
                ms, calls = seen_coverage_time()
                c = C.c_double(0)
                lib.kid_bench_coverage_count_time(C.byref(c))
                assert calls == 1
                if i >= a.warmup:
                    count.append(c.value)
                    whole.append(ms)
                    wall.append(w)
            records[name] = out.tobytes()
            figures[name] = (float(np.median(count)), float(np.median(whole)))
            n_bins = int(out["span_bins"][0].astype(np.int64).sum())
            assert int(out["n_seen"][0].astype(np.int64).sum()) == int(u.sum()) and int(out["n_probes"][0].astype(np.int64).sum()) == n_entries
            count_bytes = n * (nbytes + 8 * n_entries)
            whole_bytes = (n + 2) * 8 * n_entries + n * nbytes + (12 * n + 4) * n_bins
            cc, cw = copy_ms(device, count_bytes, a.runs, a.warmup), copy_ms(device, whole_bytes, a.runs, a.warmup)
            kc, kw = figures[name]
            print("n = %2d, %s, %d bins: count pass %.3f ms (median of %d; min %.3f, max %.3f) | copy of %.1f MB: %.3f ms | count / copy %.2f || "
                  "all kernels %.3f ms (min %.3f, max %.3f) | copy of %.1f MB: %.3f ms | kernels / copy %.2f || whole call %.1f ms wall" % (
                      n, name, n_bins, kc, a.runs, min(count), max(count), count_bytes / 1e6, cc, kc / cc, kw, min(whole), max(whole),
                      whole_bytes / 1e6, cw, kw / cw, float(np.median(wall))))
        assert records["shuffled"] == records["in (org, pos) order"], "the order of the entries changed the records"
        print("n = %2d: shuffled / ordered: count pass %.2f, all kernels %.2f; the records are the same bytes" % (
            n, figures["shuffled"][0] / figures["in (org, pos) order"][0], figures["shuffled"][1] / figures["in (org, pos) order"][1]))


if __name__ == "__main__":
    main()
