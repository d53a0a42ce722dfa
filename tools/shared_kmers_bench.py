#!/usr/bin/env python3
"""What kid_db_shared_kmers costs: the device time of its kernels for n = 2, 8 and 64 bitmaps resident in HBM, beside the
time the same device needs to stream the bytes the kernel reads, n * B + 4 * n_entries (B: bytes of a bitmap), once.

The database is bact10-synth at --scale; bitmap 0 is the seen-bitmap of a sample that classified --reads reads of the
metric workload, the others are random at its bit density (a bit per entry with that probability, seeded), all made on the
device.  The device time comes from kid_shared_kmers_time (HIP events around the pair kernel and the mirror kernel inside
the call; clearing the matrix and copying it to the host are not in it).  The streaming time is a plain device-to-device
copy of n * B + 4 * n_entries bytes in the same process, between two HIP events (torch.cuda.Event): it reads and writes
that many bytes.  Every figure is the median of --runs calls after --warmup.  The wall time of the whole call is printed
too: at 64 bitmaps it is mostly the matrix (n * n * ntar * 8 bytes cleared on the device and copied into pageable memory)."""
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
from kmer_id_amd import _lib  # noqa: E402
from kmer_id_amd.api import shared_kmers_time  # noqa: E402
from read_hits_bench import READ_LEN  # noqa: E402


def random_bitmap(device, n_words, n_entries, density, seed):
    """int32[n_words] on the device: bit o set with probability `density` for o < n_entries"""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    out = torch.zeros(n_words, dtype=torch.int32, device=device)
    weights = (torch.ones(32, dtype=torch.int64, device=device) << torch.arange(32, device=device)).to(torch.int64)
    chunk = 1 << 20  # words
    for w0 in range(0, n_words, chunk):
        w1 = min(w0 + chunk, n_words)
        bits = (torch.rand((w1 - w0, 32), generator=g, device=device) < density).to(torch.int64)
        entry = (torch.arange(w0, w1, device=device)[:, None] * 32 + torch.arange(32, device=device)[None, :])
        words = ((bits * (entry < n_entries)) * weights[None, :]).sum(dim=1)
        out[w0:w1] = (words & 0xFFFFFFFF).to(torch.int32)  # (wraps into the sign bit)
    return out


def copy_ms(device, nbytes, runs, warmup):
    src = torch.empty(nbytes, dtype=torch.uint8, device=device).fill_(1)
    dst = torch.empty_like(src)
    ts = []
    for i in range(warmup + runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--log2-slots", type=int, default=30)
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--n", type=int, nargs="+", default=[2, 8, 64])
    a = ap.parse_args()
    device = torch.device("cuda", 0)
    lib = _lib.load()
    db, parent, cum, build_s, _, _ = bench.build_db(device, a.scale, a.log2_slots, False)
    d = bench.gen_reads(device, cum, parent, 0, a.reads)
    bases = d.cpu().numpy()[:a.reads * READ_LEN].copy()
    del d
    off = np.arange(a.reads + 1, dtype=np.uint64) * np.uint64(READ_LEN)
    s = db.sample()
    s.classify(bases, off, want_final=False)
    g, u = s.end()
    n_entries, ntar, nbytes = db.info.n_entries, db.info.ntar, s.seen_bytes()
    n_words = nbytes // 4
    density = int(u.sum()) / n_entries
    maps = [torch.zeros(n_words, dtype=torch.int32, device=device)]
    s.seen_export(0, nbytes, dst_ptr=maps[0].data_ptr(), on_device=True)
    for i in range(1, max(a.n)):
        maps.append(random_bitmap(device, n_words, n_entries, density, 1000 + i))
    torch.cuda.synchronize()
    print("database: %d entries, %d targets, a bitmap of %d bytes; the metric sample (%d reads) has %d bits = %.4f of the entries; "
          "the other bitmaps are random at that density" % (n_entries, ntar, nbytes, a.reads, int(u.sum()), density))
    for n in a.n:
        ptrs = (C.c_void_p * n)(*[m.data_ptr() for m in maps[:n]])
        out = np.empty((n, n, ntar), np.int64)
        dev, wall = [], []
        for i in range(a.warmup + a.runs):
            shared_kmers_time()
            t0 = time.perf_counter()
            _lib.check(lib.kid_db_shared_kmers(db._h, ptrs, n, 1, out.ctypes.data_as(C.c_void_p)))
            w = (time.perf_counter() - t0) * 1e3
            ms, calls = shared_kmers_time()
            assert calls == 1
            if i >= a.warmup:
                dev.append(ms)
                wall.append(w)
        assert np.array_equal(out[0, 0], u) and np.array_equal(out, out.transpose(1, 0, 2))  # the sample's diagonal is its ucount
        stream_bytes = n * nbytes + 4 * n_entries
        c = copy_ms(device, stream_bytes, a.runs, a.warmup)
        k = float(np.median(dev))
        print("n = %2d: kernels %.3f ms (median of %d runs; min %.3f, max %.3f) | device-to-device copy of n * B + 4 * n_entries = %.1f MB: "
              "%.3f ms (median of %d) | kernels / copy %.2f | %.1f GB/s of the bytes read | whole call %.1f ms wall (median), matrix %.1f MB" % (
                  n, k, a.runs, min(dev), max(dev), stream_bytes / 1e6, c, a.runs, k / c, stream_bytes / k / 1e6, float(np.median(wall)),
                  out.nbytes / 1e6))
    s.close(), db.close()


if __name__ == "__main__":
    main()
