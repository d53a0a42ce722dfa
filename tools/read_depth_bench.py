#!/usr/bin/env python3
"""What KID_OPT_ENTRY_DEPTH costs: the tally kernel with the depth counters off and on, and the depth spectrum next to
kid_sample_ucount_range on the same sample.

The tally form of the support kernel has host-buffer entry points alone (kid_db_read_support with tally=): each call stages
its batch, runs the hit pass and then the kernel, and kid_db_read_support_time reports the device time of the KERNEL ALONE
(HIP events around it) -- that is the figure compared here, alternating off / on in one process after a warm-up.
Three workloads (those of tools/read_support_bench.py, plus the contention case of the tests):
  metric  bact10-synth at --scale, ~1 % of the windows hit
  dense   reads cut from genomes the database holds: every window a hit (the wave-per-read path of the kernel)
  hot     --hot-reads short reads that all hold one database k-mer: every add lands on one counter
Then, on the metric sample: wall time of kid_sample_depth_spectrum (256 bins: it streams 4 B per entry, launches three
kernels, allocates and copies ntar * 256 * 8 B back) and of kid_sample_ucount_range (1 bit per entry), both synchronous."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402
from kmer_id_amd import KID_OPT_ENTRY_DEPTH, KmerDB  # noqa: E402
from read_hits_bench import READ_LEN, genome_db  # noqa: E402


def tally_times(name, db, bases, off, calls, warmup, rule):
    """-> the two samples (off, on) after the same calls"""
    plain, deep = db.sample(), db.sample()
    deep.set_option(KID_OPT_ENTRY_DEPTH, 1)
    ms = {0: 0.0, 1: 0.0}
    for i in range(warmup + calls):
        for which, s in ((0, plain), (1, deep)):
            db.read_support_time()
            rec = db.read_support(bases, off, min_hits=rule[0], min_permille=rule[1], tally=s)
            t, n_calls, _ = db.read_support_time()
            assert n_calls == 1
            if i >= warmup:
                ms[which] += t
    n = off.size - 1
    hits = int(rec["n_hits"].astype(np.int64).sum())
    counted = int(rec["n_hits"][rec["confident"] > 0].astype(np.int64).sum())
    depth_sum = int(deep.depth_spectrum(2)[1].sum())
    # the two samples saw the same work, and the counters hold what the kernel was asked to add (hits of target 1 apart)
    assert np.array_equal(plain.gcount(), deep.gcount()) and 0 < depth_sum <= counted * (warmup + calls)
    a, b = ms[0] / calls, ms[1] / calls
    print("%-7s %d reads, %d hits (%.2f per read), %d of them in reads the rule (%d, %d) calls; depth sum %d after %d calls" % (
        name, n, hits, hits / n, counted, rule[0], rule[1], depth_sum, warmup + calls))
    print("%-7s tally kernel: depth off %.4f ms per call | depth on %.4f ms | on / off %.3f (%d calls each, alternating)" % (
        name, a, b, b / a, calls))
    return plain, deep


def wall(f, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return min(ts), float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--log2-slots", type=int, default=30)
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--hot-reads", type=int, default=5000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--min-hits", type=int, default=2)
    ap.add_argument("--min-permille", type=int, default=20)
    a = ap.parse_args()
    rule = (a.min_hits, a.min_permille)
    device = torch.device("cuda", 0)
    db, parent, cum, build_s, _, _ = bench.build_db(device, a.scale, a.log2_slots, False)
    d = bench.gen_reads(device, cum, parent, 0, a.reads)
    bases = d.cpu().numpy()[:a.reads * READ_LEN].copy()
    del d
    off = (np.arange(a.reads + 1, dtype=np.uint64) * np.uint64(READ_LEN))
    plain, deep = tally_times("metric", db, bases, off, a.calls, a.warmup, rule)
    n_entries, ntar = db.info.n_entries, db.info.ntar
    seen_bits = deep.seen_bytes() * 8
    sp = wall(lambda: deep.depth_spectrum(256), 7)
    uc = wall(lambda: deep.ucount_range(0, seen_bits), 7)
    spec, ksum, dmax = deep.depth_spectrum(256)
    assert np.array_equal(spec[:, 1:].sum(axis=1).astype(np.int64), deep.ucount_range(0, seen_bits))
    print("spectrum %d entries, %d targets, %d entries with a hit: kid_sample_depth_spectrum(256) %.3f ms min / %.3f median, %.1f MB read "
          "(%.1f GB/s at the min) | kid_sample_ucount_range %.3f ms min / %.3f median, %.1f MB read (%.1f GB/s)" % (
              n_entries, ntar, int(spec[:, 1:].sum()), sp[0], sp[1], n_entries * 4 / 1e6, n_entries * 4 / sp[0] / 1e6, uc[0], uc[1],
              n_entries / 8 / 1e6, n_entries / 8 / uc[0] / 1e6))
    plain.close(), deep.close()

    # hot: one database k-mer of the metric database (the first hit of the metric reads with a target > 1) in every read
    h = db.read_hits(bases[:4000 * READ_LEN], off[:4001])
    j = int(np.flatnonzero(h.target > 1)[0])
    r = int(np.searchsorted(h.offsets, j, side="right")) - 1
    kmer = bases[r * READ_LEN + int(h.pos[j]):r * READ_LEN + int(h.pos[j]) + bench.K]
    rng = np.random.default_rng(5)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    hot = np.concatenate([np.concatenate([rng.choice(acgt, 5), kmer, rng.choice(acgt, 5)]) for _ in range(a.hot_reads)])
    hoff = np.arange(a.hot_reads + 1, dtype=np.uint64) * np.uint64(bench.K + 10)
    p, q = tally_times("hot", db, hot, hoff, a.calls, a.warmup, (0, 0))
    assert int(q.depth_spectrum(2)[2].max()) == a.hot_reads * (a.calls + a.warmup)
    p.close(), q.close(), db.close()

    rng = np.random.default_rng(3)
    G, keys, targets = genome_db(parent, bench.K, rng, 400, 20000)
    db = KmerDB(keys, targets, parent, k=bench.K, log2_slots=26)
    gi = rng.integers(0, G.shape[0], a.reads)
    pos = rng.integers(0, G.shape[1] - READ_LEN + 1, a.reads)
    dense = np.ascontiguousarray(G[gi[:, None], pos[:, None] + np.arange(READ_LEN)[None, :]]).reshape(-1)
    p, q = tally_times("dense", db, dense, off, a.calls, a.warmup, rule)
    p.close(), q.close(), db.close()


if __name__ == "__main__":
    main()
