#!/usr/bin/env python3
"""What the hit pass (kid_db_read_hits_device) costs next to classifying the same reads.

Two workloads, 2 M 150-base reads resident in HBM each:
  metric  bact10-synth at --scale (1.0 = 108.6 M k-mers, 2^30 cells), ~1 % of the windows hit
  dense   reads cut from genomes the database holds (tools/dense_bench.py): every window a hit
For each, alternating in one process after a warm-up: device time of the hits kernels per call (kid_db_read_hits_time:
HIP events around descriptors .. fill) and kid_sample_kernel_time_device of classifying the same batch."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from kmer_id_amd import KmerDB, synth  # noqa: E402

READ_LEN = 150


def measure(name, db, d_bases, n, calls, warmup):
    dev = d_bases.device
    off = torch.arange(n + 1, dtype=torch.int64, device=dev) * READ_LEN
    d_ho = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_nk = torch.empty(n, dtype=torch.int32, device=dev)
    d_tot = torch.zeros(1, dtype=torch.int64, device=dev)
    args = (d_bases.data_ptr(), n * READ_LEN, off.data_ptr(), n, d_ho.data_ptr(), d_tot.data_ptr())
    db.read_hits_device(*args, d_n_kmers=d_nk.data_ptr())  # the sizing call
    torch.cuda.synchronize()
    total = int(d_tot.item())
    d_hits = torch.empty(max(total, 1) * 3, dtype=torch.int32, device=dev)
    s = db.sample()
    for i in range(warmup + calls):
        if i == warmup:
            torch.cuda.synchronize()
            db.read_hits_time()
            s.kernel_time_device()
        db.read_hits_device(*args, d_n_kmers=d_nk.data_ptr(), d_hits=d_hits.data_ptr(), cap=total)
        s.classify_device(d_bases.data_ptr(), n * READ_LEN, off.data_ptr(), n)
    hit_ms, hit_calls, _ = db.read_hits_time()
    cls_ms, cls_calls = s.kernel_time_device()
    st = s.stats()
    s.close()
    windows = int(d_nk.to(torch.int64).sum().item())
    # the two paths saw the same work, or no figure below means anything
    assert windows * (warmup + calls) == st["lookups"] and total * (warmup + calls) == st["hits"]
    print("%-8s %d reads, %d windows, %d hits (%.2f %% of the windows, %.1f per read)" % (
        name, n, windows, total, 100.0 * total / max(windows, 1), total / n))
    print("%-8s hits kernels %.3f ms per call (%d calls) | classify kernel %.3f ms per batch (%d batches) | ratio %.2f" % (
        name, hit_ms / hit_calls, hit_calls, cls_ms / cls_calls, cls_calls, (hit_ms / hit_calls) / (cls_ms / cls_calls)))


def genome_db(parent, k, rng, n_genomes, genome_len):
    """the k-mers of random genomes, each genome under one target -> (genomes uint8[n, len], keys, targets)"""
    G = rng.choice(np.frombuffer(b"ACGT", np.uint8), (n_genomes, genome_len))
    code = np.zeros(256, np.uint64)
    for j, ch in enumerate(b"ACGT"):
        code[ch] = j
    c = code[G]
    nwin = genome_len - k + 1
    key = np.zeros((n_genomes, nwin), np.uint64)
    for j in range(k):
        key = (key << np.uint64(2)) | c[:, j:j + nwin]
    targets = np.repeat(rng.integers(2, parent.size, n_genomes).astype(np.uint32), nwin)
    return G, key.reshape(-1), targets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--log2-slots", type=int, default=30)
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-dense", action="store_true")
    a = ap.parse_args()
    device = torch.device("cuda", 0)
    db, parent, cum, build_s, _, _ = bench.build_db(device, a.scale, a.log2_slots, False)
    d = bench.gen_reads(device, cum, parent, 0, a.reads)
    measure("metric", db, d, a.reads, a.calls, a.warmup)
    db.close()
    del d
    if a.skip_dense:
        return
    rng = np.random.default_rng(3)
    G, keys, targets = genome_db(parent, bench.K, rng, 400, 20000)
    db = KmerDB(keys, targets, parent, k=bench.K, log2_slots=26)
    gi = rng.integers(0, G.shape[0], a.reads)
    pos = rng.integers(0, G.shape[1] - READ_LEN + 1, a.reads)
    bases = G[gi[:, None], pos[:, None] + np.arange(READ_LEN)[None, :]]
    pad = np.zeros(64, np.uint8)
    d = torch.from_numpy(np.concatenate([np.ascontiguousarray(bases).reshape(-1), pad])).cuda()
    measure("dense", db, d, a.reads, a.calls, a.warmup)


if __name__ == "__main__":
    main()
