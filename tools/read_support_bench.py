#!/usr/bin/env python3
"""What the support kernel (kid_db_support_from_hits_device) costs next to the hit pass and to classifying the same reads.

Two workloads, 2 M 150-base reads resident in HBM each (those of tools/read_hits_bench.py):
  metric  bact10-synth at --scale (1.0 = 108.6 M k-mers, 2^30 cells), ~1 % of the windows hit
  dense   reads cut from genomes the database holds: every window a hit (the wave-per-read path of the kernel)
For each, alternating in one process after a warm-up: device time of the support kernel alone per call
(kid_db_read_support_time), of the hits kernels (kid_db_read_hits_time: descriptors .. fill) and
kid_sample_kernel_time_device of classifying the same batch.  The rule is --min-hits / --min-permille (2, 20)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402
from kmer_id_amd import KmerDB  # noqa: E402
from read_hits_bench import READ_LEN, genome_db  # noqa: E402


def measure(name, db, d_bases, n, calls, warmup, rule):
    dev = d_bases.device
    off = torch.arange(n + 1, dtype=torch.int64, device=dev) * READ_LEN
    d_ho = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_nk = torch.empty(n, dtype=torch.int32, device=dev)
    d_tot = torch.zeros(1, dtype=torch.int64, device=dev)
    d_out = torch.zeros(n * 6, dtype=torch.int32, device=dev)
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
            db.read_support_time()
            s.kernel_time_device()
        db.read_hits_device(*args, d_n_kmers=d_nk.data_ptr(), d_hits=d_hits.data_ptr(), cap=total)
        db.support_from_hits_device(d_ho.data_ptr(), d_hits.data_ptr(), d_nk.data_ptr(), n, d_out.data_ptr(), min_hits=rule[0],
                                    min_permille=rule[1])
        s.classify_device(d_bases.data_ptr(), n * READ_LEN, off.data_ptr(), n, d_out=0)
    sup_ms, sup_calls, _ = db.read_support_time()
    hit_ms, hit_calls, _ = db.read_hits_time()
    cls_ms, cls_calls = s.kernel_time_device()
    # the paths saw the same work, or no figure below means anything: the records' `final` is the classify kernel's answer
    d_fin = torch.empty(n, dtype=torch.int32, device=dev)
    s.classify_device(d_bases.data_ptr(), n * READ_LEN, off.data_ptr(), n, d_out=d_fin.data_ptr())
    torch.cuda.synchronize()
    rec = d_out.view(n, 6)
    assert torch.equal(rec[:, 0], d_fin) and int(rec[:, 3].to(torch.int64).sum().item()) == total
    s.close()
    per = rec[:, 3].to(torch.int64)
    called, kept = int((rec[:, 0] > 0).sum().item()), int((rec[:, 1] > 0).sum().item())
    print("%-8s %d reads, %d hits (%.1f per read, %d reads with more than 8), rule (%d, %d): %d reads called, %d confident" % (
        name, n, total, total / n, int((per > 8).sum().item()), rule[0], rule[1], called, kept))
    sup, hit, cls = sup_ms / sup_calls, hit_ms / hit_calls, cls_ms / cls_calls
    print("%-8s support kernel %.3f ms per call (%d calls) | hits kernels %.3f ms | classify kernel %.3f ms | support / hits %.3f | "
          "support / classify %.3f | %.1f GB/s of its own traffic" % (name, sup, sup_calls, hit, cls, sup / hit, sup / cls,
                                                                     (12.0 * total + 32.0 * n) / sup / 1e6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--log2-slots", type=int, default=30)
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--min-hits", type=int, default=2)
    ap.add_argument("--min-permille", type=int, default=20)
    ap.add_argument("--skip-dense", action="store_true")
    a = ap.parse_args()
    rule = (a.min_hits, a.min_permille)
    device = torch.device("cuda", 0)
    db, parent, cum, build_s, _, _ = bench.build_db(device, a.scale, a.log2_slots, False)
    d = bench.gen_reads(device, cum, parent, 0, a.reads)
    measure("metric", db, d, a.reads, a.calls, a.warmup, rule)
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
    measure("dense", db, d, a.reads, a.calls, a.warmup, rule)


if __name__ == "__main__":
    main()
