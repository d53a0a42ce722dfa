#!/usr/bin/env python3
"""What the vote kernels (kid_db_votes_from_hits_device) cost next to the support kernel on the same hit CSR.

Three workloads resident in HBM (the first two those of tools/read_support_bench.py):
  metric  2 M 150-base reads of bact10-synth at --scale (1.0 = 108.6 M k-mers, 2^30 cells), ~1 % of the windows hit:
          the lane-per-read regime of both kernels
  dense   2 M 150-base reads cut from genomes the database holds: every window a hit, 121 per read -- the wave-per-read
          regime, where the vote kernel tests hits pairwise
  long    --long-reads reads of --long-len bases cut from the same genomes: more than KID_VOTE_WAVE_HITS hits per read,
          all of them left to kid_vote_big_kernel
For each, alternating in one process after a warm-up: device time per call of the vote kernels alone
(kid_db_read_votes_time: both kernels and the list's reset between the two events) and of the support kernel alone
(kid_db_read_support_time).  The vote kernels do strictly more work per hit; the ratio is reported, not judged.
The rule is --min-hits / --min-permille (2, 20)."""
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


def measure(name, db, d_bases, n, read_len, calls, warmup, rule):
    dev = d_bases.device
    off = torch.arange(n + 1, dtype=torch.int64, device=dev) * read_len
    d_ho = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_nk = torch.empty(n, dtype=torch.int32, device=dev)
    d_tot = torch.zeros(1, dtype=torch.int64, device=dev)
    d_sup = torch.zeros(n * 6, dtype=torch.int32, device=dev)
    d_vote = torch.zeros(n * 8, dtype=torch.int32, device=dev)
    args = (d_bases.data_ptr(), n * read_len, off.data_ptr(), n, d_ho.data_ptr(), d_tot.data_ptr())
    db.read_hits_device(*args, d_n_kmers=d_nk.data_ptr())  # the sizing call
    torch.cuda.synchronize()
    total = int(d_tot.item())
    d_hits = torch.empty(max(total, 1) * 3, dtype=torch.int32, device=dev)
    db.read_hits_device(*args, d_n_kmers=d_nk.data_ptr(), d_hits=d_hits.data_ptr(), cap=total)
    for i in range(warmup + calls):
        if i == warmup:
            torch.cuda.synchronize()
            db.read_support_time()
            db.read_votes_time()
        db.support_from_hits_device(d_ho.data_ptr(), d_hits.data_ptr(), d_nk.data_ptr(), n, d_sup.data_ptr(), min_hits=rule[0],
                                    min_permille=rule[1])
        db.votes_from_hits_device(d_ho.data_ptr(), d_hits.data_ptr(), d_nk.data_ptr(), n, d_vote.data_ptr(), min_hits=rule[0],
                                  min_permille=rule[1])
    sup_ms, sup_calls, _ = db.read_support_time()
    vote_ms, vote_calls, _ = db.read_votes_time()
    torch.cuda.synchronize()
    sup, vote = d_sup.view(n, 6), d_vote.view(n, 8)
    # the two saw the same hits, or no figure below means anything
    assert torch.equal(sup[:, 3], vote[:, 3]) and int(vote[:, 3].to(torch.int64).sum().item()) == total
    per = vote[:, 3].to(torch.int64)
    print("%-7s %d reads of %d bases, %d hits (%.1f per read; %d reads above 8 hits, %d above 512), rule (%d, %d): call != final for %d "
          "reads, %d ties, %d confident by votes, %d by support" % (
              name, n, read_len, total, total / n, int((per > 8).sum().item()), int((per > 512).sum().item()), rule[0], rule[1],
              int((sup[:, 0] != vote[:, 0]).sum().item()), int((vote[:, 5] > 1).sum().item()), int((vote[:, 1] > 0).sum().item()),
              int((sup[:, 1] > 0).sum().item())))
    s, v = sup_ms / sup_calls, vote_ms / vote_calls
    print("%-7s vote kernels %.3f ms per call (%d calls) | support kernel %.3f ms | votes / support %.2f | %.3f ns per hit" % (
        name, v, vote_calls, s, v / s, v * 1e6 / max(total, 1)))


def cut_reads(G, rng, n, read_len):
    gi = rng.integers(0, G.shape[0], n)
    pos = rng.integers(0, G.shape[1] - read_len + 1, n)
    bases = G[gi[:, None], pos[:, None] + np.arange(read_len)[None, :]]
    return torch.from_numpy(np.concatenate([np.ascontiguousarray(bases).reshape(-1), np.zeros(64, np.uint8)])).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--log2-slots", type=int, default=30)
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--long-reads", type=int, default=20_000)
    ap.add_argument("--long-len", type=int, default=1200)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--min-hits", type=int, default=2)
    ap.add_argument("--min-permille", type=int, default=20)
    ap.add_argument("--skip-metric", action="store_true")
    a = ap.parse_args()
    rule = (a.min_hits, a.min_permille)
    device = torch.device("cuda", 0)
    db, parent, cum, build_s, _, _ = bench.build_db(device, a.scale, a.log2_slots, False)
    if not a.skip_metric:
        d = bench.gen_reads(device, cum, parent, 0, a.reads)
        measure("metric", db, d, a.reads, READ_LEN, a.calls, a.warmup, rule)
        del d
    db.close()
    rng = np.random.default_rng(3)
    G, keys, targets = genome_db(parent, bench.K, rng, 400, 20000)
    db = KmerDB(keys, targets, parent, k=bench.K, log2_slots=26)
    measure("dense", db, cut_reads(G, rng, a.reads, READ_LEN), a.reads, READ_LEN, a.calls, a.warmup, rule)
    measure("long", db, cut_reads(G, rng, a.long_reads, a.long_len), a.long_reads, a.long_len, a.calls, a.warmup, rule)


if __name__ == "__main__":
    main()
