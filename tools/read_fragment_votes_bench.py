#!/usr/bin/env python3
"""What the fragment-vote kernels (kid_db_fragment_votes_from_hits_device) cost next to the vote kernels and the fragment
kernel on the same hit CSR.

Three workloads resident in HBM (those of tools/read_votes_bench.py; reads 2i and 2i + 1 are the mates of fragment i):
  metric  2 M 150-base reads of bact10-synth at --scale (1.0 = 108.6 M k-mers, 2^30 cells), ~1 % of the windows hit:
          the lane-per-fragment regime
  dense   2 M 150-base reads cut from genomes the database holds: every window a hit, 121 per mate and 242 per fragment
          -- the wave-per-fragment regime, where one pairwise pass over the 242 hits feeds the three best sets
  long    --long-reads reads of --long-len bases cut from the same genomes: more than KID_VOTE_WAVE_HITS hits per
          fragment, all of them left to kid_fragment_vote_big_kernel (three rounds over the workgroup's row)
For each, alternating in one process after a warm-up: device time per call of the fragment-vote kernels alone
(kid_db_read_fragment_votes_time), of the vote kernels alone (kid_db_read_votes_time: twice as many records, half the
hits each) and of the fragment kernel alone (kid_db_read_fragments_time).  The pairwise pass of a fragment costs
(p + q)^2 tests where the two reads cost p^2 + q^2; the ratios are reported, not judged.
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
from read_votes_bench import cut_reads  # noqa: E402


def measure(name, db, d_bases, n, read_len, calls, warmup, rule):
    assert n % 2 == 0
    dev = d_bases.device
    off = torch.arange(n + 1, dtype=torch.int64, device=dev) * read_len
    d_ho = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_nk = torch.empty(n, dtype=torch.int32, device=dev)
    d_tot = torch.zeros(1, dtype=torch.int64, device=dev)
    d_vote = torch.zeros(n * 8, dtype=torch.int32, device=dev)
    d_frag = torch.zeros(n // 2 * 8, dtype=torch.int32, device=dev)
    d_fv = torch.zeros(n // 2 * 10, dtype=torch.int32, device=dev)
    args = (d_bases.data_ptr(), n * read_len, off.data_ptr(), n, d_ho.data_ptr(), d_tot.data_ptr())
    db.read_hits_device(*args, d_n_kmers=d_nk.data_ptr())  # the sizing call
    torch.cuda.synchronize()
    total = int(d_tot.item())
    d_hits = torch.empty(max(total, 1) * 3, dtype=torch.int32, device=dev)
    db.read_hits_device(*args, d_n_kmers=d_nk.data_ptr(), d_hits=d_hits.data_ptr(), cap=total)
    csr = (d_ho.data_ptr(), d_hits.data_ptr(), d_nk.data_ptr(), n)
    for i in range(warmup + calls):
        if i == warmup:
            torch.cuda.synchronize()
            db.read_votes_time()
            db.read_fragments_time()
            db.read_fragment_votes_time()
        db.votes_from_hits_device(*csr, d_vote.data_ptr(), min_hits=rule[0], min_permille=rule[1])
        db.fragments_from_hits_device(*csr, d_frag.data_ptr(), min_hits=rule[0], min_permille=rule[1])
        db.fragment_votes_from_hits_device(*csr, d_fv.data_ptr(), min_hits=rule[0], min_permille=rule[1])
    vote_ms, vote_calls, _ = db.read_votes_time()
    frag_ms, frag_calls, _ = db.read_fragments_time()
    fv_ms, fv_calls, _ = db.read_fragment_votes_time()
    torch.cuda.synchronize()
    vote, frag, fv = d_vote.view(n, 8), d_frag.view(n // 2, 8), d_fv.view(n // 2, 10)
    # the three saw the same hits and agree where they must, or no figure below means anything
    per = fv[:, 3].to(torch.int64)
    assert torch.equal(frag[:, 3], fv[:, 3]) and torch.equal(frag[:, 2], fv[:, 2]) and int(per.sum().item()) == total
    assert torch.equal(fv[:, 8], vote[0::2, 0]) and torch.equal(fv[:, 9], vote[1::2, 0])
    print("%-7s %d fragments of 2 x %d bases, %d hits (%.1f per fragment; %d fragments above 8 hits, %d above 512), rule (%d, %d): "
          "call != final for %d fragments, %d ties, %d confident by votes, %d by the fold; call != call_1 or call_2 where both mates hit: %d" % (
              name, n // 2, read_len, total, 2 * total / n, int((per > 8).sum().item()), int((per > 512).sum().item()), rule[0], rule[1],
              int((frag[:, 0] != fv[:, 0]).sum().item()), int((fv[:, 5] > 1).sum().item()), int((fv[:, 1] > 0).sum().item()),
              int((frag[:, 1] > 0).sum().item()),
              int(((fv[:, 8] > 0) & (fv[:, 9] > 0) & ((fv[:, 0] != fv[:, 8]) | (fv[:, 0] != fv[:, 9]))).sum().item())))
    v, f, x = vote_ms / vote_calls, frag_ms / frag_calls, fv_ms / fv_calls
    print("%-7s fragment-vote kernels %.3f ms per call (%d calls) | vote kernels %.3f ms | fragment kernel %.3f ms | / votes %.2f | "
          "/ fragments %.2f | %.3f ns per hit" % (name, x, fv_calls, v, f, x / v, x / f, x * 1e6 / max(total, 1)))


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
