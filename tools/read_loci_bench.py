#!/usr/bin/env python3
"""What the loci kernels (kid_db_loci_from_hits_device) cost next to the support kernel on the same hit CSR.

Three workloads resident in HBM (the first that of tools/read_support_bench.py, the others cut like tools/read_votes_bench.py's):
  metric  2 M 150-base reads of bact10-synth at --scale (1.0 = 108.6 M k-mers, 2^30 cells), ~1 % of the windows hit:
          the lane-per-read regime; the sites are made up (org = entry / 50000, pos = entry % 50000)
  dense   2 M reads of --dense-len bases (149: 120 windows) cut from genomes the database holds: the windows whose
          forward k-mer is the canonical one hit, 60 per read, all on one diagonal -- the wave-per-read regime, every
          lane's two keys against the keys of all hits; the sites are the genome and the window's start
  long    --long-reads reads of --long-len bases cut from the same genomes: more than KID_LOCI_WAVE_HITS hits per read,
          all of them left to kid_loci_big_kernel (two sorts in LDS per read)
For each, alternating in one process after a warm-up: device time per call of the loci kernels alone
(kid_db_read_loci_time: both kernels and the list's reset between the two events) and of the support kernel alone
(kid_db_read_support_time), per read and per hit.  The ratio is reported, not judged."""
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
from read_hits_bench import genome_db  # noqa: E402
from read_votes_bench import cut_reads  # noqa: E402


def measure(name, db, d_bases, n, read_len, calls, warmup, diag_bin):
    dev = d_bases.device
    off = torch.arange(n + 1, dtype=torch.int64, device=dev) * read_len
    d_ho = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_nk = torch.empty(n, dtype=torch.int32, device=dev)
    d_tot = torch.zeros(1, dtype=torch.int64, device=dev)
    d_sup = torch.zeros(n * 6, dtype=torch.int32, device=dev)
    d_loc = torch.zeros(n * 10, dtype=torch.int32, device=dev)
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
            db.read_loci_time()
        db.support_from_hits_device(d_ho.data_ptr(), d_hits.data_ptr(), d_nk.data_ptr(), n, d_sup.data_ptr())
        db.loci_from_hits_device(d_ho.data_ptr(), d_hits.data_ptr(), d_nk.data_ptr(), n, d_loc.data_ptr(), diag_bin=diag_bin)
    sup_ms, sup_calls, _ = db.read_support_time()
    loc_ms, loc_calls, _ = db.read_loci_time()
    torch.cuda.synchronize()
    sup, loc = d_sup.view(n, 6), d_loc.view(n, 10)
    # the two saw the same hits, or no figure below means anything
    assert torch.equal(sup[:, 3], loc[:, 5]) and int(loc[:, 5].to(torch.int64).sum().item()) == total
    per = loc[:, 5].to(torch.int64)
    chain = loc[:, 2].to(torch.int64)
    print("%-7s %d reads of %d bases, %d hits (%.1f per read; %d reads above 8 hits, %d above 256), W = %d: %d reads placed, %d with every "
          "hit on the chain, %d on strand 1, %d with n_other > 0" % (
              name, n, read_len, total, total / n, int((per > 8).sum().item()), int((per > 256).sum().item()), diag_bin,
              int((chain > 0).sum().item()), int(((chain == per) & (per > 0)).sum().item()), int((loc[:, 1] > 0).sum().item()),
              int((loc[:, 4] > 0).sum().item())))
    s, v = sup_ms / sup_calls, loc_ms / loc_calls
    print("%-7s loci kernels %.3f ms per call (%d calls), %.3f ns per read, %.3f ns per hit | support kernel %.3f ms, %.3f ns per read, "
          "%.3f ns per hit | loci / support %.2f" % (name, v, loc_calls, v * 1e6 / n, v * 1e6 / max(total, 1), s, s * 1e6 / n,
                                                      s * 1e6 / max(total, 1), v / s))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--log2-slots", type=int, default=30)
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--dense-len", type=int, default=149)
    ap.add_argument("--long-reads", type=int, default=20_000)
    ap.add_argument("--long-len", type=int, default=1200)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--diag-bin", type=int, default=1)
    ap.add_argument("--skip-metric", action="store_true")
    a = ap.parse_args()
    device = torch.device("cuda", 0)
    db, parent, cum, build_s, _, _ = bench.build_db(device, a.scale, a.log2_slots, False)
    if not a.skip_metric:
        e = np.arange(db.info.n_entries, dtype=np.uint64)
        db.set_sites((e // 50000).astype(np.uint32), (e % 50000).astype(np.uint32))
        del e
        d = bench.gen_reads(device, cum, parent, 0, a.reads)
        measure("metric", db, d, a.reads, 150, a.calls, a.warmup, a.diag_bin)
        del d
    db.close()
    rng = np.random.default_rng(3)
    n_genomes, genome_len = 400, 20000
    G, keys, targets = genome_db(parent, bench.K, rng, n_genomes, genome_len)
    nwin = genome_len - bench.K + 1
    db = KmerDB(keys, targets, parent, k=bench.K, log2_slots=26)
    e = np.arange(keys.size, dtype=np.uint64)
    db.set_sites((e // nwin).astype(np.uint32), (e % nwin).astype(np.uint32))
    measure("dense", db, cut_reads(G, rng, a.reads, a.dense_len), a.reads, a.dense_len, a.calls, a.warmup, a.diag_bin)
    measure("long", db, cut_reads(G, rng, a.long_reads, a.long_len), a.long_reads, a.long_len, a.calls, a.warmup, a.diag_bin)


if __name__ == "__main__":
    main()
