#!/usr/bin/env python3
"""What the fragment-loci kernels (kid_db_fragment_loci_from_hits_device) cost next to the loci kernels on the same hits.

The database is bact10-synth at --scale (1.0 = 108.6 M k-mers, 2^30 cells) with the made-up sites of tools/read_loci_bench.py
(org = entry / 50000, pos = entry % 50000).  Every workload is an interleaved hit CSR resident in HBM, read once by the loci
kernels as 2 F reads (kid_db_loci_from_hits_device, diag_bin 1) and once by the fragment-loci kernels as F fragments (diag_bin
1, max_span 1000); device time comes from HIP events (kid_db_read_loci_time, kid_db_read_fragment_loci_time), after --warmup
calls, the two families alternating in one process:
  sparse   --fragments fragments with 0..3 hits per mate, what a sparse probe database gives: half of them a proper pair (a hit
           of mate 2 lies 0..600 positions above one of mate 1 on the same organism), the others uniform over the entries.
           Every fragment is taken by a lane of the first kernel
  metric   the hit CSR of the metric's 150-base reads (bench.gen_reads through kid_db_read_hits_device), read 2 i and read
           2 i + 1 taken as the mates of fragment i: the mix of both regimes that a dense database gives
  wg       --wg-fragments fragments with LANE + 1 .. 40 hits in mate 1 and 0..40 in mate 2, uniform over a window of 20 000
           entries of one organism: every fragment goes to the workgroup kernel, a few hundred pairs within max_span each
  wg-long  --wg-fragments / 16 fragments with 300 hits in each mate, the same way: the sort of 512 keys, twice per orientation
The times and the ratio fragment-loci / loci are reported, not judged; the records' own counts (fragments per regime, paired
bests) are printed so that a figure can be read against what the kernels were given."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from kmer_id_amd import FRAGMENT_LOCUS_DTYPE  # noqa: E402

PER_ORG = 50000
LANE_HITS = 4  # KID_FLOCI_LANE_HITS


def csr(ms, pos, entry):
    """per-read hit counts int64[n], pos and entry int64[total] on the device -> (offsets int64[n + 1], hits int32[total, 3], n_kmers int32[n])"""
    off = torch.zeros(ms.numel() + 1, dtype=torch.int64, device=ms.device)
    off[1:] = torch.cumsum(ms, 0)
    hits = torch.stack([pos, torch.ones_like(pos), entry], 1).to(torch.int32).contiguous()
    return off, hits, torch.full((ms.numel(),), 121, dtype=torch.int32, device=ms.device)


def sparse(device, n_frag, n_entries, seed=11):
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    rnd = lambda hi, n: torch.randint(0, hi, (n,), generator=g, device=device, dtype=torch.int64)  # noqa: E731
    ms = rnd(4, 2 * n_frag)
    ms[0::2][ms[0::2] + ms[1::2] == 0] = 1  # (a fragment without any hit is not what the hit pass hands on)
    off = torch.zeros(2 * n_frag + 1, dtype=torch.int64, device=device)
    off[1:] = torch.cumsum(ms, 0)
    total = int(off[-1].item())
    read_of = torch.repeat_interleave(torch.arange(2 * n_frag, device=device), ms)
    frag_of = read_of // 2
    pos, entry = rnd(121, total), rnd(n_entries, total)
    # a proper pair in every second fragment: all hits of the fragment near one anchor entry of one organism, mate 1's on the
    # forward diagonal of the anchor, mate 2's on a reverse diagonal 0..600 above it
    anchor = (rnd(n_entries // PER_ORG, n_frag) * PER_ORG + 1000 + rnd(PER_ORG - 3000, n_frag))[frag_of]
    insert = rnd(600, n_frag)[frag_of]
    proper = (frag_of % 2 == 0)
    mate2 = (read_of % 2 == 1)
    e_fwd, e_rev = anchor + pos, anchor + insert - pos
    entry = torch.where(proper, torch.where(mate2, e_rev, e_fwd), entry)
    return csr(ms, pos, entry.clamp_(0, n_entries - 1))


def workgroup(device, n_frag, n_entries, m1, m2, seed=13):
    """m1, m2: (lowest, highest) hit count of the mates"""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    rnd = lambda lo, hi, n: torch.randint(lo, hi + 1, (n,), generator=g, device=device, dtype=torch.int64)  # noqa: E731
    ms = torch.stack([rnd(m1[0], m1[1], n_frag), rnd(m2[0], m2[1], n_frag)], 1).reshape(-1)
    total = int(ms.sum().item())
    frag_of = torch.repeat_interleave(torch.arange(2 * n_frag, device=device), ms) // 2
    base = (rnd(0, n_entries // PER_ORG - 1, n_frag) * PER_ORG + rnd(0, PER_ORG - 20001, n_frag))[frag_of]
    return csr(ms, rnd(0, 120, total), base + rnd(0, 19999, total))


def metric(device, db, cum, parent, n_reads):
    d_bases = bench.gen_reads(device, cum, parent, 0, n_reads)
    off = torch.arange(n_reads + 1, dtype=torch.int64, device=device) * 150
    d_ho = torch.empty(n_reads + 1, dtype=torch.int64, device=device)
    d_nk = torch.empty(n_reads, dtype=torch.int32, device=device)
    d_tot = torch.zeros(1, dtype=torch.int64, device=device)
    args = (d_bases.data_ptr(), n_reads * 150, off.data_ptr(), n_reads, d_ho.data_ptr(), d_tot.data_ptr())
    db.read_hits_device(*args, d_n_kmers=d_nk.data_ptr())  # the sizing call
    torch.cuda.synchronize()
    total = int(d_tot.item())
    d_hits = torch.empty(max(total, 1) * 3, dtype=torch.int32, device=device)
    db.read_hits_device(*args, d_n_kmers=d_nk.data_ptr(), d_hits=d_hits.data_ptr(), cap=total)
    torch.cuda.synchronize()
    return d_ho, d_hits.view(-1, 3), d_nk


def measure(db, name, work, calls, warmup):
    off, hits, nk = work
    n = off.numel() - 1
    total = int(off[-1].item())
    d_loc = torch.zeros(n * 10, dtype=torch.int32, device=off.device)
    d_frag = torch.zeros(n // 2 * 16, dtype=torch.int32, device=off.device)
    for i in range(warmup + calls):
        if i == warmup:
            torch.cuda.synchronize()
            db.read_loci_time(), db.read_fragment_loci_time()
        db.loci_from_hits_device(off.data_ptr(), hits.data_ptr(), nk.data_ptr(), n, d_loc.data_ptr(), diag_bin=1)
        db.fragment_loci_from_hits_device(off.data_ptr(), hits.data_ptr(), nk.data_ptr(), n, d_frag.data_ptr(), diag_bin=1, max_span=1000)
    l_ms, l_calls, l_reads = db.read_loci_time()
    f_ms, f_calls, f_frags = db.read_fragment_loci_time()
    assert (l_calls, l_reads, f_calls, f_frags) == (calls, calls * n, calls, calls * (n // 2))
    recs = d_frag.cpu().numpy().view(np.uint32).view(FRAGMENT_LOCUS_DTYPE)
    ms = (off[1:] - off[:-1]).cpu().numpy()
    big = int(((ms[0::2] > LANE_HITS) | (ms[1::2] > LANE_HITS)).sum())
    assert int(recs["n_hits"].astype(np.int64).sum()) == total  # every fragment was written, by one kernel or the other
    lo, fr = l_ms / l_calls, f_ms / f_calls
    print("%-8s %d fragments, %d hits, %d for the workgroup kernel, %d paired / %d solo bests" % (
        name, n // 2, total, big, int((recs["mates"] == 3).sum()), int(((recs["mates"] == 1) | (recs["mates"] == 2)).sum())))
    print("%-8s loci kernels %.3f ms per call (%.2f ns per read) | fragment-loci kernels %.3f ms per call (%.2f ns per fragment) | "
          "fragment-loci / loci %.2f (%d calls each)" % ("", lo, lo * 1e6 / n, fr, fr * 1e6 / (n // 2), fr / lo, calls))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--log2-slots", type=int, default=30)
    ap.add_argument("--fragments", type=int, default=1_000_000)
    ap.add_argument("--wg-fragments", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    device = torch.device("cuda", 0)
    db, parent, cum, build_s, _, _ = bench.build_db(device, a.scale, a.log2_slots, False)
    n_entries = db.info.n_entries
    e = np.arange(n_entries, dtype=np.uint64)
    db.set_sites((e // PER_ORG).astype(np.uint32), (e % PER_ORG).astype(np.uint32))
    del e
    print("database: %d entries, %d organisms of %d positions" % (n_entries, (n_entries + PER_ORG - 1) // PER_ORG, PER_ORG))
    measure(db, "sparse", sparse(device, a.fragments, n_entries), a.calls, a.warmup)
    measure(db, "metric", metric(device, db, cum, parent, 2 * a.fragments), a.calls, a.warmup)
    measure(db, "wg", workgroup(device, a.wg_fragments, n_entries, (LANE_HITS + 1, 40), (0, 40)), a.calls, a.warmup)
    measure(db, "wg-long", workgroup(device, max(a.wg_fragments // 16, 1), n_entries, (300, 300), (300, 300)), max(a.calls // 4, 1), 1)
    db.close()


if __name__ == "__main__":
    main()
