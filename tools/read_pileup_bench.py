#!/usr/bin/env python3
"""What the pileup's add kernel (kid_pileup_add_device) costs next to the loci kernels, and what a summary costs.

The database is bact10-synth at --scale (1.0 = 108.6 M k-mers, 2^30 cells) with the made-up sites of
tools/read_loci_bench.py (org = entry / 50000, pos = entry % 50000: 2172 organisms of 50 000 positions), piled up in bins of
--bin-width bases (10: 10.9 M bins).  Everything is resident in HBM; device time comes from HIP events (kid_pileup_time,
kid_db_read_loci_time, and events on the null stream around a summary), after --warmup calls, the workloads alternating in
one process:
  loci     the loci kernels on the hit CSR of the metric's 2 M 150-base reads: what produces 2 M records
  (a)      the add kernel on 2 M records whose placements are uniform over the geometry: entry_first drawn uniformly from
           the entries, a chain of 121 positions, strands alternating; every record is placed
  (b)      the same records all placed in one bin of one organism: the hot spot, every atomic of a launch on three addresses
  (c)      kid_pileup_summary alone at that geometry: the scan of the steps (three kernels), the reduce kernel and the
           records back (48 bytes per organism)
The times and the ratios add / loci and (b) / (a) are reported, not judged."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

PER_ORG = 50000


def records(device, n, n_entries, hot_entry=None):
    """kid_locus[n] as int32[n, 10]: org, strand, n_chain, n_org, n_other, n_hits, n_kmers, pos_first, pos_last, entry_first"""
    g = torch.Generator(device=device)
    g.manual_seed(7)
    e = torch.randint(0, n_entries, (n,), generator=g, device=device, dtype=torch.int64)
    if hot_entry is not None:
        e = torch.full_like(e, hot_entry)
    r = torch.zeros(n, 10, dtype=torch.int32, device=device)
    r[:, 0] = (e // PER_ORG).to(torch.int32)
    r[:, 1] = 0 if hot_entry is not None else (torch.arange(n, device=device) & 1).to(torch.int32)
    r[:, 2] = r[:, 3] = r[:, 5] = 40
    r[:, 6] = 121
    r[:, 8] = 0 if hot_entry is not None else 120  # (the hot spot: d = 0, every record starts in one bin and covers its k-mer's)
    r[:, 9] = e.to(torch.int32)
    return r.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--log2-slots", type=int, default=30)
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--bin-width", type=int, default=10)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    device = torch.device("cuda", 0)
    db, parent, cum, build_s, _, _ = bench.build_db(device, a.scale, a.log2_slots, False)
    n, n_entries = a.reads, db.info.n_entries
    e = np.arange(n_entries, dtype=np.uint64)
    db.set_sites((e // PER_ORG).astype(np.uint32), (e % PER_ORG).astype(np.uint32))
    del e
    # the loci kernels' input: the hit CSR of the metric's reads
    d_bases = bench.gen_reads(device, cum, parent, 0, n)
    off = torch.arange(n + 1, dtype=torch.int64, device=device) * 150
    d_ho = torch.empty(n + 1, dtype=torch.int64, device=device)
    d_nk = torch.empty(n, dtype=torch.int32, device=device)
    d_tot = torch.zeros(1, dtype=torch.int64, device=device)
    d_loc = torch.zeros(n * 10, dtype=torch.int32, device=device)
    args = (d_bases.data_ptr(), n * 150, off.data_ptr(), n, d_ho.data_ptr(), d_tot.data_ptr())
    db.read_hits_device(*args, d_n_kmers=d_nk.data_ptr())  # the sizing call
    torch.cuda.synchronize()
    total = int(d_tot.item())
    d_hits = torch.empty(max(total, 1) * 3, dtype=torch.int32, device=device)
    db.read_hits_device(*args, d_n_kmers=d_nk.data_ptr(), d_hits=d_hits.data_ptr(), cap=total)
    uniform = records(device, n, n_entries)
    hot = records(device, n, n_entries, hot_entry=n_entries // 2 + 25005)
    torch.cuda.synchronize()
    w = a.bin_width
    with db.pileup(w) as pa, db.pileup(w) as pb:
        print("geometry: %d entries, %d organisms, %d bins of %d bases, %d slots of the step array" % (
            n_entries, pa.n_orgs, pa.n_bins, w, pa.n_bins + pa.n_orgs))
        for i in range(a.warmup + a.calls):
            if i == a.warmup:
                torch.cuda.synchronize()
                db.read_loci_time(), pa.time(), pb.time()
            db.loci_from_hits_device(d_ho.data_ptr(), d_hits.data_ptr(), d_nk.data_ptr(), n, d_loc.data_ptr(), diag_bin=1)
            pa.add_device(uniform.data_ptr(), n, 2, 1)
            pb.add_device(hot.data_ptr(), n, 2, 1)
        loci_ms, loci_calls, _ = db.read_loci_time()
        a_ms, a_calls, _ = pa.time()
        b_ms, b_calls, _ = pb.time()
        # both piled up what they were handed, or no figure below means anything
        every = a.warmup + a.calls
        assert pa.counts() == (every * n, every * n) and pb.counts() == (every * n, every * n)
        rb = pb.summary()
        assert int((rb["n_placed"] > 0).sum()) == 1 and int(rb["max_depth"].max()) == int(rb["max_starts"].max()) == (every * n) % 2 ** 32
        assert int(rb["bins_covered"].sum()) <= (bench.K + w - 2) // w + 1  # (one start bin; the k-mer there reaches over ceil(k / W) bins)
        ra = pa.summary()
        assert int(ra["n_placed"].astype(np.uint64).sum()) == every * n and int(ra["depth_sum"].sum()) > every * n
        lo, aa, bb = loci_ms / loci_calls, a_ms / a_calls, b_ms / b_calls
        print("loci     %d reads, %d hits: loci kernels %.3f ms per call (%d calls), %.3f ns per read" % (n, total, lo, loci_calls, lo * 1e6 / n))
        print("(a)      %d records, uniform: add kernel %.3f ms per call (%d calls), %.3f ns per record | add / loci %.2f" % (
            n, aa, a_calls, aa * 1e6 / n, aa / lo))
        print("(b)      %d records, one bin: add kernel %.3f ms per call (%d calls), %.3f ns per record | add / loci %.2f | (b) / (a) %.2f" % (
            n, bb, b_calls, bb * 1e6 / n, bb / lo, bb / aa))
        # (c) the summary alone: events on the null stream, where its kernels run, and the host's clock around the call
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        dev_ms, host_ms = [], []
        for i in range(a.warmup + a.calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev0.record()
            pa.summary()
            ev1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                host_ms.append((time.perf_counter() - t0) * 1e3)
                dev_ms.append(ev0.elapsed_time(ev1))
        print("(c)      summary of %d organisms, %d slots: %.3f ms between events (min %.3f, max %.3f), %.3f ms on the host's clock (%d calls)" % (
            pa.n_orgs, pa.n_bins + pa.n_orgs, sum(dev_ms) / len(dev_ms), min(dev_ms), max(dev_ms), sum(host_ms) / len(host_ms), len(dev_ms)))
    db.close()


if __name__ == "__main__":
    main()
