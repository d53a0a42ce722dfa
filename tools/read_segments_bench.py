#!/usr/bin/env python3
"""What the segment kernels (kid_db_read_segments_device: segments per read and their scan, the scan of the valid masks,
kid_segments_kernel) cost next to the hit pass and to the support kernel on the same batches.

  metric    2 M 150-base reads of bact10-synth at --scale (those of tools/read_support_bench.py), seg_len above the read
            length: one segment per read, i.e. the support kernel's work plus two scans and four prefix queries per
            segment.  The records' six shared fields are checked against the support kernel's.
  megabase  --records records of --record-len bases drawn from a random genome whose every window is in the database
            (one target per 50 kb block), at 1000:500 and 1000:100: every hit is folded 2 and 10 times by the wave path.
For each, alternating in one process after a warm-up: device time per call of the segment kernels alone
(kid_db_read_segments_time), of the hits kernels (kid_db_read_hits_time) and, for metric, of the support kernel
(kid_db_read_support_time).  The rule is --min-hits / --min-permille (2, 20)."""
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
from read_hits_bench import READ_LEN  # noqa: E402


class Batch:
    """a batch resident in HBM with the buffers of kid_db_read_segments_device, sized by a first call"""

    def __init__(self, db, d_bases, off, seg, rule):
        dev = d_bases.device
        self.db, self.d_bases, self.off, self.n, self.seg, self.rule = db, d_bases, off, off.numel() - 1, seg, rule
        self.nbytes = int(off[-1].item())
        self.d_so = torch.empty(self.n + 1, dtype=torch.int64, device=dev)
        self.d_nh = torch.zeros(1, dtype=torch.int64, device=dev)
        self.d_ns = torch.zeros(1, dtype=torch.int64, device=dev)
        self.d_hits = self.d_seg = None
        self.hits = self.segs = 0
        self.run()  # the sizing call
        torch.cuda.synchronize()
        self.hits, self.segs = int(self.d_nh.item()), int(self.d_ns.item())
        self.d_hits = torch.empty(max(self.hits, 1) * 3, dtype=torch.int32, device=dev)
        self.d_seg = torch.zeros(max(self.segs, 1) * 8, dtype=torch.int32, device=dev)

    def run(self):
        self.db.read_segments_device(self.d_bases.data_ptr(), self.nbytes, self.off.data_ptr(), self.n, self.seg[0], self.seg[1],
                                     self.d_so.data_ptr(), self.d_nh.data_ptr(), self.d_ns.data_ptr(), min_hits=self.rule[0],
                                     min_permille=self.rule[1], d_hits=self.d_hits.data_ptr() if self.d_hits is not None else 0,
                                     hits_cap=self.hits, d_segments=self.d_seg.data_ptr() if self.d_seg is not None else 0, seg_cap=self.segs)


def timed(db, calls, warmup, step):
    for i in range(warmup + calls):
        if i == warmup:
            torch.cuda.synchronize()
            db.read_hits_time(), db.read_support_time(), db.read_segments_time()
        step()
    seg_ms, seg_calls, _ = db.read_segments_time()
    hit_ms, hit_calls, _ = db.read_hits_time()
    sup_ms, sup_calls, _ = db.read_support_time()
    return seg_ms / seg_calls, hit_ms / hit_calls, sup_ms / sup_calls if sup_calls else 0.0


def metric(db, d_bases, n, calls, warmup, rule):
    dev = d_bases.device
    off = torch.arange(n + 1, dtype=torch.int64, device=dev) * READ_LEN
    b = Batch(db, d_bases, off, (10 ** 6, 10 ** 6), rule)
    d_ho = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_nk = torch.empty(n, dtype=torch.int32, device=dev)
    d_tot = torch.zeros(1, dtype=torch.int64, device=dev)
    d_out = torch.zeros(n * 6, dtype=torch.int32, device=dev)

    def step():
        db.read_hits_device(d_bases.data_ptr(), n * READ_LEN, off.data_ptr(), n, d_ho.data_ptr(), d_tot.data_ptr(), d_n_kmers=d_nk.data_ptr(),
                            d_hits=b.d_hits.data_ptr(), cap=b.hits)
        db.support_from_hits_device(d_ho.data_ptr(), b.d_hits.data_ptr(), d_nk.data_ptr(), n, d_out.data_ptr(), min_hits=rule[0],
                                    min_permille=rule[1])
        b.run()

    seg, hit, sup = timed(db, calls, warmup, step)
    torch.cuda.synchronize()
    # one segment per read: the same records, or no figure below means anything
    assert b.segs == n and int(d_tot.item()) == b.hits
    rec = b.d_seg.view(n, 8)
    assert torch.equal(rec[:, 2:], d_out.view(n, 6)) and int(rec[:, 0].sum().item()) == 0 and bool((rec[:, 1] == READ_LEN - bench.K + 1).all())
    print("metric   %d reads, %d hits (%.2f per read), %d segments, rule (%d, %d)" % (n, b.hits, b.hits / n, b.segs, rule[0], rule[1]))
    print("metric   segment kernels %.3f ms per call (%d calls) | support kernel %.3f ms | hits kernels %.3f ms | segments / support %.2f | "
          "segments / hits %.3f" % (seg, calls, sup, hit, seg / sup, seg / hit))


def megabase(parent, n_rec, rec_len, calls, warmup, rule):
    rng = np.random.default_rng(5)
    k = bench.K
    glen = 4 * rec_len
    g = rng.choice(np.frombuffer(b"ACGT", np.uint8), glen)
    code = np.zeros(256, np.uint64)
    for j, ch in enumerate(b"ACGT"):
        code[ch] = j
    c = code[g]
    nwin = glen - k + 1
    kf, kr = np.zeros(nwin, np.uint64), np.zeros(nwin, np.uint64)
    for j in range(k):
        kf = (kf << np.uint64(2)) | c[j:j + nwin]
        kr = (kr << np.uint64(2)) | (np.uint64(3) - c[k - 1 - j:k - 1 - j + nwin])
    keys = np.minimum(kf, kr)
    block_t = rng.integers(2, parent.size, nwin // 50000 + 1).astype(np.uint32)
    targets = block_t[np.arange(nwin) // 50000]
    db = KmerDB(keys, targets, parent, k=k, log2_slots=int(np.ceil(np.log2(nwin * 2))))
    at = rng.integers(0, glen - rec_len + 1, n_rec)
    text = np.concatenate([g[a:a + rec_len] for a in at] + [np.zeros(64, np.uint8)])
    d_bases = torch.from_numpy(text).cuda()
    off = torch.arange(n_rec + 1, dtype=torch.int64, device=d_bases.device) * rec_len
    for seg in [(1000, 500), (1000, 100)]:
        b = Batch(db, d_bases, off, seg, rule)
        seg_ms, hit_ms, _ = timed(db, calls, warmup, b.run)
        torch.cuda.synchronize()
        rec = b.d_seg.view(b.segs, 8).to(torch.int64)
        assert int(b.d_ns.item()) == b.segs and bool((rec[:, 5] == rec[:, 1]).all()) and bool((rec[:, 2] > 0).all())  # every window a hit
        print("megabase %d records of %d bases, %d hits, %d:%d -> %d segments (each hit folded %.1f times), rule (%d, %d)" % (
            n_rec, rec_len, b.hits, seg[0], seg[1], b.segs, float(rec[:, 5].sum().item()) / b.hits, rule[0], rule[1]))
        print("megabase %d:%d segment kernels %.3f ms per call (%d calls) | hits kernels %.3f ms | segments / hits %.3f | %.1f M segments/s" % (
            seg[0], seg[1], seg_ms, calls, hit_ms, seg_ms / hit_ms, b.segs / seg_ms / 1e3))
    db.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--log2-slots", type=int, default=30)
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--records", type=int, default=16)
    ap.add_argument("--record-len", type=int, default=1_000_000)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--min-hits", type=int, default=2)
    ap.add_argument("--min-permille", type=int, default=20)
    ap.add_argument("--skip-metric", action="store_true")
    ap.add_argument("--skip-megabase", action="store_true")
    a = ap.parse_args()
    rule = (a.min_hits, a.min_permille)
    device = torch.device("cuda", 0)
    parent = None
    if not a.skip_metric:
        db, parent, cum, build_s, _, _ = bench.build_db(device, a.scale, a.log2_slots, False)
        d = bench.gen_reads(device, cum, parent, 0, a.reads)
        metric(db, d, a.reads, a.calls, a.warmup, rule)
        db.close()
        del d
    if not a.skip_megabase:
        if parent is None:
            from kmer_id_amd import synth
            parent, _ = synth.load_taxonomy("bact10")
        megabase(parent, a.records, a.record_len, a.calls, a.warmup, rule)


if __name__ == "__main__":
    main()
