#!/usr/bin/env python3
"""What the segment-vote kernels (kid_db_read_segment_votes_device: the two scans, kid_segment_votes_kernel and
kid_segment_votes_big_kernel) cost next to the segment kernels (kid_db_read_segments_device: the same scans and
kid_segments_kernel) and next to the vote kernels (kid_db_votes_from_hits_device) on the same hit lists.

  metric    2 M 150-base reads of bact10-synth at --scale (those of tools/read_segments_bench.py), seg_len above the read
            length: one segment per read, the lane regime.  The vote kernels run on the hit CSR of the same reads; the
            eight vote fields of the two are checked against each other, the geometry against the segment kernels'.
  long      one record of --record-len bases drawn from a random genome whose every window is in the database (one target
            per 50 kb block, so nearly every segment lies on one or two targets), at 1000:1000, 4096:1024 and 1024:1:
            every segment holds more than KID_VOTE_WAVE_HITS hits and is left to the workgroup kernel; at 1024:1 every hit
            is visited by 1024 segments.  The vote kernels run on the CSR that makes every segment of LEN:LEN a read
            (each hit once): at 1000:1000 those are the same hit lists and the records are checked field by field; under
            overlap the segment-vote kernels do LEN / STEP times that work by the rule.
For each, alternating in one process after a warm-up: device time per call of the segment-vote kernels alone
(kid_db_read_segment_votes_time), of the segment kernels alone (kid_db_read_segments_time) and of the vote kernels alone
(kid_db_read_votes_time).  No ratio is judged.  The rule is --min-hits / --min-permille (2, 20)."""
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
from read_segments_bench import Batch  # noqa: E402


class VoteBatch(Batch):
    """the buffers of kid_db_read_segment_votes_device (ten words per record), sized by a first call"""

    def __init__(self, db, d_bases, off, seg, rule):
        super().__init__(db, d_bases, off, seg, rule)
        self.d_seg = torch.zeros(max(self.segs, 1) * 10, dtype=torch.int32, device=d_bases.device)

    def run(self):
        self.db.read_segment_votes_device(self.d_bases.data_ptr(), self.nbytes, self.off.data_ptr(), self.n, self.seg[0], self.seg[1],
                                          self.d_so.data_ptr(), self.d_nh.data_ptr(), self.d_ns.data_ptr(), min_hits=self.rule[0],
                                          min_permille=self.rule[1], d_hits=self.d_hits.data_ptr() if self.d_hits is not None else 0,
                                          hits_cap=self.hits, d_segments=self.d_seg.data_ptr() if self.d_seg is not None else 0,
                                          seg_cap=self.segs)


def timed(db, calls, warmup, steps):
    for i in range(warmup + calls):
        if i == warmup:
            torch.cuda.synchronize()
            db.read_hits_time(), db.read_votes_time(), db.read_segments_time(), db.read_segment_votes_time()
        for step in steps:
            step()
    sv_ms, sv_calls, _ = db.read_segment_votes_time()
    seg_ms, seg_calls, _ = db.read_segments_time()
    vote_ms, vote_calls, _ = db.read_votes_time()
    torch.cuda.synchronize()
    return sv_ms / sv_calls, seg_ms / seg_calls, vote_ms / vote_calls if vote_calls else 0.0


def regimes(m):
    return int(((m > 0) & (m <= 8)).sum().item()), int(((m > 8) & (m <= 512)).sum().item()), int((m > 512).sum().item())


def report(name, what, sv, seg, vote, segs, visits, calls):
    print("%-7s %s segment-vote kernels %.3f ms per call (%d calls) | segment kernels %.3f ms | vote kernels %.3f ms | / segments %.2f | "
          "/ votes %.2f | %.2f M segments/s | %.3f ns per hit visited" % (name, what, sv, calls, seg, vote, sv / seg, sv / vote if vote else 0.0,
                                                                            segs / sv / 1e3, sv * 1e6 / max(visits, 1)))


def metric(db, d_bases, n, calls, warmup, rule):
    dev = d_bases.device
    off = torch.arange(n + 1, dtype=torch.int64, device=dev) * READ_LEN
    seg = (10 ** 6, 10 ** 6)
    v, s = VoteBatch(db, d_bases, off, seg, rule), Batch(db, d_bases, off, seg, rule)
    d_ho = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_nk = torch.empty(n, dtype=torch.int32, device=dev)
    d_tot = torch.zeros(1, dtype=torch.int64, device=dev)
    d_vote = torch.zeros(n * 8, dtype=torch.int32, device=dev)
    db.read_hits_device(d_bases.data_ptr(), n * READ_LEN, off.data_ptr(), n, d_ho.data_ptr(), d_tot.data_ptr(), d_n_kmers=d_nk.data_ptr(),
                        d_hits=v.d_hits.data_ptr(), cap=v.hits)
    torch.cuda.synchronize()
    d_hits = v.d_hits.clone()  # (the segment calls write the same hits into their scratch again)

    def votes():
        db.votes_from_hits_device(d_ho.data_ptr(), d_hits.data_ptr(), d_nk.data_ptr(), n, d_vote.data_ptr(), min_hits=rule[0], min_permille=rule[1])

    sv, sg, vt = timed(db, calls, warmup, [v.run, s.run, votes])
    # one segment per read: the same records, or no figure below means anything
    assert v.segs == s.segs == n and int(d_tot.item()) == v.hits == s.hits
    rec, fold = v.d_seg.view(n, 10), s.d_seg.view(n, 8)
    assert torch.equal(rec[:, 2:], d_vote.view(n, 8)) and torch.equal(rec[:, :2], fold[:, :2]) and torch.equal(rec[:, 4:6], fold[:, 4:6])
    print("metric  %d reads, %d hits (%.2f per read), %d segments in the regimes (lane, wave, workgroup) = %s, rule (%d, %d): call != final for "
          "%d segments" % (n, v.hits, v.hits / n, v.segs, regimes(rec[:, 5]), rule[0], rule[1], int((rec[:, 2] != fold[:, 2]).sum().item())))
    report("metric", "1 segment per read:", sv, sg, vt, v.segs, v.hits, calls)


def long_record(parent, rec_len, calls, warmup, rule, settings):
    rng = np.random.default_rng(5)
    k = bench.K
    g = rng.choice(np.frombuffer(b"ACGT", np.uint8), rec_len)
    code = np.zeros(256, np.uint64)
    for j, ch in enumerate(b"ACGT"):
        code[ch] = j
    c = code[g]
    nwin = rec_len - k + 1
    kf, kr = np.zeros(nwin, np.uint64), np.zeros(nwin, np.uint64)
    for j in range(k):
        kf = (kf << np.uint64(2)) | c[j:j + nwin]
        kr = (kr << np.uint64(2)) | (np.uint64(3) - c[k - 1 - j:k - 1 - j + nwin])
    keys = np.minimum(kf, kr)
    block_t = rng.integers(2, parent.size, nwin // 50000 + 1).astype(np.uint32)
    targets = block_t[np.arange(nwin) // 50000]
    db = KmerDB(keys, targets, parent, k=k, log2_slots=int(np.ceil(np.log2(nwin * 2))))
    d_bases = torch.from_numpy(np.concatenate([g, np.zeros(64, np.uint8)])).cuda()
    dev = d_bases.device
    off = torch.tensor([0, rec_len], dtype=torch.int64, device=dev)
    for seg in settings:
        v, s = VoteBatch(db, d_bases, off, seg, rule), Batch(db, d_bases, off, seg, rule)
        # the yardstick of the vote kernels: every segment of LEN:LEN a read of a hit CSR (each hit once)
        flat = Batch(db, d_bases, off, (seg[0], seg[0]), rule)
        flat.run()
        torch.cuda.synchronize()
        frec = flat.d_seg.view(flat.segs, 8)
        d_ho = torch.zeros(flat.segs + 1, dtype=torch.int64, device=dev)
        d_ho[1:] = torch.cumsum(frec[:, 5].to(torch.int64), 0)
        d_nk = frec[:, 4].contiguous()
        d_hits = flat.d_hits.clone()
        d_vote = torch.zeros(flat.segs * 8, dtype=torch.int32, device=dev)

        def votes():
            db.votes_from_hits_device(d_ho.data_ptr(), d_hits.data_ptr(), d_nk.data_ptr(), flat.segs, d_vote.data_ptr(), min_hits=rule[0],
                                      min_permille=rule[1])

        sv, sg, vt = timed(db, calls, warmup, [v.run, s.run, votes])
        rec, fold = v.d_seg.view(v.segs, 10), s.d_seg.view(s.segs, 8)
        assert v.segs == s.segs and v.hits == s.hits == nwin and torch.equal(rec[:, :2], fold[:, :2]) and torch.equal(rec[:, 4:6], fold[:, 4:6])
        assert bool((rec[:, 5] == rec[:, 1]).all()) and bool((rec[:, 2] > 0).all())  # every window a hit
        if seg[0] == seg[1]:  # the same hit lists: the same records
            assert torch.equal(rec[:, 2:], d_vote.view(flat.segs, 8))
        visits = int(rec[:, 5].to(torch.int64).sum().item())
        print("long    1 record of %d bases, %d hits, %d:%d -> %d segments in the regimes (lane, wave, workgroup) = %s, each hit visited %.1f "
              "times, rule (%d, %d): call != final for %d segments, %d ties; the vote kernels' CSR: %d reads" % (
                  rec_len, v.hits, seg[0], seg[1], v.segs, regimes(rec[:, 5]), visits / v.hits, rule[0], rule[1],
                  int((rec[:, 2] != fold[:, 2]).sum().item()), int((rec[:, 7] > 1).sum().item()), flat.segs))
        report("long", "%d:%d" % seg, sv, sg, vt, v.segs, visits, calls)
        del v, s, flat
    db.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--log2-slots", type=int, default=30)
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--record-len", type=int, default=1_000_000)
    ap.add_argument("--settings", default="1000:1000,4096:1024,1024:1")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--min-hits", type=int, default=2)
    ap.add_argument("--min-permille", type=int, default=20)
    ap.add_argument("--skip-metric", action="store_true")
    ap.add_argument("--skip-long", action="store_true")
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
    if not a.skip_long:
        if parent is None:
            from kmer_id_amd import synth
            parent, _ = synth.load_taxonomy("bact10")
        settings = [tuple(int(x) for x in s.split(":")) for s in a.settings.split(",")]
        long_record(parent, a.record_len, a.calls, a.warmup, rule, settings)


if __name__ == "__main__":
    main()
