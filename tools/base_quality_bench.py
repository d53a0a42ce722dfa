#!/usr/bin/env python3
"""What masking low-quality bases (kid_mask_batch_device) costs next to classifying the same reads.

One batch resident in HBM: --pairs (1 M) pairs of 150-base reads of bact10-synth at --scale (1.0 = 108.6 M k-mers,
2^30 cells) with the qualities of synth.qualities, laid out like the bases.  After a warm-up, alternating in one process:
the mask kernel at --q between two HIP events on its stream, and kid_sample_kernel_time_device of classifying the batch
(masked: the text the kernel leaves; the same figure for the untouched text first).  The mask kernel decides from the
qualities alone, so every repetition on the already masked text does the same loads and the same stores.
Bytes the kernel needs: one read of every quality byte, one byte store per masked base.  Output: stdout, and with
--out a copy under that directory (profiles/basequal/)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from kmer_id_amd import synth  # noqa: E402


def classify_ms(s, d, n, calls):
    off = torch.arange(n + 1, dtype=torch.int64, device=d.device) * bench.READ_LEN
    for i in range(calls + 2):
        if i == 2:
            torch.cuda.synchronize()
            s.kernel_time_device()
        s.classify_device(d.data_ptr(), n * bench.READ_LEN, off.data_ptr(), n)
    ms, batches = s.kernel_time_device()
    return ms / batches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--log2-slots", type=int, default=30)
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--q", type=int, default=20)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="directory that receives mask_kernel.txt")
    a = ap.parse_args()
    device = torch.device("cuda", 0)
    n, L = 2 * a.pairs, bench.READ_LEN
    db, parent, cum, _, _, _ = bench.build_db(device, a.scale, a.log2_slots, False)
    d = bench.gen_reads(device, cum, parent, 0, n)
    d_q = torch.empty(n * L + 64, dtype=torch.uint8, device=device)
    expect = 0
    for r0 in range(0, n, 1 << 18):  # (the qualities come from numpy: a piece at a time)
        q = synth.qualities(min(1 << 18, n - r0), L, r0=r0).reshape(-1)
        expect += int((q.view(np.int8) < a.q + 33).sum())
        d_q[r0 * L:r0 * L + q.size] = torch.from_numpy(q).to(device)
    off = torch.arange(n + 1, dtype=torch.int64, device=device) * L
    counter = torch.zeros(1, dtype=torch.int64, device=device)
    s = db.sample()
    plain_ms = classify_ms(s, d, n, a.calls)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.calls)]
    for i in range(a.warmup + a.calls):
        if i >= a.warmup:
            ev[i - a.warmup][0].record()
        db.mask_low_quality_device(d.data_ptr(), d_q.data_ptr(), off.data_ptr(), n, a.q, counter.data_ptr())
        if i >= a.warmup:
            ev[i - a.warmup][1].record()
    torch.cuda.synchronize()
    assert int(counter.item()) == (a.warmup + a.calls) * expect, "the kernel masked another number of bases than numpy"
    times = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    mask_ms = times[len(times) // 2]
    masked_ms = classify_ms(s, d, n, a.calls)
    s.close()
    nbytes = n * L + expect
    lines = [
        "%d pairs of %d bases, scale %g, Q = %d: %d of %d bases masked (%.2f %%)" % (a.pairs, L, a.scale, a.q, expect, n * L, 100.0 * expect / (n * L)),
        "mask kernel      median %.4f ms of %d calls (min %.4f, max %.4f): %.1f GB/s of the %.3f GB it needs (qualities read + bytes stored)" % (
            mask_ms, a.calls, times[0], times[-1], nbytes / mask_ms / 1e6, nbytes / 1e9),
        "classify kernel  %.4f ms per batch on the untouched text, %.4f ms on the masked text (device clock, %d batches each)" % (plain_ms, masked_ms, a.calls),
        "mask / classify  %.4f (untouched text)" % (mask_ms / plain_ms),
    ]
    print("\n".join(lines))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "mask_kernel.txt"), "w") as fh:
            fh.write("tools/base_quality_bench.py " + " ".join(sys.argv[1:]) + "\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
