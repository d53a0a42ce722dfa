#!/usr/bin/env python3
"""What masking low-complexity sequence (kid_lowc_batch_device) costs next to classifying the same reads.

One batch resident in HBM: --pairs (1 M) pairs of 150-base reads of bact10-synth at --scale (1.0 = 108.6 M k-mers,
2^30 cells); every --every-th read (10: a tenth of them) carries a planted run of 40 bases of period 1, 2 or 3 at
offset 55.  The mask is not idempotent -- it would see its own 'N's -- so every repetition starts from a fresh copy of
the text.  After a warm-up, alternating in one process: copy, the mask at --t between two HIP events on its stream,
kid_sample_kernel_time_device of classifying the masked batch; copy, the same figure for the untouched text.  The device
form splits no line: one lane per read.  The first --check reads are compared with the Python model
(tests/low_complexity_model.py) byte for byte, and the counter with what the text shows.
Bytes the kernel needs: one read of every base, one byte store per masked base.  Output: stdout, and with --out a copy
under that directory (profiles/lowc/)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402
from low_complexity_model import mask_reads  # noqa: E402

RUN_AT, RUN_LEN = 55, 40


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--log2-slots", type=int, default=30)
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--t", type=int, default=20)
    ap.add_argument("--every", type=int, default=10, help="one read in this many carries a repeat")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--check", type=int, default=3000, help="reads compared with the Python model")
    ap.add_argument("--out", default=None, help="directory that receives lowc_kernel.txt")
    a = ap.parse_args()
    device = torch.device("cuda", 0)
    n, L = 2 * a.pairs, bench.READ_LEN
    db, parent, cum, _, _, _ = bench.build_db(device, a.scale, a.log2_slots, False)
    d = bench.gen_reads(device, cum, parent, 0, n)
    text = d[:n * L].view(n, L)
    sel = torch.arange(0, n, a.every, device=device)
    j = torch.arange(RUN_LEN, device=device)
    runs = torch.stack([torch.tensor(list(p), dtype=torch.uint8, device=device)[j % len(p)] for p in (b"A", b"CA", b"GAT")])
    text[sel, RUN_AT:RUN_AT + RUN_LEN] = runs[(sel // a.every) % 3]
    orig = d.clone()
    off = torch.arange(n + 1, dtype=torch.int64, device=device) * L
    counter = torch.zeros(1, dtype=torch.int64, device=device)
    s_plain, s_masked = db.sample(), db.sample()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.calls)]
    for i in range(a.warmup + a.calls):
        if i == a.warmup:
            torch.cuda.synchronize()
            s_plain.kernel_time_device()
            s_masked.kernel_time_device()
        d.copy_(orig)
        if i >= a.warmup:
            ev[i - a.warmup][0].record()
        db.mask_low_complexity_device(d.data_ptr(), off.data_ptr(), n, a.t, counter.data_ptr())
        if i >= a.warmup:
            ev[i - a.warmup][1].record()
        s_masked.classify_device(d.data_ptr(), n * L, off.data_ptr(), n)
        if i == 0:
            masked = d[:n * L].clone()
        torch.cuda.synchronize()  # (the copy below must not overtake the classify kernel's reads)
        d.copy_(orig)
        s_plain.classify_device(d.data_ptr(), n * L, off.data_ptr(), n)
        torch.cuda.synchronize()
    changed = int((masked != orig[:n * L]).sum().item())
    assert int(counter.item()) == (a.warmup + a.calls) * changed, "the counter is not the number of bytes changed"
    k = min(a.check, n)
    want, _ = mask_reads(orig[:k * L].cpu().numpy(), np.arange(k + 1, dtype=np.uint64) * L, a.t)
    assert np.array_equal(masked[:k * L].cpu().numpy(), want), "the kernel's text differs from the model's"
    with_n = int((masked.view(n, L) == ord("N")).any(dim=1).sum().item())
    times = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    mask_ms = times[len(times) // 2]
    plain_ms, nb = s_plain.kernel_time_device()
    masked_ms, nbm = s_masked.kernel_time_device()
    plain_ms, masked_ms = plain_ms / nb, masked_ms / nbm
    s_plain.close()
    s_masked.close()
    nbytes = n * L + changed
    lines = [
        "%d pairs of %d bases, scale %g, T = %d, a planted run of %d in one read of %d: %d of %d bases masked (%.2f %%), in %d reads (%.2f %%)" % (
            a.pairs, L, a.scale, a.t, RUN_LEN, a.every, changed, n * L, 100.0 * changed / (n * L), with_n, 100.0 * with_n / n),
        "lowc kernel      median %.4f ms of %d calls (min %.4f, max %.4f): %.1f GB/s of the %.3f GB it needs (text read + bytes stored), %.2f Gbases/s" % (
            mask_ms, a.calls, times[0], times[-1], nbytes / mask_ms / 1e6, nbytes / 1e9, n * L / mask_ms / 1e6),
        "classify kernel  %.4f ms per batch on the untouched text, %.4f ms on the masked text (device clock, %d batches each, alternating)" % (
            plain_ms, masked_ms, a.calls),
        "lowc / classify  %.4f (untouched text)" % (mask_ms / plain_ms),
    ]
    print("\n".join(lines))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "lowc_kernel.txt"), "w") as fh:
            fh.write("tools/low_complexity_bench.py " + " ".join(sys.argv[1:]) + "\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
