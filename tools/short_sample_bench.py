#!/usr/bin/env python3
"""The short run, launch by launch: what `bench.py --steps K --warmup W` does (build, four resident batches, db.sample(),
W warm-up steps, reset, K steps, end()), with the HIP-event time of EVERY launch (kid_sample_kernel_times), the wall
time of db.sample() and the wall time of end() alone (behind a synchronise).

   python tools/short_sample_bench.py [--steps 20] [--warmup 5] [--series plain,a,b,c] [--out FILE]

One process, one database; the series run in the order given:
   plain  the sample opened right behind the build and the batches, as bench.py has it
   a      a new sample, opened and left unused for 50 ms of host sleep before its first step
   b      a second sample on the same database after the one before was destroyed: nothing is built in front of it
   c      30 launches on a throw-away sample first (the warm case)
Timing is on from the first warm-up launch (bench.py switches it on behind the warm-up), so every launch of a series
has an event pair around it.  One JSON line per series on stdout."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (its build_db / gen_reads: the same database and reads)


def series(db, batches, n_reads, device, steps, warmup, sleep_ms=0.0):
    stream = torch.cuda.current_stream(device)
    out_final = torch.empty(n_reads, dtype=torch.int32, device=device)
    torch.cuda.synchronize(device)
    t = time.perf_counter()
    sample = db.sample()
    torch.cuda.synchronize(device)
    open_ms = (time.perf_counter() - t) * 1e3
    sample.set_timing(True)
    if sleep_ms:
        time.sleep(sleep_ms / 1e3)

    def step(i):
        sample.classify_fixed_device(batches[i % len(batches)].data_ptr(), bench.READ_LEN, n_reads, d_out=out_final.data_ptr(),
                                     stream=stream.cuda_stream)
    for i in range(warmup):
        step(i)
    torch.cuda.synchronize(device)
    sample.reset()
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    for i in range(steps):
        step(i)
    g, u = sample.end()
    torch.cuda.synchronize(device)
    whole_ms = (time.perf_counter() - t0) * 1e3
    ms, n = sample.kernel_times()
    assert n == steps + warmup, (n, steps, warmup)
    # end() alone: the same K launches again, everything drained first
    sample.reset()
    for i in range(steps):
        step(i)
    torch.cuda.synchronize(device)
    t1 = time.perf_counter()
    g2, u2 = sample.end()
    torch.cuda.synchronize(device)
    end_ms = (time.perf_counter() - t1) * 1e3
    assert (g == g2).all() and (u == u2).all()
    sample.close()
    kern = float(ms[warmup:].sum())
    return {"sample_open_ms": round(open_ms, 3), "end_alone_ms": round(end_ms, 3), "steps_and_end_ms": round(whole_ms, 3),
            "kernel_ms_timed_steps": round(kern, 3), "ms_per_step": round(whole_ms / steps, 4),
            "outside_kernels_ms_per_step": round((whole_ms - kern) / steps, 4), "bits_set": int(u.sum()),
            "launch_ms": [round(float(x), 4) for x in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--series", default="plain,a,b,c")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--log2-slots", type=int, default=30)
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: no HIP device is visible")
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    n_reads = 2 * args.pairs
    db, parent, cum, build_s, _, _ = bench.build_db(device, args.scale, args.log2_slots, False)
    batches = [bench.gen_reads(device, cum, parent, b * n_reads, n_reads) for b in range(4)]
    fh = open(args.out, "a") if args.out else None
    for name in args.series.split(","):
        if name == "c":
            warm = db.sample()
            for i in range(30):
                warm.classify_fixed_device(batches[i % 4].data_ptr(), bench.READ_LEN, n_reads)
            torch.cuda.synchronize(device)
            warm.close()
        r = series(db, batches, n_reads, device, args.steps, args.warmup, sleep_ms=50.0 if name == "a" else 0.0)
        line = json.dumps({"series": name, "steps": args.steps, "warmup": args.warmup, **r})
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()
    db.close()


if __name__ == "__main__":
    main()
