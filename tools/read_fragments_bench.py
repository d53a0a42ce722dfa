#!/usr/bin/env python3
"""What calling mate pairs as one fragment costs: the fragment kernel (kid_db_fragments_from_hits_device) next to the
support kernel (kid_db_support_from_hits_device) over the same reads, and nk10 with and without --fragments.

kernel  the bench workload: bact10-synth at --scale (1.0 = 108.6 M k-mers, 2^30 cells), 1 M pairs = 2 M 150-base reads
        resident in HBM, read 2i and read 2i + 1 taken as the mates of fragment i; the hits are found once and stay in HBM.
        Alternating in one process after a warm-up: device time per call of the fragment kernel alone
        (kid_db_read_fragments_time) and of the support kernel alone (kid_db_read_support_time), both under the rule
        --min-hits / --min-permille (2, 20).  With --dense also on reads cut from genomes the database holds: every window
        a hit, every fragment on the whole-wave path with the mate boundary inside its span.
nk10    (--nk10) one sample of --pairs pairs as FASTQ.gz, a small database (the text load is not what is measured): wall
        clock of the whole program, alternating the binaries given (default: this tree's) without and with --fragments.
A ratio is quoted beside every pair of times: times alone say little about another day's clocks."""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def measure(name, db, d_bases, n, calls, warmup, rule):
    import torch
    from read_hits_bench import READ_LEN
    dev = d_bases.device
    off = torch.arange(n + 1, dtype=torch.int64, device=dev) * READ_LEN
    d_ho = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_nk = torch.empty(n, dtype=torch.int32, device=dev)
    d_tot = torch.zeros(1, dtype=torch.int64, device=dev)
    d_sup = torch.zeros(n * 6, dtype=torch.int32, device=dev)
    d_frag = torch.zeros(n // 2 * 8, dtype=torch.int32, device=dev)
    args = (d_bases.data_ptr(), n * READ_LEN, off.data_ptr(), n, d_ho.data_ptr(), d_tot.data_ptr())
    db.read_hits_device(*args, d_n_kmers=d_nk.data_ptr())  # the sizing call
    torch.cuda.synchronize()
    total = int(d_tot.item())
    d_hits = torch.empty(max(total, 1) * 3, dtype=torch.int32, device=dev)
    db.read_hits_device(*args, d_n_kmers=d_nk.data_ptr(), d_hits=d_hits.data_ptr(), cap=total)
    torch.cuda.synchronize()
    for i in range(warmup + calls):
        if i == warmup:
            torch.cuda.synchronize()
            db.read_support_time()
            db.read_fragments_time()
        db.support_from_hits_device(d_ho.data_ptr(), d_hits.data_ptr(), d_nk.data_ptr(), n, d_sup.data_ptr(), min_hits=rule[0],
                                    min_permille=rule[1])
        db.fragments_from_hits_device(d_ho.data_ptr(), d_hits.data_ptr(), d_nk.data_ptr(), n, d_frag.data_ptr(), min_hits=rule[0],
                                      min_permille=rule[1])
    sup_ms, sup_calls, _ = db.read_support_time()
    frag_ms, frag_calls, _ = db.read_fragments_time()
    torch.cuda.synchronize()
    # the two kernels saw the same hits, or no figure below means anything: the per-mate folds are the reads' own finals
    sup, frag = d_sup.view(n, 6), d_frag.view(n // 2, 8)
    assert torch.equal(frag[:, 6], sup[0::2, 0]) and torch.equal(frag[:, 7], sup[1::2, 0])
    per = frag[:, 3].to(torch.int64)
    assert int(per.sum().item()) == total
    wave = int((per > 8).sum().item())
    split = int(((per > 8) & (sup[0::2, 3] > 0) & (sup[1::2, 3] > 0)).sum().item())
    print("%-7s %d fragments of %d reads, %d hits (%.2f per fragment); %d fragments on the whole-wave path, %d of them with hits in both mates; "
          "rule (%d, %d): %d fragments called, %d confident" % (name, n // 2, n, total, 2.0 * total / n, wave, split, rule[0], rule[1],
                                                                 int((frag[:, 0] > 0).sum().item()), int((frag[:, 1] > 0).sum().item())))
    s, f = sup_ms / sup_calls, frag_ms / frag_calls
    print("%-7s fragment kernel %.4f ms per call (%d calls) | support kernel over the same %d reads %.4f ms | fragment / support %.3f | "
          "bytes it must move %.1f MB (offsets, n_kmers, hits, records) -> %.1f GB/s" % (
              name, f, frag_calls, n, s, f / s, (12.0 * total + 12.0 * n + 16.0 * n) / 1e6, (12.0 * total + 28.0 * n) / f / 1e6))


def kernel_part(a):
    import torch
    import bench
    from kmer_id_amd import KmerDB
    from read_hits_bench import READ_LEN, genome_db
    rule = (a.min_hits, a.min_permille)
    device = torch.device("cuda", 0)
    n = 2 * a.pairs
    db, parent, cum, _, _, _ = bench.build_db(device, a.scale, a.log2_slots, False)
    d = bench.gen_reads(device, cum, parent, 0, n)
    measure("metric", db, d, n, a.calls, a.warmup, rule)
    db.close()
    del d
    if not a.dense:
        return
    rng = np.random.default_rng(3)
    G, keys, targets = genome_db(parent, bench.K, rng, 400, 20000)
    db = KmerDB(keys, targets, parent, k=bench.K, log2_slots=26)
    gi = rng.integers(0, G.shape[0], n)
    pos = rng.integers(0, G.shape[1] - READ_LEN + 1, n)
    bases = G[gi[:, None], pos[:, None] + np.arange(READ_LEN)[None, :]]
    d = torch.from_numpy(np.concatenate([np.ascontiguousarray(bases).reshape(-1), np.zeros(64, np.uint8)])).cuda()
    measure("dense", db, d, n, max(a.calls // 5, 3), a.warmup, rule)
    db.close()


def nk10_part(a):
    from kmer_id_amd import _build, synth
    binaries = [os.path.abspath(b) for b in a.binaries] or [_build.build_cli()]
    P, L, K = a.pairs, 150, 30
    cwd = tempfile.mkdtemp(prefix="frag_")
    parent, cnt = synth.load_taxonomy("bact10")
    cum = synth.cumulative(synth.scaled_counts(cnt, 0.01))
    keys, targets = synth.db_keys(cum, K)
    os.makedirs(os.path.join(cwd, "bact10"))
    with open(os.path.join(cwd, "bact10", "btree_10.txt"), "w") as fh:
        for y, x in enumerate(parent.tolist()):
            if y >= 2 and x != 1:
                fh.write("%d\t%d\n" % (x, y))
    open(os.path.join(cwd, "bact10", "bData10.txt"), "w").write("4\tX\n")
    synth.write_probes_gz(os.path.join(cwd, "bact10", "probes10.txt.gz"), keys, targets, K)
    fq, empty = os.path.join(cwd, "fq") + "/", os.path.join(cwd, "empty") + "/"
    os.makedirs(fq)
    os.makedirs(empty)
    t0 = time.time()
    for mate in (1, 2):
        r0 = (mate - 1) * P
        synth.write_fastq_gz(fq + "S0_R%d_tr.fastq.gz" % mate, synth.reads(cum, parent, P, L, K, r0=r0), synth.qualities(P, L, r0=r0), L, mate=mate)
    print("nk10    inputs generated in %.0f s: 1 sample of %d pairs" % (time.time() - t0, P), flush=True)
    cache = os.path.join(cwd, "db.kidx")

    def run(nk10, d, extra):
        t = time.time()
        subprocess.run([nk10, d, "--log2-slots", "24", "--db-cache", cache, "--threads", str(a.threads)] + extra, cwd=cwd, check=True,
                       stdout=subprocess.DEVNULL)
        return time.time() - t

    run(binaries[-1], empty, [])  # writes the cache
    run(binaries[-1], fq, ["--fragments"])  # warm-up: the file cache and the device
    ways = [(b, []) for b in binaries] + [(binaries[-1], ["--fragments"])]
    times = {i: [] for i in range(len(ways))}
    for r in range(a.repeats):
        for i in (range(len(ways)) if r % 2 == 0 else reversed(range(len(ways)))):  # (who goes first takes turns)
            times[i].append(run(ways[i][0], fq, ways[i][1]))
    ref = min(times[0])
    for i, (b, extra) in enumerate(ways):
        print("nk10    %s %s: %s s wall (min %.3f) -> min / min of the first line %.3f, %.2f M pairs/s" % (
            b, " ".join(extra) or "(no side option)", " ".join("%.3f" % t for t in times[i]), min(times[i]), min(times[i]) / ref, P / min(times[i]) / 1e6),
            flush=True)
    fragments = open(fq + "S0_fragments.txt").read().splitlines()
    result = open(fq + "S0_result.txt").read().splitlines()
    assert sum(int(l.split(",")[1]) for l in fragments) <= P and [l.split(",")[2] for l in fragments] == [l.split(",")[2] for l in result]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--log2-slots", type=int, default=30)
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--min-hits", type=int, default=2)
    ap.add_argument("--min-permille", type=int, default=20)
    ap.add_argument("--dense", action="store_true")
    ap.add_argument("--nk10", action="store_true", help="the front-end part instead of the kernel part")
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("binaries", nargs="*", help="nk10 binaries to run without the option first (e.g. the parent commit's)")
    a = ap.parse_args()
    nk10_part(a) if a.nk10 else kernel_part(a)


if __name__ == "__main__":
    main()
