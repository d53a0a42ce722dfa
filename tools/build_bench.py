"""kmer_build_vf6 on a seeded synthetic genome set: one JSON line with the per-phase device time (HIP events), the
k-mer rates, the host read/inflate seconds, the wall time, the table's `size` and the probe count.

    python tools/build_bench.py [--gbases 2.0] [--org-mbases 5] [--log2-cells 35] [--workdir DIR] [--keep]

The set: --gbases of ingroup genomes of --org-mbases each, mutated down a 15-node tree (1 % per edge, 0.3 % per
genome), plus 4 outgroups, written as .fasta.gz by 16 worker processes.  The program runs at the reference's table
size by default (2^35 cells, 128 GiB of device memory).
"""
import argparse
import gzip
import json
import multiprocessing as mp
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EDGES = [(1, 2), (1, 3), (2, 4), (2, 5), (3, 6), (3, 7), (4, 8), (4, 9), (5, 10), (5, 11), (6, 12), (6, 13), (7, 14), (7, 15)]
LEAVES = list(range(8, 16))
ACGT = np.frombuffer(b"ACGT", np.uint8)


def mutate(rng, g, rate):
    g = g.copy()
    m = rng.random(g.size) < rate
    g[m] = rng.integers(0, 4, int(m.sum()), dtype=np.uint8)
    return g


def node_genome(seed, length, node):
    """a node's genome: the root mutated along the tree path (deterministic per node)"""
    path = [node]
    par = {c: p for p, c in EDGES}
    while path[-1] in par:
        path.append(par[path[-1]])
    g = np.random.default_rng(seed).integers(0, 4, length, dtype=np.uint8)
    for v in reversed(path[:-1]):
        g = mutate(np.random.default_rng(seed * 1000 + v), g, 0.01)
    return g


def write_org(args):
    seed, length, node, o, path = args
    g = mutate(np.random.default_rng(seed * 7919 + o), node_genome(seed, length, node), 0.003)
    s = ACGT[g].tobytes()
    body = b"\n".join(s[i:i + 80] for i in range(0, len(s), 80))
    with open(path, "wb") as f:
        f.write(gzip.compress(b">org%d\n" % o + body + b"\n", 1))
    return len(s)


def make_set(d, gbases, org_mbases, seed):
    os.makedirs(os.path.join(d, "bb", "fa"), exist_ok=True)
    length = int(org_mbases * 1e6)
    n = max(1, int(gbases * 1e9 // length))
    jobs, data = [], []
    for o in range(n):
        t = LEAVES[o % len(LEAVES)]
        acc = "B%05d" % o
        jobs.append((seed, length, t, o, os.path.join(d, "bb", "fa", acc + ".fasta.gz")))
        data.append((t, acc))
    outs = []
    for j in range(4):  # outgroups: random genomes of the same size
        acc = "OUT%d" % j
        jobs.append((seed + 100 + j, length, 1, n + j, os.path.join(d, "bb", "fa", acc + ".fasta.gz")))
        outs.append(acc)
    with mp.Pool(16) as pool:
        total = sum(pool.map(write_org, jobs))
    open(os.path.join(d, "bb", "bb_data.txt"), "w").write("".join("%d %s\n" % x for x in data))
    open(os.path.join(d, "bb", "bb_tree.txt"), "w").write("".join("%d %d\n" % e for e in EDGES))
    open(os.path.join(d, "bb", "bb_filter.txt"), "w").write("".join(a + "\n" for a in outs))
    return total, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gbases", type=float, default=2.0)
    ap.add_argument("--org-mbases", type=float, default=5.0)
    ap.add_argument("--log2-cells", type=int, default=35)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--keep", action="store_true")
    a = ap.parse_args()
    from kmer_id_amd import _build
    d = a.workdir or tempfile.mkdtemp(prefix="build_bench_")
    t0 = time.time()
    total, n = make_set(d, a.gbases, a.org_mbases, a.seed)
    gen_s = time.time() - t0
    t0 = time.time()
    r = subprocess.run([_build.cli_path("kmer_build_vf6"), "-name", "bb", "-fadir", "bb/fa/", "--genbank-dir", "none/", "--log2-cells",
                        str(a.log2_cells), "--timing"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    wall = time.time() - t0
    if r.returncode != 0:
        sys.stderr.write(r.stderr.decode())
        sys.exit(r.returncode)
    t = json.loads(r.stderr.decode().strip().splitlines()[-1])
    res = {"workload": "kmer_build_vf6", "log2_cells": a.log2_cells, "orgs": n, "bases_total": total, "generate_s": round(gen_s, 2),
           "add_ms": t["add_ms"], "remove_ms": t["remove_ms"], "claim_ms": t["claim_ms"],
           "add_gkmer_s": round(t["add_bases"] / t["add_ms"] / 1e6, 3) if t["add_ms"] else None,
           "remove_gkmer_s": round(t["remove_bases"] / t["remove_ms"] / 1e6, 3) if t["remove_ms"] else None,
           "claim_gkmer_s": round(t["claim_bases"] / t["claim_ms"] / 1e6, 3) if t["claim_ms"] else None,
           "read_s": t["read_s"], "program_wall_s": t["wall_s"], "wall_s": round(wall, 3), "size": t["size"], "probes": t["probes"]}
    print(json.dumps(res))
    if not a.keep and not a.workdir:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
