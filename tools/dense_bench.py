#!/usr/bin/env python3
"""Development aid: classify-kernel time on reads whose every k-mer is in the DB (the lookup queue and
the resolver are the hot path then), next to reads of the same DB without any hit."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from kmer_id_amd import KmerDB, synth  # noqa: E402
from test_gpu_parity import _genome_db, K  # noqa: E402

read_len, n = 150, 2_000_000
parent, _ = synth.load_taxonomy("bact10")
rng = np.random.default_rng(3)
genomes, keys, targets = _genome_db(parent, 400, 20000, rng)
db = KmerDB(keys, targets, parent, k=K, log2_slots=int(os.environ.get("LOG2", "26")))
G = np.stack(genomes)
# DENSE_FRACS: the shares of reads cut from the genomes (the database holds the genomes' forward k-mers: about 60 hits per
# such read), e.g. 0.25,1.0 for 15 and 60 hits per read; LINE_DIGEST: KID_OPT_LINE_DIGEST for the samples (unset: the
# library's default, and nothing is asked of a library without it); DENSE_LAUNCHES: launches per case (6); DENSE_SYNC=1:
# the host waits for every launch, as a caller that reads its results does -- only then does it see what a pass over
# the hit log found while the case still runs
n_launch = int(os.environ.get("DENSE_LAUNCHES", "6"))
cases = (("no hits", 0.0), ("25 % of the reads from the genomes", 0.25), ("all reads from the genomes", 1.0))
if os.environ.get("DENSE_FRACS"):
    cases = tuple(("%.1f %% of the reads from the genomes" % (100 * float(f)), float(f)) for f in os.environ["DENSE_FRACS"].split(","))
for name, frac in cases:
    gi = rng.integers(0, G.shape[0], n); pos = rng.integers(0, G.shape[1] - read_len + 1, n)
    idx = pos[:, None] + np.arange(read_len)[None, :]
    bases = G[gi[:, None], idx]
    rnd = rng.random(n) >= frac
    bases[rnd] = rng.choice(np.frombuffer(b"ACGT", np.uint8), (int(rnd.sum()), read_len))
    d = torch.from_numpy(np.ascontiguousarray(bases).reshape(-1)).cuda()
    s = db.sample(); s.set_timing(True)
    if os.environ.get("LINE_DIGEST"):
        from kmer_id_amd import KID_OPT_LINE_DIGEST
        s.set_option(KID_OPT_LINE_DIGEST, int(os.environ["LINE_DIGEST"]))
    for _ in range(n_launch):
        s.classify_fixed_device(d.data_ptr(), read_len, n)
        if os.environ.get("DENSE_SYNC"):
            torch.cuda.synchronize()
    ms, launches = s.kernel_time()
    st = s.stats()
    print("%-40s %.3f ms per 2 M reads, %.1f G lookups/s, hits per read %.1f, cells per lookup %.3f" % (name, ms / launches, st["lookups"] / n_launch / (ms / launches) / 1e6, st["hits"] / st["reads"], st["probes"] / st["lookups"]))
    s.close()
