"""nk10 --fragment-loci W[:MAX_SPAN]: the fragment_loci file beside the result file equals, line for line, what the model of
tests/read_fragment_loci_model.py writes from the same probes (with their sites) and mate files; it does not depend on
--block-bytes, --threads, --batch-reads, --devices or --samples-in-flight; every other output is what it is without the
option; unequal mate files give absent mates and one line on stderr, once, whatever fragment options are given; a stale file
goes and a failing sample leaves none."""
import os
import subprocess

import numpy as np
import pytest

import read_fragment_loci_model as fm
import read_support_cases as sc
from helpers import K, concat_reads, oracle_db
from kmer_id_amd import read_probe_sites
from read_fragments_model import interleave
from read_hits_model import HitModel, trim_ranges
from test_cli_host import make_db_dir, nk10  # noqa: F401  (nk10: fixture)
from test_gpu_cli_fragments import mate_records, outputs, write_fastq_gz

pytestmark = pytest.mark.gpu

SAMPLES = ("S1", "S2")
OPT = ["--fragment-loci", "7:2000"]


def run(nk10, fq, cwd, extra, check=True, clean=True):  # noqa: F811
    for f in os.listdir(fq):
        if f.endswith(".txt") and clean:
            os.remove(os.path.join(fq, f))
    r = subprocess.run([nk10, fq + "/", "--log2-slots", "22"] + extra, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert not check or r.returncode == 0, r.stderr
    return r


def implanted_pairs(rng, keys, r1, r2, n):
    """n records of both files replaced by a pair that is one: mate 1 holds two probes, mate 2 one a few hundred entries on
    (the synthetic probes lie at org 0, position = their index)"""
    for i in rng.choice(min(len(r1), len(r2)), n, replace=False).tolist():
        j, d = int(rng.integers(0, keys.size - 900)), int(rng.integers(50, 800))
        s1 = sc.implanted(rng, [sc.cases.key_seq(keys[j], K), sc.cases.key_seq(keys[j + 40], K)], gap=10)
        s2 = sc.implanted(rng, [sc.cases.key_seq(keys[j + d], K)], gap=int(rng.integers(1, 40)))
        r1[i], r2[i] = (s1, b"I" * len(s1)), (s2, b"I" * len(s2))


def model_file(hm, sites, r1, r2, w, span):
    """record j of r1 with record j of r2, the surplus of the longer with an absent mate -> the fragment_loci file"""
    org, pos = sites
    n = max(len(r1), len(r2))
    per = []
    for recs in (r1, r2):
        recs = recs + [(b"", b"")] * (n - len(recs))
        start, stop, keep = trim_ranges([q for _, q in recs], [len(s) for s, _ in recs], K)
        start[~keep], stop[~keep] = 0, -1
        per.append(([s for s, _ in recs], start, stop))
    bases, off = concat_reads(interleave(per[0][0], per[1][0]))
    start, stop = np.zeros(2 * n, np.int32), np.zeros(2 * n, np.int32)
    start[0::2], start[1::2], stop[0::2], stop[1::2] = per[0][1], per[1][1], per[0][2], per[1][2]
    recs = fm.batch(hm.batch(bases, off, start, stop), org, pos, K, w, span)
    lines = [fm.line(j, recs[j]) + "\n" for j in range(n) if recs["n_hits"][j]]
    return "".join(lines).encode(), recs


def test_nk10_file_equals_the_model_for_any_way_of_running(nk10, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    parent, cum, keys, targets = make_db_dir(cwd, 2e-4)
    fq = os.path.join(cwd, "fq")
    os.makedirs(fq)
    rng = np.random.default_rng(2025)
    mates = {"S1": (mate_records(cum, parent, 620, 1000, rng, 11), mate_records(cum, parent, 617, 5000, rng, 7)),  # R2 is 3 records shorter
             "S2": (mate_records(cum, parent, 600, 9000, rng, 5), mate_records(cum, parent, 600, 13000, rng, 5))}
    for p, (r1, r2) in mates.items():
        implanted_pairs(rng, keys, r1, r2, 60)
        sizes = [write_fastq_gz(os.path.join(fq, p + "_R1_tr.fastq.gz"), r1, b"\n"), write_fastq_gz(os.path.join(fq, p + "_R2_tr.fastq.gz"), r2, b"\r\n")]
        assert min(sizes) > 3 * 32768 and sizes[0] != sizes[1]  # under --block-bytes 32768 the two files are cut differently
    sites = read_probe_sites(os.path.join(cwd, "bact10", "probes10.txt.gz"))
    hm = HitModel(oracle_db(parent, keys, targets, 22), keys, targets, K)
    exp, exp1 = {}, {}
    for p, (r1, r2) in mates.items():
        exp[p], recs = model_file(hm, sites, r1, r2, 7, 2000)
        exp1[p], _ = model_file(hm, sites, r1, r2, 1, 1000)
        assert int((recs["mates"] == 3).sum()) >= 50 and int((recs["mates"] == 1).sum()) >= 20 and int((recs["mates"] == 2).sum()) >= 20
        assert exp[p].count(b"\n") > 300 and exp[p] != exp1[p]
    base = run(nk10, fq, cwd, [])
    plain = {s: outputs(fq, s) for s in ("_result.txt", "_reads.txt")}
    assert sorted(plain["_result.txt"]) == list(SAMPLES) and outputs(fq, "_fragment_loci.txt") == {} and b"--fragment" not in base.stderr
    for p in SAMPLES:
        open(os.path.join(fq, p + "_fragment_loci.txt"), "w").write("left by an earlier run\n")  # removed when its sample starts
    ways = [[], ["--block-bytes", "32768"], ["--block-bytes", "40000", "--threads", "2"], ["--batch-reads", "64"], ["--devices", "0,0"],
            ["--samples-in-flight", "1", "--threads", "3"]]
    for extra in ways:
        r = run(nk10, fq, cwd, OPT + extra, clean=bool(extra))  # (the first run meets the stale files)
        assert outputs(fq, "_fragment_loci.txt") == exp, extra
        # every other file and stdout are what they are without the option
        assert r.stdout == base.stdout and outputs(fq, "_result.txt") == plain["_result.txt"] and outputs(fq, "_reads.txt") == plain["_reads.txt"], extra
        # one line on stderr for the sample whose files are unequal, with both counts
        lines = [l for l in r.stderr.decode().splitlines() if "absent mate" in l]
        assert len(lines) == 1 and "--fragment-loci" in lines[0] and "S1_result.txt" in lines[0] and " 620 " in lines[0] and " 617 " in lines[0], r.stderr
    r = run(nk10, fq, cwd, ["--fragment-loci", "1", "--fragments", "--fragment-votes", "--block-bytes", "32768"])
    assert outputs(fq, "_fragment_loci.txt") == exp1  # (MAX_SPAN is 1000 when not given)
    assert len([l for l in r.stderr.decode().splitlines() if "absent mate" in l]) == 1  # once, for the three options together
    fragments = outputs(fq, "_fragments.txt"), outputs(fq, "_fragment_votes.txt")
    run(nk10, fq, cwd, ["--fragments", "--fragment-votes", "--block-bytes", "32768"])
    assert (outputs(fq, "_fragments.txt"), outputs(fq, "_fragment_votes.txt")) == fragments and sorted(fragments[0]) == list(SAMPLES)
    # the masks apply as they do to the fragments file: the file changes, and is that of the masked text whatever the blocks
    masks = ["--min-base-quality", "20", "--low-complexity", "20"]
    run(nk10, fq, cwd, OPT + masks)
    masked = outputs(fq, "_fragment_loci.txt")
    assert masked != exp and sorted(masked) == list(SAMPLES)
    run(nk10, fq, cwd, OPT + masks + ["--block-bytes", "32768", "--batch-reads", "100"])
    assert outputs(fq, "_fragment_loci.txt") == masked


def test_a_failing_sample_leaves_no_file(nk10, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    parent, cum, keys, targets = make_db_dir(cwd, 2e-5)
    fq = os.path.join(cwd, "fq")
    os.makedirs(fq)
    write_fastq_gz(os.path.join(fq, "S1_R1_tr.fastq.gz"), mate_records(cum, parent, 50, 1000, np.random.default_rng(1), 9), b"\n")  # no R2 file
    open(os.path.join(fq, "S1_fragment_loci.txt"), "w").write("left by an earlier run\n")
    r = run(nk10, fq, cwd, ["--fragment-loci", "1"], check=False, clean=False)
    assert r.returncode == 255 and not os.path.exists(os.path.join(fq, "S1_fragment_loci.txt"))
