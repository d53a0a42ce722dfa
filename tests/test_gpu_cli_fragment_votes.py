"""nk10 --fragment-votes: the fragment_votes file beside the result file equals, byte for byte, the file the model of
tests/read_fragment_votes_model.py writes from the same probes and mate files; it does not depend on --block-bytes,
--devices, --threads, --samples-in-flight or --batch-reads; it needs neither --fragments nor --votes and changes nothing
they write; the line about unequal mate files comes once; a sample that fails leaves none."""
import os
import subprocess

import numpy as np
import pytest

import test_gpu_cli_fragments as cf
from helpers import K, concat_reads, oracle_db
from read_fragment_votes_model import FragmentVoteModel
from read_fragments_model import interleave
from read_hits_model import HitModel, trim_ranges
from read_support_model import SupportModel, result_text
from read_votes_model import VoteModel
from test_cli_host import make_db_dir, nk10  # noqa: F401  (nk10: fixture)

pytestmark = pytest.mark.gpu

RULE = ["--min-hits", "2", "--confidence", "0.025"]
SAMPLES = ("S1", "S2")
SIDE = ("_fragment_votes.txt", "_fragments.txt", "_votes.txt")


def model_file(fvm, hm, targets, r1, r2, rule):
    """record j of r1 with record j of r2, the surplus of the longer with an absent mate -> the fragment_votes file, and
    how many fragments were counted"""
    n = max(len(r1), len(r2))
    per = []
    for recs in (r1, r2):
        recs = recs + [(b"", b"")] * (n - len(recs))
        start, stop, keep = trim_ranges([q for _, q in recs], [len(s) for s, _ in recs], K)
        start[~keep], stop[~keep] = 0, -1
        per.append(([s for s, _ in recs], start, stop, keep))
    bases, off = concat_reads(interleave(per[0][0], per[1][0]))
    start, stop = np.zeros(2 * n, np.int32), np.zeros(2 * n, np.int32)
    start[0::2], start[1::2], stop[0::2], stop[1::2] = per[0][1], per[1][1], per[0][2], per[1][2]
    hits = hm.batch(bases, off, start, stop)
    counted = per[0][3] | per[1][3]
    g, u = fvm.tally(hits, fvm.batch_anc(hits, rule), counted, targets)
    return result_text(g, u).encode(), int(counted.sum())


def run(nk10, fq, cwd, extra, check=True):  # noqa: F811
    for f in os.listdir(fq):
        if f.endswith(".txt") and not f.endswith(SIDE):
            os.remove(os.path.join(fq, f))
    r = subprocess.run([nk10, fq + "/", "--log2-slots", "22"] + extra, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert not check or r.returncode == 0, r.stderr
    return r


def outputs(fq, suffix):
    return {p: open(os.path.join(fq, p + suffix), "rb").read() for p in SAMPLES if os.path.exists(os.path.join(fq, p + suffix))}


def test_nk10_fragment_votes_file_equals_the_model_for_any_way_of_running(nk10, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    parent, cum, keys, targets = make_db_dir(cwd, 2e-4)
    fq = os.path.join(cwd, "fq")
    os.makedirs(fq)
    rng = np.random.default_rng(2025)
    mates = {"S1": (cf.mate_records(cum, parent, 620, 1000, rng, 11), cf.mate_records(cum, parent, 617, 5000, rng, 7)),  # R2 is 3 records shorter
             "S2": (cf.mate_records(cum, parent, 600, 9000, rng, 5), cf.mate_records(cum, parent, 600, 13000, rng, 5))}
    for p, (r1, r2) in mates.items():
        sizes = [cf.write_fastq_gz(os.path.join(fq, p + "_R1_tr.fastq.gz"), r1, b"\n"),
                 cf.write_fastq_gz(os.path.join(fq, p + "_R2_tr.fastq.gz"), r2, b"\r\n")]
        assert min(sizes) > 3 * 32768  # under --block-bytes 32768 each mate file spans at least three blocks
    hm = HitModel(oracle_db(parent, keys, targets, 22), keys, targets, K)
    fvm = FragmentVoteModel(VoteModel(SupportModel(hm, parent)))
    exp, exp_rule = {}, {}
    for p, (r1, r2) in mates.items():
        exp[p], counted = model_file(fvm, hm, targets, r1, r2, (0, 0))
        exp_rule[p], _ = model_file(fvm, hm, targets, r1, r2, (2, 25))
        assert max(len(r1), len(r2)) // 2 < counted < max(len(r1), len(r2)) and exp[p] != exp_rule[p]
    base = run(nk10, fq, cwd, [])
    plain = {s: outputs(fq, s) for s in ("_result.txt", "_reads.txt")}
    assert sorted(plain["_result.txt"]) == list(SAMPLES) and all(outputs(fq, s) == {} for s in SIDE) and b"--fragment" not in base.stderr
    for p in SAMPLES:
        open(os.path.join(fq, p + "_fragment_votes.txt"), "w").write("left by an earlier run\n")
    ways = [[], ["--block-bytes", "32768"], ["--devices", "0,0"], ["--threads", "2"], ["--samples-in-flight", "1"], ["--batch-reads", "64"]]
    for extra in ways:
        for rule, want in (([], exp), (RULE, exp_rule)) if extra in ways[:2] else (([], exp),):
            r = run(nk10, fq, cwd, ["--fragment-votes"] + rule + extra)
            assert outputs(fq, "_fragment_votes.txt") == want, (extra, rule)
            # it needs neither --fragments nor --votes and writes neither file; every other file and stdout are what they are without it
            assert outputs(fq, "_fragments.txt") == {} and outputs(fq, "_votes.txt") == {}
            assert r.stdout == base.stdout and outputs(fq, "_result.txt") == plain["_result.txt"] and outputs(fq, "_reads.txt") == plain["_reads.txt"], extra
            lines = [l for l in r.stderr.decode().splitlines() if "absent mate" in l]
            assert len(lines) == 1 and "--fragment-votes" in lines[0] and "S1_result.txt" in lines[0] and " 620 " in lines[0] and " 617 " in lines[0], r.stderr
            if not rule:  # under no rule the unique k-mers are those of the result file
                for p in SAMPLES:
                    col3 = lambda text: [l.split(b",")[2] for l in text.splitlines()]  # noqa: E731
                    assert col3(want[p]) == col3(plain["_result.txt"][p])
    # beside --fragments and --votes: their files, the result and reads files and stdout are what the same run gives
    # without --fragment-votes, and the line about the unequal mate files comes once
    for rule, want in (([], exp), (RULE, exp_rule)):
        without = run(nk10, fq, cwd, ["--fragments", "--votes"] + rule)
        ref = {s: outputs(fq, s) for s in ("_fragments.txt", "_votes.txt", "_result.txt", "_reads.txt")}
        assert all(sorted(ref[s]) == list(SAMPLES) for s in ref)
        for p in SAMPLES:
            os.remove(os.path.join(fq, p + "_fragments.txt"))
            os.remove(os.path.join(fq, p + "_votes.txt"))
        r = run(nk10, fq, cwd, ["--fragments", "--votes", "--fragment-votes"] + rule)
        assert {s: outputs(fq, s) for s in ref} == ref and r.stdout == without.stdout == base.stdout, rule
        assert outputs(fq, "_fragment_votes.txt") == want, rule
        about = lambda run_: [l for l in run_.stderr.decode().splitlines() if "absent mate" in l]  # noqa: E731
        assert about(r) == about(without) and len(about(r)) == 1 and "--fragments:" in about(r)[0], r.stderr
        for p in SAMPLES:
            os.remove(os.path.join(fq, p + "_fragments.txt"))
            os.remove(os.path.join(fq, p + "_votes.txt"))


def test_a_failing_sample_leaves_no_fragment_votes_file(nk10, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    parent, cum, keys, targets = make_db_dir(cwd, 2e-5)
    fq = os.path.join(cwd, "fq")
    os.makedirs(fq)
    cf.write_fastq_gz(os.path.join(fq, "S1_R1_tr.fastq.gz"), cf.mate_records(cum, parent, 50, 1000, np.random.default_rng(1), 9), b"\n")  # no R2 file
    open(os.path.join(fq, "S1_fragment_votes.txt"), "w").write("left by an earlier run\n")
    r = run(nk10, fq, cwd, ["--fragment-votes"], check=False)
    assert r.returncode == 255 and not os.path.exists(os.path.join(fq, "S1_fragment_votes.txt"))
