"""--segment-votes LEN[:STEP] of the three front-ends: the segment_votes file beside the result file equals, byte for
byte, the file the model of tests/read_segment_votes_model.py writes from the same probes and reads; it does not depend
on --batch-reads, --threads, --devices or --block-bytes; with --segments as well, under another geometry, the segments
file is what it is without; every other output is what it is without the option; a stale file goes and a sample that
fails leaves none."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from helpers import K, concat_reads, ob, oracle_db
from read_hits_model import HitModel
from read_segment_votes_model import SegmentVoteModel, segment_votes_line
from read_support_model import SupportModel
from test_cli_host import make_db_dir, nk10  # noqa: F401  (nk10: fixture)
from test_cli_vf6_m3 import bins, parse_dump, setup_m3, setup_vf6  # noqa: F401  (bins: fixture)
from test_gpu_cli_hits import fastq_reads, probes_of, stage_small
from test_gpu_cli_segments import run_dir

pytestmark = pytest.mark.gpu


def model_file(odb, keys, targets, parent, reads, seg, rule, u_is_t=False):
    """reads: [(header, start, stop, sequence)] in the reference's order, each one handed to process_read"""
    sm = SupportModel(HitModel(odb, keys, targets, K, u_is_t=u_is_t), parent)
    bases, off = concat_reads([r[3] for r in reads])
    start = np.array([r[1] for r in reads], np.int32)
    stop = np.array([r[2] for r in reads], np.int32)
    so, rec = SegmentVoteModel(sm, bases, off, start, stop).direct(seg[0], seg[1], rule)
    final = ob.OracleSample(odb).classify(bases, off, start, stop)
    return b"".join(segment_votes_line(int(final[r]), sp - st + 1, rec[int(so[r]):int(so[r + 1])], acc) for r, (acc, st, sp, _) in enumerate(reads))


def test_nk10_file_equals_the_model_for_any_way_of_running(nk10, gold_dir, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    src, fq, parent = stage_small(gold_dir, cwd)
    keys, targets = probes_of(os.path.join(cwd, "bact10", "probes10.txt.gz"))
    odb = oracle_db(parent, keys, targets, 22)
    samples = ("S1", "S2")
    reads = {p: fastq_reads(os.path.join(fq, p + "_R1_tr.fastq.gz")) + fastq_reads(os.path.join(fq, p + "_R2_tr.fastq.gz")) for p in samples}
    seg = (40, 20)
    exp00 = {p: model_file(odb, keys, targets, parent, reads[p], seg, (0, 0)) for p in reads}
    exp = {p: model_file(odb, keys, targets, parent, reads[p], seg, (2, 20)) for p in reads}
    assert all(e.count(b"\n") > 50 for e in exp.values()) and exp != exp00
    cols = [c.split(b":") for e in exp00.values() for l in e.splitlines() for c in l.split(b"\t")[4].split(b" ")]
    assert all(len(c) == 8 and c[4] == c[5] for c in cols)  # without a rule confident = call
    rule = ["--min-hits", "2", "--confidence", "0.02"]
    # the runs without the option: alone, and with --segments under another geometry
    base_out, base = run_dir(nk10, fq, cwd, ["--hits", "--segments", "64:16"] + rule)
    assert sorted(base) == sorted(p + s for p in samples for s in ("_confident.txt", "_hits.txt", "_reads.txt", "_result.txt", "_segments.txt"))
    for p in samples:  # a file an earlier run left is removed when its sample starts
        open(os.path.join(fq, p + "_segment_votes.txt"), "w").write("left by an earlier run\n")
    opt = ["--segment-votes", "40:20"]
    for extra in ([], ["--batch-reads", "7"], ["--batch-reads", "53", "--devices", "0,0"], ["--threads", "1", "--samples-in-flight", "1"],
                  ["--block-bytes", "32768", "--threads", "3"]):
        out, got = run_dir(nk10, fq, cwd, ["--hits", "--segments", "64:16"] + rule + opt + extra, clean=bool(extra))  # (the first run meets the stale files)
        assert out == base_out, extra
        for p in samples:
            assert got.pop(p + "_segment_votes.txt") == exp[p], (extra, p)
        assert got == base, extra  # every other output, the segments file included, is byte for byte what it is without the option
    out, got = run_dir(nk10, fq, cwd, opt)
    assert {p: got[p + "_segment_votes.txt"] for p in samples} == exp00 and sorted(got) == sorted(
        p + s for p in samples for s in ("_reads.txt", "_result.txt", "_segment_votes.txt"))
    plain_out, plain = run_dir(nk10, fq, cwd, [])
    assert sorted(plain) == sorted(p + s for p in samples for s in ("_reads.txt", "_result.txt"))
    assert all(got[f] == plain[f] for f in plain) and out == plain_out


def test_nk10_failing_sample_leaves_no_file(nk10, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    make_db_dir(cwd, 2e-5)
    fq = os.path.join(cwd, "fq"); os.makedirs(fq)
    with gzip.open(os.path.join(fq, "L_R1_tr.fastq.gz"), "wb") as fh:
        fh.write(b"@a\n" + b"ACGT" * 10 + b"\n+\n" + b"I" * 39 + b"\n")  # a quality line shorter than its sequence
    with gzip.open(os.path.join(fq, "L_R2_tr.fastq.gz"), "wb") as fh:
        fh.write(b"@b\nACGT\n+\nIIII\n")
    open(os.path.join(fq, "L_segment_votes.txt"), "w").write("left by an earlier run\n")
    r = subprocess.run([nk10, fq + "/", "--log2-slots", "16", "--segment-votes", "10"], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 134, (r.returncode, r.stderr[-500:])
    assert b"quality line shorter than the sequence" in r.stderr
    assert not os.path.exists(os.path.join(fq, "L_segment_votes.txt")) and not os.path.exists(os.path.join(fq, "L_result.txt"))


def test_vf6_file_equals_the_model(bins, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    src, params = setup_vf6(cwd)
    prog = bins["kmer_read_vf6"]
    dump = os.path.join(cwd, "dry.txt")
    subprocess.run([prog, "-name", "DB", "-jname", "J", "--dry-run", dump], cwd=cwd, check=True, stdout=subprocess.PIPE)
    par, _, _, files = parse_dump(dump)
    keys, targets = probes_of(os.path.join(cwd, "DB", "DB_probes.txt.gz"))
    odb = oracle_db(par, keys, targets, 22, flags=ob.KO_FLAG_U_IS_T)
    exp = {"jobA": model_file(odb, keys, targets, par, files[0][1] + files[1][1], (50, 25), (0, 0), u_is_t=True),
           "jobB": model_file(odb, keys, targets, par, files[2][1] + files[3][1], (50, 25), (0, 0), u_is_t=True)}
    assert all(e.count(b"\n") > 5 for e in exp.values())
    jdir = os.path.join(cwd, "J")
    run = [prog, "-name", "DB", "-jname", "J", "--log2-slots", "22", "--batch-reads", "37"]
    plain = subprocess.run(run, cwd=cwd, check=True, stdout=subprocess.PIPE).stdout
    before = {f: open(os.path.join(jdir, f), "rb").read() for f in os.listdir(jdir)}
    open(os.path.join(jdir, "jobA_segment_votes.txt"), "w").write("left by an earlier run\n")
    r = subprocess.run(run + ["--segment-votes", "50:25"], cwd=cwd, check=True, stdout=subprocess.PIPE)
    after = {f: open(os.path.join(jdir, f), "rb").read() for f in os.listdir(jdir)}
    got = {job: after.pop(job + "_segment_votes.txt") for job in exp}
    assert r.stdout == plain and after == before and got == exp


def test_m3_runs_once(bins, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    src, params, wd = setup_m3(cwd)
    keys, targets = probes_of(wd + "mitochondria_probes.txt.gz")
    tag, (f1, f2) = sorted(params["runs"].items())[0]
    files_args = ["-wdir", wd, "-f1", wd + f1, "-f2", (wd + f2) if f2 != "none" else "none"]
    dump = os.path.join(cwd, "dry.txt")
    subprocess.run([bins["kmer_read_m3"]] + files_args + ["--dry-run", dump], cwd=cwd, check=True, stdout=subprocess.PIPE)
    par, _, _, files = parse_dump(dump)
    odb = oracle_db(par, keys, targets, params["log2_slots"], max_probes=16)
    exp = model_file(odb, keys, targets, par, [r for f in files for r in f[1]], (50, 25), (2, 0))
    assert exp.count(b"\n") > 5
    open(wd + "segment_votes.txt", "w").write("left by an earlier run\n")
    subprocess.run([bins["kmer_read_m3"]] + files_args + ["--log2-slots", str(params["log2_slots"]), "--batch-reads", "53", "--segment-votes", "50:25",
                                                          "--min-hits", "2"], cwd=cwd, check=True, stdout=subprocess.PIPE)
    assert open(wd + "segment_votes.txt", "rb").read() == exp
