"""--seen of the three front-ends and kmer_shared on their files: the seen file beside a result file has the right
header, its bits per target (the model of tests/shared_kmers_model.py over the probes) are column 3 of the result file,
or of the confident file under a rule; it does not depend on --batch-reads, --devices or --samples-in-flight; every other
file and stdout are what they are without the option; a sample that fails leaves none; kmer_shared prints exactly the
lines the model gives."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import shared_kmers_model as sm
from kmer_id_amd import _build, read_seen_file, synth
from test_cli_host import make_db_dir, nk10  # noqa: F401  (fixture)
from test_cli_vf6_m3 import bins, m3_reference_result, setup_m3, setup_vf6  # noqa: F401  (bins: fixture)
from test_gpu_cli_hits import probes_of, run_small, stage_small

pytestmark = pytest.mark.gpu

RULE = ["--min-hits", "2"]


def column3(path):
    return np.array([int(line.split(b",")[2]) for line in open(path, "rb").read().splitlines()], np.int64)


def seen_of(path, keys, ntar, k=30):
    """a seen file, its header checked against the database -> (raw bytes, bitmap)"""
    bitmap, n_entries, file_ntar, file_k = read_seen_file(path)
    assert (n_entries, file_ntar, file_k) == (keys.size, ntar, k) and bitmap.size == sm.seen_bytes(keys.size), path
    return open(path, "rb").read(), bitmap


def bits_per_target(bitmap, targets, ntar):
    return sm.shared(targets, ntar, [bitmap])[0, 0]


def seen_files(top):
    return sorted(f for _, _, fs in os.walk(top) for f in fs if "seen" in f)


def test_nk10_seen_files_and_kmer_shared(nk10, gold_dir, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    src, fq, parent = stage_small(gold_dir, cwd)
    probes = os.path.join(cwd, "bact10", "probes10.txt.gz")
    keys, targets = probes_of(probes)
    ntar = parent.size
    assert run_small(nk10, src, fq, cwd, []) == {} and seen_files(fq) == []  # without the option: the goldens, no seen file
    for p in ("S1", "S2"):
        open(os.path.join(fq, p + "_seen.bin"), "w").write("left by an earlier run\n")
    seen = {}
    for extra in ([], ["--batch-reads", "64"], ["--devices", "0,0"], ["--samples-in-flight", "2"]):
        run_small(nk10, src, fq, cwd, ["--seen"] + extra)  # (_result.txt, _reads.txt and stdout against the goldens)
        assert seen_files(fq) == ["S1_seen.bin", "S2_seen.bin"], extra
        for p in ("S1", "S2"):
            raw, bitmap = seen_of(os.path.join(fq, p + "_seen.bin"), keys, ntar)
            assert seen.setdefault(p, (raw, bitmap))[0] == raw, (extra, p)
    for p in ("S1", "S2"):
        bits = bits_per_target(seen[p][1], targets, ntar)
        assert np.array_equal(bits, column3(os.path.join(src, p + "_result.txt"))) and bits.sum() > 0, p
    # under a rule: the bitmap of the tallied sample
    confident = {}
    for extra in ([], ["--devices", "0,0", "--batch-reads", "64"]):
        run_small(nk10, src, fq, cwd, ["--seen"] + RULE + extra)
        for p in ("S1", "S2"):
            raw, bitmap = seen_of(os.path.join(fq, p + "_seen.bin"), keys, ntar)
            assert confident.setdefault(p, (raw, bitmap))[0] == raw, (extra, p)
            assert np.array_equal(bits_per_target(bitmap, targets, ntar), column3(os.path.join(fq, p + "_confident.txt"))), (extra, p)
    assert any(confident[p][0] != seen[p][0] for p in seen)  # the rule uncalls some reads
    # ---- kmer_shared on the two files of the run without a rule, and on them with S1's file under the rule (S2 is a sample
    # of two k-mers that shares no target with S1: only the third file gives pair lines for a threshold to drop)
    _build.build_cli()
    kmer_shared = _build.cli_path("kmer_shared")
    paths, maps = [], []
    for name, (raw, bitmap) in (("S1", seen["S1"]), ("S2", seen["S2"]), ("S1_rule", confident["S1"])):
        paths.append(os.path.join(cwd, name + "_seen.bin"))
        open(paths[-1], "wb").write(raw)
        maps.append(bitmap)
    base = [kmer_shared, "--probes", probes, "--ntar", str(ntar)]
    for files in ([0, 1], [0, 1, 2]):
        fp = [paths[f] for f in files]
        matrix = sm.shared(targets, ntar, [maps[f] for f in files])
        plain, cut = sm.cli_lines(fp, matrix), sm.cli_lines(fp, matrix, 2)
        if len(files) == 3:  # the threshold drops some lines and keeps some
            assert len(files) < cut.count(b"\n") < plain.count(b"\n")
        for args, exp in (([], plain), (["--min-shared", "0"], plain), (["--min-shared", "2", "--threads", "2"], cut)):
            r = subprocess.run(base + args + fp, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            assert r.returncode == 0 and r.stdout == exp, (files, args, r.stderr)
    order = [1, 0, 1]  # a file named twice
    both = subprocess.run(base + [paths[f] for f in order], cwd=cwd, stdout=subprocess.PIPE, check=True).stdout
    assert both == sm.cli_lines([paths[f] for f in order], sm.shared(targets, ntar, [maps[f] for f in order]))
    # the probes of another database: their number is not the files'
    fewer = os.path.join(cwd, "fewer_probes.txt.gz")
    synth.write_probes_gz(fewer, keys[:-1], targets[:-1])
    r = subprocess.run([kmer_shared, "--probes", fewer, "--ntar", str(ntar)] + paths, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 3 and r.stdout == b"" and r.stderr.count(b"\n") == 1, r.stderr


@pytest.mark.parametrize("options", [["--seen"], ["--seen", "--min-hits", "2"]], ids=["seen", "seen-and-rule"])
def test_nk10_failing_sample_leaves_no_seen_file(nk10, tmp_path, options):  # noqa: F811
    cwd = str(tmp_path)
    make_db_dir(cwd, 2e-5)
    fq = os.path.join(cwd, "fq")
    os.makedirs(fq)
    with gzip.open(os.path.join(fq, "L_R1_tr.fastq.gz"), "wb") as fh:
        fh.write(b"@a\n" + b"ACGT" * 10 + b"\n+\n" + b"I" * 39 + b"\n")  # a quality line shorter than its sequence
    with gzip.open(os.path.join(fq, "L_R2_tr.fastq.gz"), "wb") as fh:
        fh.write(b"@b\nACGT\n+\nIIII\n")
    open(os.path.join(fq, "L_seen.bin"), "w").write("left by an earlier run\n")
    r = subprocess.run([nk10, fq + "/", "--log2-slots", "16"] + options, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 134, (r.returncode, r.stderr[-500:])
    assert b"quality line shorter than the sequence" in r.stderr
    assert seen_files(fq) == [] and not os.path.exists(os.path.join(fq, "L_result.txt"))


def test_vf6_seen_file_matches_its_result(bins, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    src, params = setup_vf6(cwd)
    keys, targets = probes_of(os.path.join(cwd, "DB", "DB_probes.txt.gz"))
    r = subprocess.run([bins["kmer_read_vf6"], "-name", "DB", "-jname", "J", "--log2-slots", "22", "--seen", "--devices", "0,0"], cwd=cwd,
                       check=True, stdout=subprocess.PIPE)
    assert r.stdout.decode() == open(os.path.join(src, "plain", "stdout.txt")).read()
    assert seen_files(os.path.join(cwd, "J")) == ["jobA_seen.bin", "jobB_seen.bin"]
    for job in ("jobA", "jobB"):
        result = os.path.join(cwd, "J", job + "_result.txt")
        assert open(result, "rb").read() == open(os.path.join(src, "plain", job + "_result.txt"), "rb").read()
        ntar = column3(result).size
        raw, bitmap = seen_of(os.path.join(cwd, "J", job + "_seen.bin"), keys, ntar)
        assert np.array_equal(bits_per_target(bitmap, targets, ntar), column3(result)) and column3(result).sum() > 0, job


def test_m3_seen_file_matches_its_result(bins, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    src, params, wd = setup_m3(cwd)
    keys, targets = probes_of(wd + "mitochondria_probes.txt.gz")
    tag, (f1, f2) = sorted(params["runs"].items())[0]
    files_args = ["-wdir", wd, "-f1", wd + f1, "-f2", (wd + f2) if f2 != "none" else "none"]
    subprocess.run([bins["kmer_read_m3"]] + files_args + ["--log2-slots", str(params["log2_slots"]), "--seen", "--min-hits", "2"], cwd=cwd, check=True,
                   stdout=subprocess.PIPE)
    assert open(wd + "result.txt", "rb").read() == m3_reference_result(os.path.join(src, tag + "_result.txt"), 17227)
    ntar = column3(wd + "confident.txt").size
    raw, bitmap = seen_of(wd + "seen.bin", keys, ntar)
    assert np.array_equal(bits_per_target(bitmap, targets, ntar), column3(wd + "confident.txt")) and column3(wd + "confident.txt").sum() > 0
