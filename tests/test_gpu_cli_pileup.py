"""--pileup W[:MIN_CHAIN[:MIN_MARGIN]] of the three front-ends: the pileup file beside the result file equals, byte for byte,
the lines formatted from the model of tests/read_pileup_model.py on the loci records the model of tests/read_loci_model.py
makes from the same probes (with their sites) and reads; it does not depend on --batch-reads, --threads, --devices,
--samples-in-flight or --block-bytes; with --loci W' the one loci pass feeds both files and the pileup uses its records;
every other output is what it is without the option; a stale file goes and a sample that fails leaves none."""
import gzip
import os
import subprocess

import numpy as np

import read_loci_model as lm
import read_pileup_model as pm
from helpers import K, concat_reads, ob, oracle_db
from kmer_id_amd import read_probe_sites
from read_hits_model import HitModel
from test_cli_host import make_db_dir, nk10  # noqa: F401  (nk10: fixture)
from test_cli_vf6_m3 import bins, parse_dump, setup_m3, setup_vf6  # noqa: F401  (bins: fixture)
from test_gpu_cli_hits import fastq_reads, probes_of, stage_small
from test_gpu_cli_segments import run_dir

import pytest

pytestmark = pytest.mark.gpu


def model_file(odb, keys, targets, sites, reads, w, min_chain=2, min_margin=1, diag_bin=1, u_is_t=False):
    """reads: [(header, start, stop, sequence)], each one handed to process_read -> the pileup file"""
    org, pos = sites
    assert org.size == keys.size and pos.size == keys.size
    bases, off = concat_reads([r[3] for r in reads])
    start = np.array([r[1] for r in reads], np.int32)
    stop = np.array([r[2] for r in reads], np.int32)
    hits = HitModel(odb, keys, targets, K, u_is_t=u_is_t).batch(bases, off, start, stop)
    loci = lm.batch(hits, org, pos, diag_bin)
    bin_base, starts, depth, recs, n_placed = pm.batch(loci, org, pos, K, w, min_chain, min_margin)
    out = [b"#%d,%d,%d,%d,%d\n" % (len(reads), n_placed, w, min_chain, min_margin)]
    for g in np.flatnonzero(recs["n_placed"]).tolist():
        out.append(b"%d,%s\n" % (g, b",".join(b"%d" % int(recs[g][f]) for f in pm.PILEUP_DTYPE.names if f != "reserved")))
    return b"".join(out)


def test_nk10_file_equals_the_model_for_any_way_of_running(nk10, gold_dir, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    src, fq, parent = stage_small(gold_dir, cwd)
    probes = os.path.join(cwd, "bact10", "probes10.txt.gz")
    keys, targets = probes_of(probes)
    sites = read_probe_sites(probes)
    odb = oracle_db(parent, keys, targets, 22)
    samples = ("S1", "S2")
    reads = {p: fastq_reads(os.path.join(fq, p + "_R1_tr.fastq.gz")) + fastq_reads(os.path.join(fq, p + "_R2_tr.fastq.gz")) for p in samples}
    assert sum(len(r) for r in reads.values()) >= 200
    exp = {p: model_file(odb, keys, targets, sites, reads[p], 100, 1, 0) for p in reads}
    exp7 = {p: model_file(odb, keys, targets, sites, reads[p], 100, diag_bin=7) for p in reads}
    exp1 = {p: model_file(odb, keys, targets, sites, reads[p], 100) for p in reads}
    exp_default = {p: model_file(odb, keys, targets, sites, reads[p], 1000) for p in reads}
    placed = lambda e: int(e.split(b"\n")[0].split(b",")[1])  # noqa: E731
    assert all(placed(e) > 50 and e.count(b"\n") == 2 and b"\r" not in e for e in exp.values())
    assert placed(exp7["S1"]) > placed(exp1["S1"]) >= 1  # (the reads are synthetic: wider diagonals gather longer chains)
    base_out, base = run_dir(nk10, fq, cwd, ["--hits"])
    for p in samples:
        open(os.path.join(fq, p + "_pileup.txt"), "w").write("left by an earlier run\n")  # removed when its sample starts
    opt = ["--pileup", "100:1:0"]
    for extra in ([], ["--batch-reads", "7"], ["--batch-reads", "53", "--devices", "0,0"], ["--threads", "1", "--samples-in-flight", "1"],
                  ["--block-bytes", "32768", "--threads", "3"], ["--samples-in-flight", "2", "--batch-reads", "31"]):
        out, got = run_dir(nk10, fq, cwd, ["--hits"] + opt + extra, clean=bool(extra))  # (the first run meets the stale files)
        assert out == base_out, extra
        for p in samples:
            assert got.pop(p + "_pileup.txt") == exp[p], (extra, p)
        assert got == base, extra  # every other output is byte for byte what it is without the option
    loci_out, with_loci = run_dir(nk10, fq, cwd, ["--hits", "--loci", "7"])
    # with --loci 7 there is one loci pass: the loci file is what it is without --pileup, and the pileup is of its diag_bin = 7 records
    for extra in ([], ["--batch-reads", "11", "--devices", "0,0"]):
        out, got = run_dir(nk10, fq, cwd, ["--hits", "--loci", "7", "--pileup", "100:2:1"] + extra)
        assert out == loci_out
        for p in samples:
            assert got.pop(p + "_pileup.txt") == exp7[p], (extra, p)
        assert got == with_loci, extra
    out, got = run_dir(nk10, fq, cwd, ["--pileup", "1000"])  # MIN_CHAIN 2 and MIN_MARGIN 1 when not given; diag_bin 1 without --loci
    assert {p: got[p + "_pileup.txt"] for p in samples} == exp_default and sorted(got) == sorted(
        p + s for p in samples for s in ("_pileup.txt", "_reads.txt", "_result.txt"))


def test_nk10_masks_apply_as_they_do_to_the_loci_file(nk10, gold_dir, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    src, fq, parent = stage_small(gold_dir, cwd)
    masks = ["--min-base-quality", "20", "--low-complexity", "20"]
    _, got = run_dir(nk10, fq, cwd, ["--loci", "1", "--pileup", "1:1:0"] + masks)
    _, plain = run_dir(nk10, fq, cwd, ["--loci", "1", "--pileup", "1:1:0"])
    changed = 0
    for p in ("S1", "S2"):
        # under (1, 0) every read of the loci file with a chain is placed: the head line counts them
        with_chain = sum(1 for l in got[p + "_loci.txt"].splitlines() if int(l.split(b"\t")[4].split(b":")[2]) >= 1)
        head = got[p + "_pileup.txt"].splitlines()[0]
        assert int(head[1:].split(b",")[1]) == with_chain > 50
        changed += got[p + "_pileup.txt"] != plain[p + "_pileup.txt"]
    assert changed


def test_nk10_failing_sample_leaves_no_file(nk10, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    make_db_dir(cwd, 2e-5)
    fq = os.path.join(cwd, "fq"); os.makedirs(fq)
    with gzip.open(os.path.join(fq, "L_R1_tr.fastq.gz"), "wb") as fh:
        fh.write(b"@a\n" + b"ACGT" * 10 + b"\n+\n" + b"I" * 39 + b"\n")  # a quality line shorter than its sequence
    with gzip.open(os.path.join(fq, "L_R2_tr.fastq.gz"), "wb") as fh:
        fh.write(b"@b\nACGT\n+\nIIII\n")
    open(os.path.join(fq, "L_pileup.txt"), "w").write("left by an earlier run\n")
    r = subprocess.run([nk10, fq + "/", "--log2-slots", "16", "--pileup", "10"], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 134, (r.returncode, r.stderr[-500:])
    assert b"quality line shorter than the sequence" in r.stderr
    assert not os.path.exists(os.path.join(fq, "L_pileup.txt")) and not os.path.exists(os.path.join(fq, "L_result.txt"))


def test_vf6_file_equals_the_model(bins, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    src, params = setup_vf6(cwd)
    prog = bins["kmer_read_vf6"]
    dump = os.path.join(cwd, "dry.txt")
    subprocess.run([prog, "-name", "DB", "-jname", "J", "--dry-run", dump], cwd=cwd, check=True, stdout=subprocess.PIPE)
    par, _, _, files = parse_dump(dump)
    probes = os.path.join(cwd, "DB", "DB_probes.txt.gz")
    keys, targets = probes_of(probes)
    sites = read_probe_sites(probes)
    odb = oracle_db(par, keys, targets, 22, flags=ob.KO_FLAG_U_IS_T)
    exp = {"jobA": model_file(odb, keys, targets, sites, files[0][1] + files[1][1], 50, 1, 0, u_is_t=True),
           "jobB": model_file(odb, keys, targets, sites, files[2][1] + files[3][1], 50, 1, 0, u_is_t=True)}
    assert all(e.count(b"\n") >= 2 for e in exp.values())
    jdir = os.path.join(cwd, "J")
    run = [prog, "-name", "DB", "-jname", "J", "--log2-slots", "22", "--batch-reads", "37"]
    plain = subprocess.run(run, cwd=cwd, check=True, stdout=subprocess.PIPE).stdout
    before = {f: open(os.path.join(jdir, f), "rb").read() for f in os.listdir(jdir)}
    open(os.path.join(jdir, "jobA_pileup.txt"), "w").write("left by an earlier run\n")
    r = subprocess.run(run + ["--pileup", "50:1:0"], cwd=cwd, check=True, stdout=subprocess.PIPE)
    after = {f: open(os.path.join(jdir, f), "rb").read() for f in os.listdir(jdir)}
    got = {job: after.pop(job + "_pileup.txt") for job in exp}
    assert r.stdout == plain and after == before and got == exp


def test_m3_runs_once(bins, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    src, params, wd = setup_m3(cwd)
    probes = wd + "mitochondria_probes.txt.gz"
    keys, targets = probes_of(probes)
    sites = read_probe_sites(probes)
    tag, (f1, f2) = sorted(params["runs"].items())[0]
    files_args = ["-wdir", wd, "-f1", wd + f1, "-f2", (wd + f2) if f2 != "none" else "none"]
    dump = os.path.join(cwd, "dry.txt")
    subprocess.run([bins["kmer_read_m3"]] + files_args + ["--dry-run", dump], cwd=cwd, check=True, stdout=subprocess.PIPE)
    par, _, _, files = parse_dump(dump)
    odb = oracle_db(par, keys, targets, params["log2_slots"], max_probes=16)
    exp = model_file(odb, keys, targets, sites, [r for f in files for r in f[1]], 30, 1, 0, diag_bin=3)
    assert exp.count(b"\n") >= 2
    open(wd + "pileup.txt", "w").write("left by an earlier run\n")
    subprocess.run([bins["kmer_read_m3"]] + files_args + ["--log2-slots", str(params["log2_slots"]), "--batch-reads", "53", "--loci", "3",
                                                         "--pileup", "30:1:0"], cwd=cwd, check=True, stdout=subprocess.PIPE)
    assert open(wd + "pileup.txt", "rb").read() == exp
