"""--loci W of the three front-ends: the loci file beside the result file equals, byte for byte, the file the model of
tests/read_loci_model.py writes from the same probes (with their sites) and reads; it does not depend on --batch-reads,
--threads, --devices, --samples-in-flight or --block-bytes, nor on the database coming from --db-cache; every other output
is what it is without the option; a stale file goes and a sample that fails leaves none."""
import gzip
import os
import subprocess

import numpy as np

import read_loci_model as lm
from helpers import K, concat_reads, ob, oracle_db
from kmer_id_amd import read_probe_sites
from read_hits_model import HitModel
from test_cli_host import make_db_dir, nk10  # noqa: F401  (nk10: fixture)
from test_cli_vf6_m3 import bins, parse_dump, setup_m3, setup_vf6  # noqa: F401  (bins: fixture)
from test_gpu_cli_hits import fastq_reads, probes_of, stage_small
from test_gpu_cli_segments import run_dir

import pytest

pytestmark = pytest.mark.gpu


def model_file(odb, keys, targets, sites, reads, w, u_is_t=False):
    """reads: [(header, start, stop, sequence)] in the reference's order, each one handed to process_read"""
    org, pos = sites
    assert org.size == keys.size and pos.size == keys.size
    bases, off = concat_reads([r[3] for r in reads])
    start = np.array([r[1] for r in reads], np.int32)
    stop = np.array([r[2] for r in reads], np.int32)
    hits = HitModel(odb, keys, targets, K, u_is_t=u_is_t).batch(bases, off, start, stop)
    recs = lm.batch(hits, org, pos, w)
    final = ob.OracleSample(odb).classify(bases, off, start, stop)
    out = []
    for r, (acc, st, sp, _) in enumerate(reads):
        if recs["n_hits"][r]:
            out.append(b"%d\t%d\t%d\t%d\t%s\t%s\n" % (int(final[r]), sp - st + 1, int(recs["n_kmers"][r]), int(recs["n_hits"][r]),
                                                    lm.line(recs[r], pos).encode(), acc))
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
    exp = {p: model_file(odb, keys, targets, sites, reads[p], 7) for p in reads}
    exp1 = {p: model_file(odb, keys, targets, sites, reads[p], 1) for p in reads}
    assert all(e.count(b"\n") > 50 for e in exp.values())
    base_out, base = run_dir(nk10, fq, cwd, ["--hits"])
    assert sorted(base) == sorted(p + s for p in samples for s in ("_hits.txt", "_reads.txt", "_result.txt"))
    for p in samples:  # the lines of the loci file are those of the hits file, in its order
        assert [l.split(b"\t")[:4] + l.split(b"\t")[5:] for l in exp[p].splitlines()] == \
               [l.split(b"\t")[:4] + l.split(b"\t")[5:] for l in base[p + "_hits.txt"].splitlines()]
        open(os.path.join(fq, p + "_loci.txt"), "w").write("left by an earlier run\n")  # removed when its sample starts
    opt = ["--loci", "7"]
    cache = os.path.join(cwd, "db.cache")
    for extra in ([], ["--batch-reads", "7"], ["--batch-reads", "53", "--devices", "0,0"], ["--threads", "1", "--samples-in-flight", "1"],
                  ["--block-bytes", "32768", "--threads", "3"], ["--db-cache", cache], ["--db-cache", cache, "--batch-reads", "31"]):
        out, got = run_dir(nk10, fq, cwd, ["--hits"] + opt + extra, clean=bool(extra))  # (the first run meets the stale files)
        assert out == base_out, extra
        for p in samples:
            assert got.pop(p + "_loci.txt") == exp[p], (extra, p)
        assert got == base, extra  # every other output is byte for byte what it is without the option
    assert os.path.getsize(cache) > 0  # (the second of the two runs read the database from it, and the sites from the text)
    out, got = run_dir(nk10, fq, cwd, ["--loci", "1"])
    assert {p: got[p + "_loci.txt"] for p in samples} == exp1 and sorted(got) == sorted(
        p + s for p in samples for s in ("_loci.txt", "_reads.txt", "_result.txt"))
    plain_out, plain = run_dir(nk10, fq, cwd, [])
    assert all(got[f] == plain[f] for f in plain) and out == plain_out and sorted(plain) == sorted(p + s for p in samples for s in ("_reads.txt", "_result.txt"))


def test_nk10_masks_apply_as_they_do_to_the_hits_file(nk10, gold_dir, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    src, fq, parent = stage_small(gold_dir, cwd)
    masks = ["--min-base-quality", "20", "--low-complexity", "20"]
    _, got = run_dir(nk10, fq, cwd, ["--hits", "--loci", "1"] + masks)
    _, plain = run_dir(nk10, fq, cwd, ["--hits", "--loci", "1"])
    changed = 0
    for p in ("S1", "S2"):
        hits, loci = got[p + "_hits.txt"].splitlines(), got[p + "_loci.txt"].splitlines()
        assert len(hits) == len(loci)
        for h, l in zip(hits, loci):  # the reads, windows and hits of the masked text, in both files
            assert h.split(b"\t")[:4] == l.split(b"\t")[:4] and h.split(b"\t")[5:] == l.split(b"\t")[5:]
        changed += got[p + "_loci.txt"] != plain[p + "_loci.txt"]
    assert changed


def test_nk10_failing_sample_leaves_no_file(nk10, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    make_db_dir(cwd, 2e-5)
    fq = os.path.join(cwd, "fq"); os.makedirs(fq)
    with gzip.open(os.path.join(fq, "L_R1_tr.fastq.gz"), "wb") as fh:
        fh.write(b"@a\n" + b"ACGT" * 10 + b"\n+\n" + b"I" * 39 + b"\n")  # a quality line shorter than its sequence
    with gzip.open(os.path.join(fq, "L_R2_tr.fastq.gz"), "wb") as fh:
        fh.write(b"@b\nACGT\n+\nIIII\n")
    open(os.path.join(fq, "L_loci.txt"), "w").write("left by an earlier run\n")
    r = subprocess.run([nk10, fq + "/", "--log2-slots", "16", "--loci", "10"], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 134, (r.returncode, r.stderr[-500:])
    assert b"quality line shorter than the sequence" in r.stderr
    assert not os.path.exists(os.path.join(fq, "L_loci.txt")) and not os.path.exists(os.path.join(fq, "L_result.txt"))


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
    exp = {"jobA": model_file(odb, keys, targets, sites, files[0][1] + files[1][1], 5, u_is_t=True),
           "jobB": model_file(odb, keys, targets, sites, files[2][1] + files[3][1], 5, u_is_t=True)}
    assert all(e.count(b"\n") > 5 for e in exp.values())
    jdir = os.path.join(cwd, "J")
    run = [prog, "-name", "DB", "-jname", "J", "--log2-slots", "22", "--batch-reads", "37"]
    plain = subprocess.run(run, cwd=cwd, check=True, stdout=subprocess.PIPE).stdout
    before = {f: open(os.path.join(jdir, f), "rb").read() for f in os.listdir(jdir)}
    open(os.path.join(jdir, "jobA_loci.txt"), "w").write("left by an earlier run\n")
    r = subprocess.run(run + ["--loci", "5"], cwd=cwd, check=True, stdout=subprocess.PIPE)
    after = {f: open(os.path.join(jdir, f), "rb").read() for f in os.listdir(jdir)}
    got = {job: after.pop(job + "_loci.txt") for job in exp}
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
    exp = model_file(odb, keys, targets, sites, [r for f in files for r in f[1]], 3)
    assert exp.count(b"\n") > 5
    open(wd + "loci.txt", "w").write("left by an earlier run\n")
    subprocess.run([bins["kmer_read_m3"]] + files_args + ["--log2-slots", str(params["log2_slots"]), "--batch-reads", "53", "--loci", "3"], cwd=cwd,
                   check=True, stdout=subprocess.PIPE)
    assert open(wd + "loci.txt", "rb").read() == exp
