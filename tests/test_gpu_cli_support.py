"""--min-hits / --confidence of the three front-ends: the confident file beside the result file equals, byte for byte,
the file the model of tests/read_support_model.py writes from the same probes and reads; every other output equals the
committed goldens (and the hits file the one written without the options); the file does not depend on --batch-reads,
--threads, --devices or --samples-in-flight; --min-hits 0 writes the result file once more."""
import filecmp
import os
import subprocess

import numpy as np
import pytest

from helpers import K, concat_reads, ob, oracle_db
from read_hits_model import HitModel
from read_support_model import SupportModel, result_text
from test_cli_host import nk10  # noqa: F401  (fixture)
from test_cli_vf6_m3 import bins, m3_reference_result, parse_dump, setup_m3, setup_vf6  # noqa: F401  (bins: fixture)
from test_gpu_cli_hits import fastq_reads, probes_of, run_small, stage_small

pytestmark = pytest.mark.gpu

RULE = ["--min-hits", "2", "--confidence", "0.02"]


def model_confident_file(odb, parent, keys, targets, reads, rule=(2, 20), u_is_t=False):
    """reads: [(header, start, stop, sequence)], each one handed to process_read -> the confident file, and how many of
    the reads the rule counts elsewhere than the result file does"""
    hm = HitModel(odb, keys, targets, K, u_is_t=u_is_t)
    model = SupportModel(hm, parent)
    bases, off = concat_reads([r[3] for r in reads])
    start = np.array([r[1] for r in reads], np.int32)
    stop = np.array([r[2] for r in reads], np.int32)
    hits = hm.batch(bases, off, start, stop)
    finals = model.finals(hits)
    assert np.array_equal(ob.OracleSample(odb).classify(bases, off, start, stop), finals)
    rec = model.batch_identity(hits, rule, finals)
    g, u = model.tally(hits, rec, np.ones(len(reads), bool), targets)
    return result_text(g, u).encode(), int((rec["confident"] != rec["final"]).sum())


def confident_of(fq):
    return {p: open(os.path.join(fq, p + "_confident.txt"), "rb").read() for p in ("S1", "S2") if os.path.exists(os.path.join(fq, p + "_confident.txt"))}


def test_nk10_confident_file_equals_the_model_for_any_way_of_running(nk10, gold_dir, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    src, fq, parent = stage_small(gold_dir, cwd)
    keys, targets = probes_of(os.path.join(cwd, "bact10", "probes10.txt.gz"))
    odb = oracle_db(parent, keys, targets, 22)
    exp, moved = {}, 0
    for p in ("S1", "S2"):
        exp[p], m = model_confident_file(odb, parent, keys, targets, fastq_reads(os.path.join(fq, p + "_R1_tr.fastq.gz")) +
                                         fastq_reads(os.path.join(fq, p + "_R2_tr.fastq.gz")))
        moved += m
        assert exp[p] != open(os.path.join(src, p + "_result.txt"), "rb").read()
    assert moved > 20  # the rule decides something on these inputs
    assert run_small(nk10, src, fq, cwd, []) == {} and confident_of(fq) == {}  # without the options: the goldens, nothing else
    hits_alone = run_small(nk10, src, fq, cwd, ["--hits"])
    assert sorted(hits_alone) == ["S1", "S2"] and confident_of(fq) == {}
    for p in ("S1", "S2"):
        open(os.path.join(fq, p + "_confident.txt"), "w").write("left by an earlier run\n")
    for extra in ([], ["--hits"], ["--batch-reads", "37"], ["--threads", "1"], ["--devices", "0,0"], ["--samples-in-flight", "2"]):
        hits = run_small(nk10, src, fq, cwd, RULE + extra)  # (asserts _result.txt, _reads.txt and stdout against the goldens)
        assert hits == (hits_alone if "--hits" in extra else {}), extra
        assert confident_of(fq) == exp, extra
    # --min-hits 0: the rule (0, 0), confident = final for every read
    run_small(nk10, src, fq, cwd, ["--min-hits", "0"])
    for p in ("S1", "S2"):
        assert filecmp.cmp(os.path.join(fq, p + "_confident.txt"), os.path.join(src, p + "_result.txt"), shallow=False)
    run_small(nk10, src, fq, cwd, ["--confidence", "0.02"])  # either option switches the feature on; the other is 0
    one = confident_of(fq)
    assert sorted(one) == ["S1", "S2"] and one != exp


def test_vf6_confident_file_equals_the_model(bins, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    src, params = setup_vf6(cwd)
    dump = os.path.join(cwd, "dry.txt")
    subprocess.run([bins["kmer_read_vf6"], "-name", "DB", "-jname", "J", "--dry-run", dump] + RULE, cwd=cwd, check=True, stdout=subprocess.PIPE)
    par, _, _, files = parse_dump(dump)
    assert not [f for f in os.listdir(os.path.join(cwd, "J")) if "confident" in f]
    keys, targets = probes_of(os.path.join(cwd, "DB", "DB_probes.txt.gz"))
    odb = oracle_db(par, keys, targets, 22, flags=ob.KO_FLAG_U_IS_T)
    exp = {"jobA": model_confident_file(odb, par, keys, targets, files[0][1] + files[1][1], u_is_t=True)[0],
           "jobB": model_confident_file(odb, par, keys, targets, files[2][1] + files[3][1], u_is_t=True)[0]}
    r = subprocess.run([bins["kmer_read_vf6"], "-name", "DB", "-jname", "J", "--log2-slots", "22", "--batch-reads", "37"] + RULE, cwd=cwd,
                       check=True, stdout=subprocess.PIPE)
    assert r.stdout.decode() == open(os.path.join(src, "plain", "stdout.txt")).read()
    produced = sorted(f for f in os.listdir(os.path.join(cwd, "J")) if f != "J.txt")
    golden = sorted(f for f in os.listdir(os.path.join(src, "plain")) if f != "stdout.txt")
    assert produced == sorted(golden + ["jobA_confident.txt", "jobB_confident.txt"])
    for f in golden:
        assert filecmp.cmp(os.path.join(cwd, "J", f), os.path.join(src, "plain", f), shallow=False), f
    for job in ("jobA", "jobB"):
        assert open(os.path.join(cwd, "J", job + "_confident.txt"), "rb").read() == exp[job], job


def test_m3_confident_file_equals_the_model(bins, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    src, params, wd = setup_m3(cwd)
    keys, targets = probes_of(wd + "mitochondria_probes.txt.gz")
    tag, (f1, f2) = sorted(params["runs"].items())[0]
    files_args = ["-wdir", wd, "-f1", wd + f1, "-f2", (wd + f2) if f2 != "none" else "none"]
    dump = os.path.join(cwd, "dry.txt")
    subprocess.run([bins["kmer_read_m3"]] + files_args + ["--dry-run", dump], cwd=cwd, check=True, stdout=subprocess.PIPE)
    par, _, _, files = parse_dump(dump)
    odb = oracle_db(par, keys, targets, params["log2_slots"], max_probes=16)
    exp, _ = model_confident_file(odb, par, keys, targets, [r for f in files for r in f[1]])
    r = subprocess.run([bins["kmer_read_m3"]] + files_args + ["--log2-slots", str(params["log2_slots"]), "--batch-reads", "53"] + RULE,
                       cwd=cwd, check=True, stdout=subprocess.PIPE)
    got = r.stdout.decode().replace(wd, "<WD>").splitlines()
    ref = open(os.path.join(src, tag + "_stdout.txt")).read().splitlines()
    assert [l for i, l in enumerate(got) if i != 6] == [l for i, l in enumerate(ref) if i != 6]
    assert open(wd + "result.txt", "rb").read() == m3_reference_result(os.path.join(src, tag + "_result.txt"), 17227)
    assert open(wd + "confident.txt", "rb").read() == exp and not os.path.exists(wd + "hits.txt")
