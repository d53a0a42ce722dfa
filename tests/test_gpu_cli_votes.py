"""--votes of the three front-ends: the votes file beside the result file equals, byte for byte, the file the model of
tests/read_votes_model.py writes from the same probes and reads; it is the same for two values each of --batch-reads and
--threads; every other output is what it is without the option (the committed goldens; the confident and hits files
those written without --votes)."""
import filecmp
import os
import subprocess

import numpy as np
import pytest

from helpers import K, concat_reads, ob, oracle_db
from read_hits_model import HitModel
from read_support_model import SupportModel, result_text
from read_votes_model import VoteModel
from test_cli_host import nk10  # noqa: F401  (fixture)
from test_cli_vf6_m3 import bins, m3_reference_result, parse_dump, setup_m3, setup_vf6  # noqa: F401  (bins: fixture)
from test_gpu_cli_hits import fastq_reads, probes_of, run_small, stage_small
from test_gpu_cli_support import confident_of

pytestmark = pytest.mark.gpu

RULE = ["--min-hits", "2", "--confidence", "0.02"]


def model_votes_file(odb, parent, keys, targets, reads, rule=(0, 0), u_is_t=False):
    """reads: [(header, start, stop, sequence)], each one handed to process_read -> the votes file, and how many of the
    reads are counted elsewhere than the result file counts them"""
    hm = HitModel(odb, keys, targets, K, u_is_t=u_is_t)
    sm = SupportModel(hm, parent)
    bases, off = concat_reads([r[3] for r in reads])
    start = np.array([r[1] for r in reads], np.int32)
    stop = np.array([r[2] for r in reads], np.int32)
    hits = hm.batch(bases, off, start, stop)
    rec = VoteModel(sm).batch_anc(hits, rule)
    g, u = sm.tally(hits, rec, np.ones(len(reads), bool), targets)
    return result_text(g, u).encode(), int((rec["confident"] != sm.finals(hits)).sum())


def votes_of(fq):
    return {p: open(os.path.join(fq, p + "_votes.txt"), "rb").read() for p in ("S1", "S2") if os.path.exists(os.path.join(fq, p + "_votes.txt"))}


def test_nk10_votes_file_equals_the_model_for_any_way_of_running(nk10, gold_dir, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    src, fq, parent = stage_small(gold_dir, cwd)
    keys, targets = probes_of(os.path.join(cwd, "bact10", "probes10.txt.gz"))
    odb = oracle_db(parent, keys, targets, 22)
    exp, exp_rule, n_reads, order_matters = {}, {}, 0, 0
    for p in ("S1", "S2"):
        reads = fastq_reads(os.path.join(fq, p + "_R1_tr.fastq.gz")) + fastq_reads(os.path.join(fq, p + "_R2_tr.fastq.gz"))
        n_reads += len(reads)
        exp[p], moved = model_votes_file(odb, parent, keys, targets, reads)
        order_matters += moved
        exp_rule[p], moved = model_votes_file(odb, parent, keys, targets, reads, (2, 20))
        assert moved > 10 and exp_rule[p] != exp[p]
    assert n_reads > 500 and order_matters >= 1  # a few hundred reads, one at least called elsewhere than its fold
    assert exp["S1"] != open(os.path.join(src, "S1_result.txt"), "rb").read()
    assert run_small(nk10, src, fq, cwd, []) == {} and votes_of(fq) == {}  # without the option: the goldens, nothing else
    hits_alone = run_small(nk10, src, fq, cwd, ["--hits"] + RULE)
    confident_alone = confident_of(fq)
    assert sorted(hits_alone) == ["S1", "S2"] and sorted(confident_alone) == ["S1", "S2"] and votes_of(fq) == {}
    for p in ("S1", "S2"):
        open(os.path.join(fq, p + "_votes.txt"), "w").write("left by an earlier run\n")
    for extra in ([], ["--batch-reads", "37"], ["--batch-reads", "1000"], ["--threads", "1"], ["--threads", "3"], ["--devices", "0,0"],
                  ["--samples-in-flight", "2"]):
        assert run_small(nk10, src, fq, cwd, ["--votes"] + extra) == {}, extra  # (asserts _result.txt, _reads.txt and stdout against the goldens)
        assert votes_of(fq) == exp and confident_of(fq) == {}, extra
    # under a rule: the votes file follows it, and the confident and hits files are what they are without --votes
    assert run_small(nk10, src, fq, cwd, ["--votes", "--hits"] + RULE) == hits_alone
    assert votes_of(fq) == exp_rule and confident_of(fq) == confident_alone
    assert sorted(f for f in os.listdir(fq) if f.endswith(".txt")) == sorted(p + s for p in ("S1", "S2") for s in
                                                                             ("_confident.txt", "_hits.txt", "_reads.txt", "_result.txt", "_votes.txt"))


def test_vf6_votes_file_equals_the_model(bins, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    src, params = setup_vf6(cwd)
    dump = os.path.join(cwd, "dry.txt")
    subprocess.run([bins["kmer_read_vf6"], "-name", "DB", "-jname", "J", "--dry-run", dump, "--votes"], cwd=cwd, check=True, stdout=subprocess.PIPE)
    par, _, _, files = parse_dump(dump)
    assert not [f for f in os.listdir(os.path.join(cwd, "J")) if "votes" in f]
    keys, targets = probes_of(os.path.join(cwd, "DB", "DB_probes.txt.gz"))
    odb = oracle_db(par, keys, targets, 22, flags=ob.KO_FLAG_U_IS_T)
    exp = {"jobA": model_votes_file(odb, par, keys, targets, files[0][1] + files[1][1], u_is_t=True)[0],
           "jobB": model_votes_file(odb, par, keys, targets, files[2][1] + files[3][1], u_is_t=True)[0]}
    golden = sorted(f for f in os.listdir(os.path.join(src, "plain")) if f != "stdout.txt")
    for extra in (["--batch-reads", "37"], ["--batch-reads", "500", "--threads", "1"], ["--threads", "4"]):
        r = subprocess.run([bins["kmer_read_vf6"], "-name", "DB", "-jname", "J", "--log2-slots", "22", "--votes"] + extra, cwd=cwd, check=True,
                           stdout=subprocess.PIPE)
        assert r.stdout.decode() == open(os.path.join(src, "plain", "stdout.txt")).read(), extra
        produced = sorted(f for f in os.listdir(os.path.join(cwd, "J")) if f != "J.txt")
        assert produced == sorted(golden + ["jobA_votes.txt", "jobB_votes.txt"]), extra
        for f in golden:
            assert filecmp.cmp(os.path.join(cwd, "J", f), os.path.join(src, "plain", f), shallow=False), (extra, f)
        for job in ("jobA", "jobB"):
            assert open(os.path.join(cwd, "J", job + "_votes.txt"), "rb").read() == exp[job], (extra, job)


def test_m3_votes_file_equals_the_model(bins, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    src, params, wd = setup_m3(cwd)
    keys, targets = probes_of(wd + "mitochondria_probes.txt.gz")
    tag, (f1, f2) = sorted(params["runs"].items())[0]
    files_args = ["-wdir", wd, "-f1", wd + f1, "-f2", (wd + f2) if f2 != "none" else "none"]
    dump = os.path.join(cwd, "dry.txt")
    subprocess.run([bins["kmer_read_m3"]] + files_args + ["--dry-run", dump], cwd=cwd, check=True, stdout=subprocess.PIPE)
    par, _, _, files = parse_dump(dump)
    odb = oracle_db(par, keys, targets, params["log2_slots"], max_probes=16)
    exp, _ = model_votes_file(odb, par, keys, targets, [r for f in files for r in f[1]], (2, 20))
    ref = open(os.path.join(src, tag + "_stdout.txt")).read().splitlines()
    for extra in (["--batch-reads", "53"], ["--batch-reads", "400", "--threads", "1"], ["--threads", "4"]):
        r = subprocess.run([bins["kmer_read_m3"]] + files_args + ["--log2-slots", str(params["log2_slots"]), "--votes"] + RULE + extra,
                           cwd=cwd, check=True, stdout=subprocess.PIPE)
        got = r.stdout.decode().replace(wd, "<WD>").splitlines()
        assert [l for i, l in enumerate(got) if i != 6] == [l for i, l in enumerate(ref) if i != 6], extra
        assert open(wd + "result.txt", "rb").read() == m3_reference_result(os.path.join(src, tag + "_result.txt"), 17227), extra
        assert open(wd + "votes.txt", "rb").read() == exp and not os.path.exists(wd + "hits.txt"), extra
