"""--depth of the three front-ends: the depth file beside the result file equals, byte for byte, the lines the model of
tests/read_depth_model.py writes from the same probes and reads (and those it writes from the Python path's spectrum),
with and without a rule; its third column is the third column of the confident file (of the result file without a rule);
it does not depend on --batch-reads, --threads, --devices or --samples-in-flight; every other file and stdout are what
they are without the option; a sample that fails leaves none."""
import filecmp
import os
import subprocess

import numpy as np
import pytest

import read_depth_model as dm
from helpers import K, concat_reads, ob, oracle_db
from kmer_id_amd import KID_OPT_ENTRY_DEPTH, KmerDB
from read_hits_model import HitModel
from read_support_model import SupportModel
from test_cli_host import nk10  # noqa: F401  (fixture)
from test_cli_vf6_m3 import bins, m3_reference_result, parse_dump, setup_m3, setup_vf6  # noqa: F401  (bins: fixture)
from test_gpu_cli_hits import fastq_reads, probes_of, run_small, stage_small

pytestmark = pytest.mark.gpu

RULE = ["--min-hits", "2", "--confidence", "0.02"]


def batch_of(reads):
    """reads: [(header, start, stop, sequence)], each one handed to process_read"""
    bases, off = concat_reads([r[3] for r in reads])
    return bases, off, np.array([r[1] for r in reads], np.int32), np.array([r[2] for r in reads], np.int32)


def model_depth_file(odb, parent, keys, targets, reads, rule, u_is_t=False):
    hm = HitModel(odb, keys, targets, K, u_is_t=u_is_t)
    model = SupportModel(hm, parent)
    bases, off, start, stop = batch_of(reads)
    hits = hm.batch(bases, off, start, stop)
    rec = model.batch_identity(hits, rule, model.finals(hits))
    depth = dm.depth_of(hits, rec, np.ones(len(reads), bool), keys.size)
    return dm.depth_lines(*dm.spectrum_of(depth, targets, parent.size, dm.FILE_BINS)).encode()


def column3(text):
    return [line.split(b",")[2] for line in text.splitlines()]


def side_files(fq, word):
    return {p: open(os.path.join(fq, "%s_%s.txt" % (p, word)), "rb").read() for p in ("S1", "S2")
            if os.path.exists(os.path.join(fq, "%s_%s.txt" % (p, word)))}


def test_nk10_depth_file_equals_the_model_for_any_way_of_running(nk10, gold_dir, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    src, fq, parent = stage_small(gold_dir, cwd)
    keys, targets = probes_of(os.path.join(cwd, "bact10", "probes10.txt.gz"))
    odb = oracle_db(parent, keys, targets, 22)
    reads = {p: fastq_reads(os.path.join(fq, p + "_R1_tr.fastq.gz")) + fastq_reads(os.path.join(fq, p + "_R2_tr.fastq.gz")) for p in ("S1", "S2")}
    exp = {rule: {p: model_depth_file(odb, parent, keys, targets, reads[p], rule) for p in ("S1", "S2")} for rule in ((0, 0), (2, 20))}
    assert exp[(0, 0)] != exp[(2, 20)] and all(e.count(b"\n") == parent.size for e in exp[(0, 0)].values())
    assert any(int(line.split(b",")[6]) > 1 for line in exp[(0, 0)]["S1"].splitlines())  # some k-mer is hit more than once
    # the Python path on the same reads: its spectrum, written by the model's rule, is the same file
    db = KmerDB(keys, targets, parent, k=30, log2_slots=22)
    s = db.sample()
    s.set_option(KID_OPT_ENTRY_DEPTH, 1)
    for rule in exp:
        for p in ("S1", "S2"):
            s.reset()
            bases, off, start, stop = batch_of(reads[p])
            db.read_support(bases, off, start, stop, min_hits=rule[0], min_permille=rule[1], tally=s)
            assert dm.depth_lines(*s.depth_spectrum(dm.FILE_BINS)).encode() == exp[rule][p], (rule, p)
    s.close(), db.close()
    # without the option: the goldens (run_small holds _result.txt, _reads.txt and stdout against them) and no depth file
    assert run_small(nk10, src, fq, cwd, []) == {} and side_files(fq, "depth") == {}
    run_small(nk10, src, fq, cwd, RULE)
    confident_alone = side_files(fq, "confident")
    assert sorted(confident_alone) == ["S1", "S2"] and side_files(fq, "depth") == {}
    for p in ("S1", "S2"):
        open(os.path.join(fq, p + "_depth.txt"), "w").write("left by an earlier run\n")
    for extra in ([], ["--batch-reads", "37"], ["--batch-reads", "1000000", "--threads", "1"], ["--devices", "0,0"], ["--samples-in-flight", "2"]):
        assert run_small(nk10, src, fq, cwd, ["--depth"] + RULE + extra) == {}, extra  # (no hits file)
        assert side_files(fq, "depth") == exp[(2, 20)] and side_files(fq, "confident") == confident_alone, extra
    for p in ("S1", "S2"):
        assert column3(exp[(2, 20)][p]) == column3(confident_alone[p])
    # without a rule: (0, 0), and no confident file
    for extra in ([], ["--devices", "0,0", "--batch-reads", "37"]):
        assert run_small(nk10, src, fq, cwd, ["--depth"] + extra) == {}
        assert side_files(fq, "depth") == exp[(0, 0)] and side_files(fq, "confident") == {}, extra
    for p in ("S1", "S2"):
        assert column3(exp[(0, 0)][p]) == column3(open(os.path.join(src, p + "_result.txt"), "rb").read())


@pytest.mark.parametrize("options, words", [(["--depth"], ["depth"]), (["--depth", "--min-hits", "2"], ["depth", "confident"])],
                         ids=["depth", "depth-and-rule"])
def test_nk10_failing_sample_leaves_no_depth_file(nk10, gold_dir, tmp_path, options, words):  # noqa: F811
    cwd = str(tmp_path)
    src, fq, parent = stage_small(gold_dir, cwd)
    p = os.path.join(fq, "S2_R2_tr.fastq.gz")
    raw = open(p, "rb").read()
    open(p, "wb").write(raw[:len(raw) * 2 // 3])  # cut off: everything in front is read, then "failed gzclose", exit 255
    for prefix in ("S1", "S2"):
        for word in words:
            open(os.path.join(fq, "%s_%s.txt" % (prefix, word)), "w").write("left by an earlier run\n")
    r = subprocess.run([nk10, fq + "/", "--log2-slots", "22", "--samples-in-flight", "1"] + options, cwd=cwd, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE)
    assert r.returncode == 255 and b"failed gzclose" in r.stderr
    for word in words + ["result"]:
        assert not os.path.exists(os.path.join(fq, "S2_%s.txt" % word)), word
    # S1 is whole if the directory order put it first, and was never started (or was taken back) otherwise
    whole = os.path.exists(os.path.join(fq, "S1_result.txt"))
    for word in words:
        s1 = os.path.join(fq, "S1_%s.txt" % word)
        assert os.path.exists(s1) == whole, word
        if whole:
            assert b"left by an earlier run" not in open(s1, "rb").read(), word


def test_vf6_depth_file_equals_the_model(bins, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    src, params = setup_vf6(cwd)
    dump = os.path.join(cwd, "dry.txt")
    subprocess.run([bins["kmer_read_vf6"], "-name", "DB", "-jname", "J", "--dry-run", dump, "--depth"], cwd=cwd, check=True, stdout=subprocess.PIPE)
    par, _, _, files = parse_dump(dump)
    assert not [f for f in os.listdir(os.path.join(cwd, "J")) if "depth" in f]
    keys, targets = probes_of(os.path.join(cwd, "DB", "DB_probes.txt.gz"))
    odb = oracle_db(par, keys, targets, 22, flags=ob.KO_FLAG_U_IS_T)
    jobs = {"jobA": files[0][1] + files[1][1], "jobB": files[2][1] + files[3][1]}
    golden = sorted(f for f in os.listdir(os.path.join(src, "plain")) if f != "stdout.txt")
    for rule, words, more in (((0, 0), [], ["depth"]), ((2, 20), RULE, ["confident", "depth"])):
        exp = {job: model_depth_file(odb, par, keys, targets, reads, rule, u_is_t=True) for job, reads in jobs.items()}
        for extra in (["--batch-reads", "37"], ["--devices", "0,0"]):
            for f in os.listdir(os.path.join(cwd, "J")):
                if f != "J.txt":
                    os.remove(os.path.join(cwd, "J", f))
            r = subprocess.run([bins["kmer_read_vf6"], "-name", "DB", "-jname", "J", "--log2-slots", "22", "--depth"] + words + extra, cwd=cwd,
                               check=True, stdout=subprocess.PIPE)
            assert r.stdout.decode() == open(os.path.join(src, "plain", "stdout.txt")).read()
            produced = sorted(f for f in os.listdir(os.path.join(cwd, "J")) if f != "J.txt")
            assert produced == sorted(golden + ["%s_%s.txt" % (job, w) for job in jobs for w in more]), (rule, extra)
            for f in golden:
                assert filecmp.cmp(os.path.join(cwd, "J", f), os.path.join(src, "plain", f), shallow=False), f
            for job in jobs:
                got = open(os.path.join(cwd, "J", job + "_depth.txt"), "rb").read()
                assert got == exp[job], (rule, extra, job)
                other = os.path.join(cwd, "J", job + ("_confident.txt" if words else "_result.txt"))
                assert column3(got) == column3(open(other, "rb").read()), (rule, job)


def test_m3_depth_file_equals_the_model(bins, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    src, params, wd = setup_m3(cwd)
    keys, targets = probes_of(wd + "mitochondria_probes.txt.gz")
    tag, (f1, f2) = sorted(params["runs"].items())[0]
    files_args = ["-wdir", wd, "-f1", wd + f1, "-f2", (wd + f2) if f2 != "none" else "none"]
    dump = os.path.join(cwd, "dry.txt")
    subprocess.run([bins["kmer_read_m3"]] + files_args + ["--dry-run", dump, "--depth"], cwd=cwd, check=True, stdout=subprocess.PIPE)
    assert not os.path.exists(wd + "depth.txt")
    par, _, _, files = parse_dump(dump)
    odb = oracle_db(par, keys, targets, params["log2_slots"], max_probes=16)
    reads = [r for f in files for r in f[1]]
    ref = open(os.path.join(src, tag + "_stdout.txt")).read().splitlines()
    for rule, words in (((0, 0), []), ((2, 20), RULE)):
        exp = model_depth_file(odb, par, keys, targets, reads, rule)
        for extra in (["--batch-reads", "53"], ["--devices", "0,0"]):
            for f in ("depth.txt", "confident.txt", "result.txt"):
                if os.path.exists(wd + f):
                    os.remove(wd + f)
            r = subprocess.run([bins["kmer_read_m3"]] + files_args + ["--log2-slots", str(params["log2_slots"]), "--depth"] + words + extra,
                               cwd=cwd, check=True, stdout=subprocess.PIPE)
            got = r.stdout.decode().replace(wd, "<WD>").splitlines()
            assert [l for i, l in enumerate(got) if i != 6] == [l for i, l in enumerate(ref) if i != 6]
            assert open(wd + "result.txt", "rb").read() == m3_reference_result(os.path.join(src, tag + "_result.txt"), 17227)
            depth = open(wd + "depth.txt", "rb").read()
            assert depth == exp and os.path.exists(wd + "confident.txt") == bool(words) and not os.path.exists(wd + "hits.txt"), (rule, extra)
            assert column3(depth) == column3(open(wd + ("confident.txt" if words else "result.txt"), "rb").read())
