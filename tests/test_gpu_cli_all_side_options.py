"""Every side option of a front-end given together: each side file is byte for byte the file of a run with that file's
option alone (under the same rule of --min-hits / --confidence, which every one of them follows; the pileup file under
the same --loci, whose records it piles up), stdout and the result and reads files are what they are in every such run,
and no other file appears.  The run with everything has replicas, workers, merges and many batches (--devices 0,0
--samples-in-flight 2 --batch-reads 7), the runs with one option are plain.  The two masks (--min-base-quality,
--low-complexity) write no file and change every one: they are not part of this."""
import os
import subprocess

import pytest

from test_cli_host import nk10  # noqa: F401  (nk10: fixture)
from test_cli_vf6_m3 import bins, setup_vf6  # noqa: F401  (bins: fixture)
from test_gpu_cli_hits import stage_small
from test_gpu_cli_segments import run_dir

pytestmark = pytest.mark.gpu

RULE = ["--min-hits", "2", "--confidence", "0.02"]
# side file -> its option with the modifiers it depends on beside the rule; the geometries are those the tests of each
# option use on this input (the pileup under (1, 0): under (2, 1) the second sample has no placed read)
OPTIONS = {"confident": [], "fragments": ["--fragments"], "votes": ["--votes"], "fragment_votes": ["--fragment-votes"], "depth": ["--depth"],
           "seen": ["--seen"], "hits": ["--hits"], "segments": ["--segments", "64:16"], "segment_votes": ["--segment-votes", "40:20"],
           "loci": ["--loci", "7"], "pileup": ["--loci", "7", "--pileup", "100:1:0"]}
# kmer_read_vf6: without the two switches of nk10 alone, with the geometries its tests use on its input
VF6_OPTIONS = {w: o for w, o in OPTIONS.items() if w not in ("fragments", "fragment_votes")}
VF6_OPTIONS.update(segment_votes=["--segment-votes", "50:25"], loci=["--loci", "5"], pileup=["--loci", "5", "--pileup", "50:1:0"])
SAMPLES = ("S1", "S2")
JOBS = ("jobA", "jobB")


def file_of(word):
    return "_seen.bin" if word == "seen" else "_%s.txt" % word


def together(options, words):
    """(--loci may come twice, with the same value)"""
    return RULE + [o for w in words for o in options[w]]


def run_nk10(prog, fq, cwd, extra):
    """run_dir, the files that are no .txt included (the seen file) -> (stdout, {name: bytes} of everything but the inputs)"""
    for f in os.listdir(fq):
        if f.endswith(".bin"):
            os.remove(os.path.join(fq, f))
    out, files = run_dir(prog, fq, cwd, extra)
    for f in os.listdir(fq):
        if not f.endswith((".txt", ".fastq.gz")):
            files[f] = open(os.path.join(fq, f), "rb").read()
    return out, files


def count_sum(result_text):
    return sum(int(l.split(b",")[1]) for l in result_text.splitlines())


@pytest.fixture(scope="module")
def all_together(nk10, gold_dir, tmp_path_factory):  # noqa: F811
    cwd = str(tmp_path_factory.mktemp("all_side_options"))
    src, fq, parent = stage_small(gold_dir, cwd)
    out, files = run_nk10(nk10, fq, cwd, together(OPTIONS, OPTIONS) + ["--devices", "0,0", "--samples-in-flight", "2", "--batch-reads", "7"])
    for p in SAMPLES:  # the comparisons below compare something
        for w in ("hits", "segments", "segment_votes", "loci"):
            assert files[p + file_of(w)].count(b"\n") >= 1, (p, w)
        pileup = files[p + "_pileup.txt"].splitlines()
        assert pileup[0].startswith(b"#") and len(pileup) >= 2, p
        for w in ("confident", "fragments", "votes", "fragment_votes"):
            assert count_sum(files[p + file_of(w)]) > 0, (p, w)
    return fq, cwd, out, files


@pytest.mark.parametrize("word", list(OPTIONS))
def test_nk10_each_side_file_is_what_its_option_alone_writes(nk10, all_together, word):  # noqa: F811
    fq, cwd, all_out, all_files = all_together
    assert sorted(all_files) == sorted(p + s for p in SAMPLES for s in ["_result.txt", "_reads.txt"] + [file_of(w) for w in OPTIONS])
    out, files = run_nk10(nk10, fq, cwd, together(OPTIONS, [word]))
    assert out == all_out
    for p in SAMPLES:
        for s in (file_of(word), "_result.txt", "_reads.txt"):
            assert files[p + s] == all_files[p + s], p + s


def test_vf6_each_side_file_is_what_its_option_alone_writes(bins, tmp_path):  # noqa: F811
    """a job's files are read one after the other: its outputs span several calls of the read pipeline"""
    cwd = str(tmp_path)
    setup_vf6(cwd)
    jdir = os.path.join(cwd, "J")

    def run(words, extra):
        for f in os.listdir(jdir):
            if f != "J.txt":
                os.remove(os.path.join(jdir, f))
        r = subprocess.run([bins["kmer_read_vf6"], "-name", "DB", "-jname", "J", "--log2-slots", "22"] + together(VF6_OPTIONS, words) + extra,
                           cwd=cwd, check=True, stdout=subprocess.PIPE)
        return r.stdout, {f: open(os.path.join(jdir, f), "rb").read() for f in os.listdir(jdir) if f != "J.txt"}

    all_out, all_files = run(list(VF6_OPTIONS), ["--devices", "0,0", "--batch-reads", "7"])
    rule_out, rule_files = run(["confident"], [])  # (the rule alone)
    assert set(all_files) == set(rule_files) | {job + file_of(w) for job in JOBS for w in VF6_OPTIONS} and all_out == rule_out
    for job in JOBS:
        for w in ("hits", "segments", "segment_votes", "loci", "pileup"):
            assert all_files[job + file_of(w)].count(b"\n") >= (2 if w == "pileup" else 1), (job, w)
    for w in VF6_OPTIONS:
        out, files = (rule_out, rule_files) if w == "confident" else run([w], [])
        assert out == all_out, w
        assert set(files) == set(rule_files) | {job + file_of(x) for job in JOBS for x in ([w, "loci"] if w == "pileup" else [w])}, w
        for f in files:
            assert files[f] == all_files[f], (w, f)
