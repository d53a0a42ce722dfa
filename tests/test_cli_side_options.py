"""The side options of the three front-ends given together, without a GPU: under --dry-run good values change nothing and
leave no side file, and of two malformed options the one diagnosed is decided by a fixed order (--min-hits /
--confidence, then --min-base-quality / --low-complexity, then --segments, --segment-votes, --loci, --pileup), whatever
their order on the command line; of two of the same step, the first on the command line."""
import os
import subprocess

import pytest

from test_cli_host import make_db_dir, nk10  # noqa: F401  (nk10: fixture)
from test_cli_vf6_m3 import bins, setup_m3, setup_vf6  # noqa: F401  (bins: fixture)

# every side option with a good value; the two switches of nk10 alone apart
ALL_GOOD = ["--hits", "--min-hits", "2", "--confidence", "0.02", "--min-base-quality", "20", "--low-complexity", "20", "--segments", "1000:500",
            "--segment-votes", "500:250", "--loci", "7", "--pileup", "100:2:1", "--depth", "--seen", "--votes"]
NK10_ALONE = ["--fragments", "--fragment-votes"]
# (the one diagnosed, the other): each pair is given in both command-line orders.  The first two are older than the
# rest, which walk the order of diagnosis step by step.
PAIRS = [(["--min-hits", "x"], ["--segments", "0"]), (["--min-base-quality", "94"], ["--segments", "0"]),
         (["--min-hits", "x"], ["--min-base-quality", "94"]), (["--low-complexity", "1001"], ["--segments", "0"]),
         (["--segments", "0"], ["--segment-votes", "0"]), (["--segment-votes", "0"], ["--loci", "0"]), (["--loci", "0"], ["--pileup", "0"])]
WORDS = ("confident", "fragments", "votes", "fragment_votes", "depth", "seen", "hits", "segments", "segment_votes", "loci", "pileup")


def side_files(top):
    return [f for _, _, fs in os.walk(top) for f in fs if any(w in f for w in WORDS)]


@pytest.fixture(params=["nk10", "kmer_read_vf6", "kmer_read_m3"])
def front_end(request, nk10, bins, tmp_path):  # noqa: F811
    """(the command up to and including --dry-run FILE, its working directory, the dump's path)"""
    cwd = str(tmp_path)
    if request.param == "nk10":
        make_db_dir(cwd, 2e-5)
        os.makedirs(os.path.join(cwd, "fq"))
        cmd = [nk10, os.path.join(cwd, "fq") + "/"]
    elif request.param == "kmer_read_vf6":
        setup_vf6(cwd)
        cmd = [bins["kmer_read_vf6"], "-name", "DB", "-jname", "J"]
    else:
        src, params, wd = setup_m3(cwd)
        f1, f2 = sorted(params["runs"].values())[0]
        cmd = [bins["kmer_read_m3"], "-wdir", wd, "-f1", wd + f1, "-f2", (wd + f2) if f2 != "none" else "none"]
    dump = os.path.join(cwd, "dry.txt")
    return cmd + ["--dry-run", dump], cwd, dump


def test_all_four_together_change_nothing_under_dry_run(front_end):
    """(all four when it was written: every side option the front-end has)"""
    cmd, cwd, dump = front_end
    before = side_files(cwd)
    plain = subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, check=True).stdout
    ref = open(dump, "rb").read()
    os.remove(dump)
    good = ALL_GOOD + (NK10_ALONE if os.path.basename(cmd[0]) == "nk10" else [])
    r = subprocess.run(cmd + good, cwd=cwd, stdout=subprocess.PIPE, check=True)
    assert r.stdout == plain and open(dump, "rb").read() == ref
    assert side_files(cwd) == before == []


@pytest.mark.parametrize("first, other", PAIRS, ids=["min-hits+segments", "min-base-quality+segments", "min-hits+min-base-quality",
                                                     "low-complexity+segments", "segments+segment-votes", "segment-votes+loci", "loci+pileup"])
def test_of_two_malformed_options_the_fixed_order_decides(front_end, first, other):
    cmd, cwd, dump = front_end
    for args in (first + other, other + first):
        r = subprocess.run(cmd + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 2, args
        assert first[0].encode() in r.stderr and other[0].encode() not in r.stderr, (args, r.stderr)


def test_of_two_malformed_options_of_one_step_the_first_on_the_command_line_is_named(front_end):
    cmd, cwd, dump = front_end
    quality, complexity = ["--min-base-quality", "94"], ["--low-complexity", "1001"]
    for first, other in ((quality, complexity), (complexity, quality)):
        r = subprocess.run(cmd + first + other, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 2, first + other
        assert first[0].encode() in r.stderr and other[0].encode() not in r.stderr, (first + other, r.stderr)


def test_nk10_segments_as_the_last_word_needs_a_value(nk10, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    make_db_dir(cwd, 2e-5)
    os.makedirs(os.path.join(cwd, "fq"))
    r = subprocess.run([nk10, os.path.join(cwd, "fq") + "/", "--dry-run", os.path.join(cwd, "dry.txt"), "--segments"], cwd=cwd,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 2 and r.stderr == b"nk10: --segments needs a value\n"
