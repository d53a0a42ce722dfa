"""--segment-votes LEN[:STEP] of the three front-ends without a GPU: malformed values are usage errors (also with
--dry-run, which otherwise ignores the option: no segment_votes file), of several malformed options --segments is
reported first, and the C ABI of the feature is declared and bound."""
import os
import re
import subprocess

import pytest

from helpers import ROOT
from kmer_id_amd import _lib
from test_cli_host import make_db_dir, nk10  # noqa: F401  (nk10: fixture)
from test_cli_vf6_m3 import bins, setup_m3, setup_vf6  # noqa: F401  (bins: fixture)

OPT = "--segment-votes"
BAD = [[OPT, v] for v in ("0", "10:0", "10:11", "x", "10:", ":5", "-5", "10:5:2", "2048:1", "2147483648")] + [[OPT]]
GOOD = [[OPT, v] for v in ("1000", "1000:500", "64:64", "1024:1")] + [[OPT, "100:50", "--segments", "64"], ["--segments", "1000:500", OPT, "7"]]
FUNCTIONS = {"kid_db_read_segment_votes": 14, "kid_db_read_segment_votes_fastq": 13, "kid_db_read_segment_votes_device": 19,
             "kid_db_read_segment_votes_time": 4}
FIELDS = ("pos", "n_pos", "call", "confident", "n_kmers", "n_hits", "p_best", "n_best", "s_call", "s_confident")


def side_files(top):
    return [f for _, _, fs in os.walk(top) for f in fs if "segment" in f]


def check_option(cmd, cwd, dump):
    for bad in BAD:
        r = subprocess.run(cmd + ["--dry-run", dump] + bad, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 2 and OPT.encode() in r.stderr, bad
    # the first of several errors: --segments is reported in front of --segment-votes, whatever their order in argv
    for both in ([OPT, "0", "--segments", "x"], ["--segments", "x", OPT, "0"]):
        r = subprocess.run(cmd + ["--dry-run", dump] + both, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 2 and b"--segments" in r.stderr and OPT.encode() not in r.stderr, both
    r = subprocess.run(cmd + ["--dry-run", dump, OPT, "0", "--low-complexity", "x"], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 2 and b"--low-complexity" in r.stderr and OPT.encode() not in r.stderr
    plain = subprocess.run(cmd + ["--dry-run", dump], cwd=cwd, stdout=subprocess.PIPE, check=True).stdout
    ref = open(dump, "rb").read()
    for good in GOOD:
        r = subprocess.run(cmd + ["--dry-run", dump] + good, cwd=cwd, stdout=subprocess.PIPE, check=True)
        assert r.stdout == plain and open(dump, "rb").read() == ref and not side_files(cwd), good


def test_nk10_option_under_dry_run(nk10, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    make_db_dir(cwd, 2e-5)
    fq = os.path.join(cwd, "fq")
    os.makedirs(fq)
    check_option([nk10, fq + "/"], cwd, os.path.join(cwd, "dry.txt"))


@pytest.mark.parametrize("prog", ["kmer_read_vf6", "kmer_read_m3"])
def test_vf6_m3_option_under_dry_run(bins, tmp_path, prog):  # noqa: F811
    cwd = str(tmp_path)
    if prog == "kmer_read_vf6":
        setup_vf6(cwd)
        args = ["-name", "DB", "-jname", "J"]
    else:
        src, params, wd = setup_m3(cwd)
        f1, f2 = sorted(params["runs"].values())[0]
        args = ["-wdir", wd, "-f1", wd + f1, "-f2", (wd + f2) if f2 != "none" else "none"]
    check_option([bins[prog]] + args, cwd, os.path.join(cwd, "dry.txt"))


def test_the_header_declares_and_the_binding_binds_the_four_functions():
    header = open(os.path.join(ROOT, "include", "kmer_id_amd.h")).read()
    for name, nargs in FUNCTIONS.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == nargs, name
        # argument for argument the read_segments form
        assert _lib.PROTOTYPES[name] == _lib.PROTOTYPES[name.replace("segment_votes", "segments")], name
    assert re.search(r"typedef struct kid_segment_vote \{\s*uint32_t %s;\s*\} kid_segment_vote;" % ", ".join(FIELDS), header)
    from kmer_id_amd import SEGMENT_VOTE_DTYPE, KmerDB
    from kmer_id_amd.api import VOTE_DTYPE
    assert SEGMENT_VOTE_DTYPE.itemsize == 40 and SEGMENT_VOTE_DTYPE.names == FIELDS and SEGMENT_VOTE_DTYPE.names[2:] == VOTE_DTYPE.names
    assert all(SEGMENT_VOTE_DTYPE.fields[f][1] == 4 * i for i, f in enumerate(FIELDS))
    for method in ("read_segment_votes", "read_segment_votes_fastq", "read_segment_votes_device", "read_segment_votes_time"):
        assert callable(getattr(KmerDB, method)), method
    api = open(os.path.join(ROOT, "kmer_id_amd", "csrc", "kid_api_segment_votes.h")).read()
    assert re.search(r"static_assert\(sizeof\(kid_segment_vote\) == sizeof\(KidSegmentVote\) && sizeof\(KidSegmentVote\) == 40", api)
    lib = _lib.lib_path()
    if os.path.exists(lib):  # the built library exports them (nm: no device needed)
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, check=True).stdout.decode()
        for name in FUNCTIONS:
            assert re.search(r" T %s\b" % name, syms), name
