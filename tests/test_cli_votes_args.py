"""--votes of the three front-ends without a GPU: it is a flag without a value (the word behind it is not taken), it is
checked together with the options whose rule it follows -- a malformed --min-hits / --confidence beside it is a usage
error, also with --dry-run -- and is otherwise ignored with --dry-run: no votes file, the same dump and stdout; and the C
ABI of the feature is declared, bound and exported."""
import os
import re
import subprocess

import pytest

from helpers import ROOT
from kmer_id_amd import VOTE_DTYPE, _lib
from test_cli_host import make_db_dir, nk10  # noqa: F401  (nk10: fixture)
from test_cli_vf6_m3 import bins, setup_m3, setup_vf6  # noqa: F401  (bins: fixture)

BAD = [["--votes", "--confidence", "1.5"], ["--min-hits", "-1", "--votes"], ["--votes", "--confidence"], ["--votes", "--min-base-quality", "94"],
       ["--votes", "--segments", "0"]]
GOOD = [["--votes"], ["--votes", "--votes"], ["--votes", "--min-hits", "2", "--confidence", "0.02"], ["--hits", "--votes", "--depth", "--seen"]]
FUNCTIONS = ["kid_db_read_votes", "kid_db_read_votes_fastq", "kid_db_votes_from_hits_device", "kid_db_read_votes_time"]


def votes_files(top):
    return [f for _, _, fs in os.walk(top) for f in fs if "votes" in f]


def test_nk10_option_under_dry_run(nk10, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    make_db_dir(cwd, 2e-5)
    fq = os.path.join(cwd, "fq")
    os.makedirs(fq)
    dump = os.path.join(cwd, "dry.txt")
    for bad in BAD:
        r = subprocess.run([nk10, fq + "/", "--dry-run", dump] + bad, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 2 and [w for w in bad if w != "--votes"][0].encode() in r.stderr, bad
    # the flag takes no value: a word behind it is nk10's next argument, and a second directory is one it does not expect
    r = subprocess.run([nk10, fq + "/", "--dry-run", dump, "--votes", "3"], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 2 and b"unexpected argument 3" in r.stderr
    plain = subprocess.run([nk10, fq + "/", "--dry-run", dump], cwd=cwd, stdout=subprocess.PIPE, check=True).stdout
    ref = open(dump, "rb").read()
    for good in GOOD + [["--votes", "--fasta"]]:
        r = subprocess.run([nk10, fq + "/", "--dry-run", dump] + good, cwd=cwd, stdout=subprocess.PIPE, check=True)
        assert r.stdout == plain and not votes_files(cwd), good
        assert "--fasta" in good or open(dump, "rb").read() == ref, good
    r = subprocess.run([nk10, fq + "/", "--dry-run", dump, "--votes"], cwd=cwd, stdout=subprocess.PIPE, check=True)  # the last word
    assert r.stdout == plain and open(dump, "rb").read() == ref


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
    dump = os.path.join(cwd, "dry.txt")
    for bad in BAD:
        r = subprocess.run([bins[prog]] + args + ["--dry-run", dump] + bad, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 2 and [w for w in bad if w != "--votes"][0].encode() in r.stderr, bad
    plain = subprocess.run([bins[prog]] + args + ["--dry-run", dump], cwd=cwd, stdout=subprocess.PIPE, check=True).stdout
    ref = open(dump, "rb").read()
    for good in GOOD[:3]:
        r = subprocess.run([bins[prog]] + args + ["--dry-run", dump] + good, cwd=cwd, stdout=subprocess.PIPE, check=True)
        assert r.stdout == plain and open(dump, "rb").read() == ref and not votes_files(cwd), good


def test_the_header_declares_and_the_binding_binds_the_four_functions():
    header = open(os.path.join(ROOT, "include", "kmer_id_amd.h")).read()
    for name in FUNCTIONS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.PROTOTYPES, name
    assert re.search(r"typedef struct kid_vote \{[^}]*\bcall, confident, n_kmers, n_hits\b[^}]*p_best[^}]*n_best[^}]*s_call[^}]*s_confident[^}]*\} kid_vote;",
                     header)
    assert VOTE_DTYPE.names == ("call", "confident", "n_kmers", "n_hits", "p_best", "n_best", "s_call", "s_confident") and VOTE_DTYPE.itemsize == 32
    for name, ref in zip(FUNCTIONS, ["kid_db_read_support", "kid_db_read_support_fastq", "kid_db_support_from_hits_device", "kid_db_read_support_time"]):
        assert _lib.PROTOTYPES[name] == _lib.PROTOTYPES[ref], name  # argument for argument the support quartet
    lib = _lib.lib_path()
    if os.path.exists(lib):  # the built library exports them (nm: no device needed)
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, check=True).stdout.decode()
        for name in FUNCTIONS:
            assert re.search(r" T %s\b" % name, syms), name
