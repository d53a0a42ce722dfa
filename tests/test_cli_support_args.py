"""--min-hits / --confidence of the three front-ends without a GPU: malformed values are usage errors (also with
--dry-run, which otherwise ignores the options: no confident file), and the C ABI of the feature is declared and bound."""
import os
import re
import subprocess

import pytest

from helpers import ROOT
from kmer_id_amd import _lib
from test_cli_host import make_db_dir, nk10  # noqa: F401  (nk10: fixture)
from test_cli_vf6_m3 import bins, setup_m3, setup_vf6  # noqa: F401  (bins: fixture)

BAD = [["--confidence", "1.5"], ["--confidence", "0.0005"], ["--confidence", "x"], ["--min-hits", "-1"], ["--confidence"],
       ["--min-hits", "3x"], ["--confidence", "0."], ["--confidence", "1.001"]]
GOOD = [["--min-hits", "2", "--confidence", "0.02"], ["--confidence", "1"], ["--confidence", "1.000"], ["--min-hits", "0"],
        ["--confidence", "0.5"]]
FUNCTIONS = ["kid_db_read_support", "kid_db_read_support_fastq", "kid_db_support_from_hits_device", "kid_db_read_support_time"]


def stage_nk10(cwd):
    make_db_dir(cwd, 2e-5)
    fq = os.path.join(cwd, "fq")
    os.makedirs(fq)
    return fq


def confident_files(top):
    return [f for _, _, fs in os.walk(top) for f in fs if "confident" in f]


def test_nk10_options_under_dry_run(nk10, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    fq = stage_nk10(cwd)
    dump = os.path.join(cwd, "dry.txt")
    for bad in BAD:
        r = subprocess.run([nk10, fq + "/", "--dry-run", dump] + bad, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 2 and bad[0].encode() in r.stderr, bad  # nk10's exit code for its other malformed options
    # (the same code as for an argument nk10 does not know)
    assert subprocess.run([nk10, fq + "/", "--no-such-option"], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE).returncode == 2
    plain = subprocess.run([nk10, fq + "/", "--dry-run", dump], cwd=cwd, stdout=subprocess.PIPE, check=True).stdout
    ref = open(dump, "rb").read()
    for good in GOOD:
        r = subprocess.run([nk10, fq + "/", "--dry-run", dump] + good, cwd=cwd, stdout=subprocess.PIPE, check=True)
        assert r.stdout == plain and open(dump, "rb").read() == ref and not confident_files(cwd), good


@pytest.mark.parametrize("prog", ["kmer_read_vf6", "kmer_read_m3"])
def test_vf6_m3_options_under_dry_run(bins, tmp_path, prog):  # noqa: F811
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
        assert r.returncode == 2 and bad[0].encode() in r.stderr, bad
    plain = subprocess.run([bins[prog]] + args + ["--dry-run", dump], cwd=cwd, stdout=subprocess.PIPE, check=True).stdout
    ref = open(dump, "rb").read()
    for good in GOOD[:2]:
        r = subprocess.run([bins[prog]] + args + ["--dry-run", dump] + good, cwd=cwd, stdout=subprocess.PIPE, check=True)
        assert r.stdout == plain and open(dump, "rb").read() == ref and not confident_files(cwd), good


def test_the_header_declares_and_the_binding_binds_the_four_functions():
    header = open(os.path.join(ROOT, "include", "kmer_id_amd.h")).read()
    for name in FUNCTIONS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.PROTOTYPES, name
    assert re.search(r"typedef struct kid_support \{[^}]*\bfinal, confident, n_kmers, n_hits\b[^}]*s_final[^}]*s_confident[^}]*\} kid_support;", header)
    assert len(_lib.PROTOTYPES["kid_db_read_support"][1]) == 10 and len(_lib.PROTOTYPES["kid_db_read_support_fastq"][1]) == 9
    assert len(_lib.PROTOTYPES["kid_db_support_from_hits_device"][1]) == 9 and len(_lib.PROTOTYPES["kid_db_read_support_time"][1]) == 4
    lib = _lib.lib_path()
    if os.path.exists(lib):  # the built library exports them (nm: no device needed)
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, check=True).stdout.decode()
        for name in FUNCTIONS:
            assert re.search(r" T %s\b" % name, syms), name
