"""--low-complexity of the three front-ends without a GPU: a missing or malformed value is a usage error (exit code 2,
one line on stderr) also with --dry-run, which otherwise ignores the option; the C ABI of the feature is declared and
bound."""
import os
import re
import subprocess

import pytest

from helpers import ROOT
from kmer_id_amd import _lib
from test_cli_host import nk10  # noqa: F401  (fixture)
from test_cli_support_args import stage_nk10
from test_cli_vf6_m3 import bins, setup_m3, setup_vf6  # noqa: F401  (bins: fixture)

BAD = [["--low-complexity"], ["--low-complexity", "-1"], ["--low-complexity", "1001"], ["--low-complexity", "2.5"],
       ["--low-complexity", "abc"], ["--low-complexity", "99999999999999999999"], ["--low-complexity", ""], ["--low-complexity", "20x"],
       ["--low-complexity", "+20"]]
GOOD = [["--low-complexity", "20"], ["--low-complexity", "0"], ["--low-complexity", "1000"],
        ["--low-complexity", "20", "--min-base-quality", "20", "--hits", "--min-hits", "2"]]
FUNCTIONS = {"kid_sample_lowc_bases": 2, "kid_lowc_batch": 7, "kid_lowc_batch_device": 7}


def check(prog, args, cwd):
    dump = os.path.join(cwd, "dry.txt")
    for bad in BAD:
        r = subprocess.run([prog] + args + ["--dry-run", dump] + bad, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 2, bad
        assert b"--low-complexity" in r.stderr and r.stderr.count(b"\n") == 1, (bad, r.stderr)
    plain = subprocess.run([prog] + args + ["--dry-run", dump], cwd=cwd, stdout=subprocess.PIPE, check=True).stdout
    ref = open(dump, "rb").read()
    before = sorted(f for _, _, fs in os.walk(cwd) for f in fs)
    for good in GOOD:
        r = subprocess.run([prog] + args + ["--dry-run", dump] + good, cwd=cwd, stdout=subprocess.PIPE, check=True)
        assert r.stdout == plain and open(dump, "rb").read() == ref, good
        assert sorted(f for _, _, fs in os.walk(cwd) for f in fs) == before, good


def test_nk10_option_under_dry_run(nk10, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    fq = stage_nk10(cwd)
    check(nk10, [fq + "/"], cwd)


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
    check(bins[prog], args, cwd)


def test_the_header_declares_and_the_binding_binds_the_feature():
    header = open(os.path.join(ROOT, "include", "kmer_id_amd.h")).read()
    assert re.search(r"#define\s+KID_OPT_LOW_COMPLEXITY\s+5\b", header) and _lib.KID_OPT_LOW_COMPLEXITY == 5
    assert re.search(r"#define\s+KID_DB_OPT_LOW_COMPLEXITY\s+2\b", header) and _lib.KID_DB_OPT_LOW_COMPLEXITY == 2
    for name, nargs in FUNCTIONS.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert len(_lib.PROTOTYPES[name][1]) == nargs, name
    lib = _lib.lib_path()
    if os.path.exists(lib):  # the built library exports them (nm: no device needed)
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, check=True).stdout.decode()
        for name in FUNCTIONS:
            assert re.search(r" T %s\b" % name, syms), name
