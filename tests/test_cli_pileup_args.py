"""--pileup W[:MIN_CHAIN[:MIN_MARGIN]] of the three front-ends without a GPU: a missing or malformed value (an empty part
and a fourth part too) is a usage error with exit code 2 and the option's name on stderr (also with --dry-run, which
otherwise ignores the option: no pileup file, the same dump and stdout), of several malformed options it is reported after
--loci, and the C ABI of the feature is declared and bound."""
import os
import re
import subprocess

import pytest

from helpers import ROOT
from kmer_id_amd import _lib
from read_calls import header_constant
from test_cli_host import make_db_dir, nk10  # noqa: F401  (nk10: fixture)
from test_cli_vf6_m3 import bins, setup_m3, setup_vf6  # noqa: F401  (bins: fixture)

OPT = "--pileup"
BAD = [[OPT, v] for v in ("0", "x", "-5", "7x", "", "+7", "1.5", "2147483648", "99999999999999999999", ":2", "7:", "7::1", "7:2:", "7:2:1:5",
                          "7:2:1:", "7:0", "7:4097", "7:2:4097", "7:x", "7:2:x", "7:-1", "7 :2", "0:2:1")] + [[OPT]]
GOOD = [[OPT, v] for v in ("1", "7", "1000", "2147483647", "7:1", "7:4096", "7:2:0", "7:2:4096", "2147483647:4096:4096")] + \
       [[OPT, "9", OPT, "5:3"], [OPT, "3", "--hits"], [OPT, "100:2:1", "--loci", "7"]]
FUNCTIONS = {"kid_pileup_create": 3, "kid_pileup_destroy": 1, "kid_pileup_info": 4, "kid_pileup_reset": 1, "kid_pileup_add": 5,
             "kid_pileup_add_device": 6, "kid_pileup_counts": 3, "kid_pileup_summary": 2, "kid_pileup_bins": 5, "kid_pileup_export": 3,
             "kid_pileup_merge": 5, "kid_pileup_time": 4}
FIELDS = ("n_placed", "span_bins", "bins_covered", "max_gap", "max_depth", "max_depth_bin", "max_starts", "max_starts_bin", "reserved", "depth_sum")


def side_files(top):
    return [f for _, _, fs in os.walk(top) for f in fs if "pileup" in f or "loci" in f]


def check_option(cmd, cwd, dump):
    for bad in BAD:
        r = subprocess.run(cmd + ["--dry-run", dump] + bad, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 2 and OPT.encode() in r.stderr, bad
    # the first of several errors: --loci, --segment-votes and the masks are reported in front of --pileup, whatever their order in argv
    for both in ([OPT, "0", "--loci", "x"], ["--loci", "0", OPT, "7:"], [OPT, "7:2:1:5", "--segment-votes", "x"], [OPT, "0", "--low-complexity", "x"]):
        r = subprocess.run(cmd + ["--dry-run", dump] + both, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        other = [w for w in both if w.startswith("--") and w != OPT][0]
        assert r.returncode == 2 and other.encode() in r.stderr and OPT.encode() not in r.stderr, both
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


def test_the_header_declares_and_the_binding_binds_the_functions():
    header = open(os.path.join(ROOT, "include", "kmer_id_amd.h")).read()
    for name, nargs in FUNCTIONS.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, header)
        assert m and re.sub(r"/\*.*?\*/", "", m.group(1)).count(",") + 1 == nargs, name
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == nargs, name
    assert re.search(r"typedef struct kid_pileup_rec \{\s*uint32_t n_placed, span_bins, bins_covered, max_gap, max_depth, max_depth_bin, max_starts, "
                     r"max_starts_bin, reserved;\s*uint64_t depth_sum;[^}]*\} kid_pileup_rec;", header)
    from kmer_id_amd import PILEUP_DTYPE, KmerDB, Pileup
    assert PILEUP_DTYPE.itemsize == 48 and PILEUP_DTYPE.names == FIELDS
    assert [PILEUP_DTYPE.fields[f][1] for f in FIELDS] == [4 * i for i in range(9)] + [40]
    assert callable(KmerDB.pileup)
    for method in ("add", "add_device", "counts", "summary", "bins", "export", "merge", "reset", "time", "close", "__enter__", "__exit__"):
        assert callable(getattr(Pileup, method)), method
    api = open(os.path.join(ROOT, "kmer_id_amd", "csrc", "kid_api_pileup.h")).read()
    assert re.search(r"static_assert\(sizeof\(kid_pileup_rec\) == 48 && offsetof\(kid_pileup_rec, reserved\) == 32 && offsetof\(kid_pileup_rec, depth_sum\) == 40", api)
    assert header_constant("kid_pileup.hip.h", "KID_PILEUP_REC_WORDS") * 4 == PILEUP_DTYPE.itemsize
    assert header_constant("kid_pileup.hip.h", "KID_PILEUP_SCAN_TILE") >= 64
    lib = _lib.lib_path()
    if os.path.exists(lib):  # the built library exports them (nm: no device needed)
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, check=True).stdout.decode()
        for name in FUNCTIONS:
            assert re.search(r" T %s\b" % name, syms), name
