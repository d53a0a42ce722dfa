"""--depth of the three front-ends without a GPU: a flag without a value that --dry-run ignores (the same stdout, the same
dump, no depth file), and the C ABI of the feature is declared, bound with the declared arity and exported."""
import os
import re
import subprocess

import pytest

from helpers import ROOT
from kmer_id_amd import _lib
from test_cli_host import make_db_dir, nk10  # noqa: F401  (nk10: fixture)
from test_cli_vf6_m3 import bins, setup_m3, setup_vf6  # noqa: F401  (bins: fixture)

FUNCTIONS = {"kid_sample_depth_export": 5, "kid_sample_depth_add": 5, "kid_sample_depth_spectrum": 5, "kid_sample_depth_spectrum_merged": 6}
WAYS = [["--depth"], ["--depth", "--min-hits", "2", "--confidence", "0.02"], ["--hits", "--depth", "--depth"]]


def depth_files(top):
    return [f for _, _, fs in os.walk(top) for f in fs if "depth" in f]


def test_nk10_depth_under_dry_run(nk10, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    make_db_dir(cwd, 2e-5)
    fq = os.path.join(cwd, "fq")
    os.makedirs(fq)
    dump = os.path.join(cwd, "dry.txt")
    plain = subprocess.run([nk10, fq + "/", "--dry-run", dump], cwd=cwd, stdout=subprocess.PIPE, check=True).stdout
    ref = open(dump, "rb").read()
    for way in WAYS:
        r = subprocess.run([nk10, fq + "/"] + way[:1] + ["--dry-run", dump] + way[1:], cwd=cwd, stdout=subprocess.PIPE, check=True)
        assert r.stdout == plain and open(dump, "rb").read() == ref and not depth_files(cwd), way
    # it takes no value: the word behind it is read as an argument of its own
    r = subprocess.run([nk10, fq + "/", "--dry-run", dump, "--depth", "--no-such-option"], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 2
    r = subprocess.run([nk10, fq + "/", "--depth", "--dry-run", dump, "--min-hits"], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 2 and b"--min-hits" in r.stderr


@pytest.mark.parametrize("prog", ["kmer_read_vf6", "kmer_read_m3"])
def test_vf6_m3_depth_under_dry_run(bins, tmp_path, prog):  # noqa: F811
    cwd = str(tmp_path)
    if prog == "kmer_read_vf6":
        setup_vf6(cwd)
        args = ["-name", "DB", "-jname", "J"]
    else:
        src, params, wd = setup_m3(cwd)
        f1, f2 = sorted(params["runs"].values())[0]
        args = ["-wdir", wd, "-f1", wd + f1, "-f2", (wd + f2) if f2 != "none" else "none"]
    dump = os.path.join(cwd, "dry.txt")
    plain = subprocess.run([bins[prog]] + args + ["--dry-run", dump], cwd=cwd, stdout=subprocess.PIPE, check=True).stdout
    ref = open(dump, "rb").read()
    for way in WAYS[:2]:
        r = subprocess.run([bins[prog]] + args + way[:1] + ["--dry-run", dump] + way[1:], cwd=cwd, stdout=subprocess.PIPE, check=True)
        assert r.stdout == plain and open(dump, "rb").read() == ref and not depth_files(cwd), way


def test_the_header_declares_and_the_binding_binds_the_depth_functions():
    header = open(os.path.join(ROOT, "include", "kmer_id_amd.h")).read()
    assert re.search(r"#define\s+KID_OPT_ENTRY_DEPTH\s+4\b", header) and _lib.KID_OPT_ENTRY_DEPTH == 4
    for name, arity in FUNCTIONS.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, name
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == arity == m.group(1).count(",") + 1, name
    lib = _lib.lib_path()
    if os.path.exists(lib):  # the built library exports them (nm: no device needed)
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, check=True).stdout.decode()
        for name in FUNCTIONS:
            assert re.search(r" T %s\b" % name, syms), name
