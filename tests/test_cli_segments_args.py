"""--segments LEN[:STEP] of the three front-ends without a GPU: malformed values are usage errors (also with --dry-run,
which otherwise ignores the option: no segments file), and the C ABI of the feature is declared and bound."""
import os
import re
import subprocess

import pytest

from helpers import ROOT
from kmer_id_amd import _lib
from test_cli_host import make_db_dir, nk10  # noqa: F401  (nk10: fixture)
from test_cli_vf6_m3 import bins, setup_m3, setup_vf6  # noqa: F401  (bins: fixture)

BAD = [["--segments", v] for v in ("0", "10:0", "10:11", "x", "10:", ":5", "-5", "10:5:2", "2048:1", "2147483648")] + [["--segments"]]
GOOD = [["--segments", v] for v in ("1000", "1000:500", "64:64", "1024:1")]
FUNCTIONS = {"kid_db_read_segments": 14, "kid_db_read_segments_fastq": 13, "kid_db_read_segments_device": 19, "kid_db_read_segments_time": 4}


def segments_files(top):
    return [f for _, _, fs in os.walk(top) for f in fs if "segments" in f]


def test_nk10_option_under_dry_run(nk10, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    make_db_dir(cwd, 2e-5)
    fq = os.path.join(cwd, "fq")
    os.makedirs(fq)
    dump = os.path.join(cwd, "dry.txt")
    for bad in BAD:
        r = subprocess.run([nk10, fq + "/", "--dry-run", dump] + bad, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 2 and b"--segments" in r.stderr, bad
    plain = subprocess.run([nk10, fq + "/", "--dry-run", dump], cwd=cwd, stdout=subprocess.PIPE, check=True).stdout
    ref = open(dump, "rb").read()
    for good in GOOD:
        r = subprocess.run([nk10, fq + "/", "--dry-run", dump] + good, cwd=cwd, stdout=subprocess.PIPE, check=True)
        assert r.stdout == plain and open(dump, "rb").read() == ref and not segments_files(cwd), good


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
        assert r.returncode == 2 and b"--segments" in r.stderr, bad
    plain = subprocess.run([bins[prog]] + args + ["--dry-run", dump], cwd=cwd, stdout=subprocess.PIPE, check=True).stdout
    ref = open(dump, "rb").read()
    for good in GOOD:
        r = subprocess.run([bins[prog]] + args + ["--dry-run", dump] + good, cwd=cwd, stdout=subprocess.PIPE, check=True)
        assert r.stdout == plain and open(dump, "rb").read() == ref and not segments_files(cwd), good


def test_the_header_declares_and_the_binding_binds_the_four_functions():
    header = open(os.path.join(ROOT, "include", "kmer_id_amd.h")).read()
    for name, nargs in FUNCTIONS.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == nargs, name
    assert re.search(r"typedef struct kid_segment \{\s*uint32_t pos, n_pos, final, confident, n_kmers, n_hits, s_final, s_confident;\s*\} kid_segment;", header)
    assert re.search(r"#define\s+KID_SEGMENT_MAX_OVERLAP\s+1024u", header)
    from kmer_id_amd.api import SEGMENT_DTYPE
    assert SEGMENT_DTYPE.itemsize == 32 and SEGMENT_DTYPE.names == ("pos", "n_pos", "final", "confident", "n_kmers", "n_hits", "s_final", "s_confident")
    lib = _lib.lib_path()
    if os.path.exists(lib):  # the built library exports them (nm: no device needed)
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, check=True).stdout.decode()
        for name in FUNCTIONS:
            assert re.search(r" T %s\b" % name, syms), name
