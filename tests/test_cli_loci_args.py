"""--loci W of the three front-ends without a GPU: a missing or malformed value is a usage error with exit code 2 and the
option's name on stderr (also with --dry-run, which otherwise ignores the option: no loci file, the same dump and
stdout), of several malformed options the earlier ones of the order are reported first, and the C ABI of the feature is
declared and bound."""
import os
import re
import subprocess

import pytest

from helpers import ROOT
from kmer_id_amd import _lib
from test_cli_host import make_db_dir, nk10  # noqa: F401  (nk10: fixture)
from test_cli_vf6_m3 import bins, setup_m3, setup_vf6  # noqa: F401  (bins: fixture)

OPT = "--loci"
BAD = [[OPT, v] for v in ("0", "x", "-5", "7x", "1:2", "", "+7", "1.5", "2147483648", "99999999999999999999")] + [[OPT]]
GOOD = [[OPT, v] for v in ("1", "7", "1000", "2147483647")] + [[OPT, "9", OPT, "5"], [OPT, "3", "--hits"]]
FUNCTIONS = {"kid_db_set_sites": 4, "kid_db_read_loci": 8, "kid_db_read_loci_fastq": 7, "kid_db_loci_from_hits_device": 8, "kid_db_read_loci_time": 4}
FIELDS = ("org", "strand", "n_chain", "n_org", "n_other", "n_hits", "n_kmers", "pos_first", "pos_last", "entry_first")


def side_files(top):
    return [f for _, _, fs in os.walk(top) for f in fs if "loci" in f]


def check_option(cmd, cwd, dump):
    for bad in BAD:
        r = subprocess.run(cmd + ["--dry-run", dump] + bad, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 2 and OPT.encode() in r.stderr, bad
    # the first of several errors: --segment-votes and the masks are reported in front of --loci, whatever their order in argv
    for both in ([OPT, "0", "--segment-votes", "x"], ["--segment-votes", "x", OPT, "0"], [OPT, "0", "--low-complexity", "x"]):
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
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == nargs, name
    assert re.search(r"typedef struct kid_locus \{\s*uint32_t org, strand, n_chain, n_org, n_other, n_hits /\* m \*/, n_kmers, pos_first, pos_last, "
                     r"entry_first;\s*\} kid_locus;", header)
    assert re.search(r"#define KID_LOCI_MAX_HITS 4096u", header) and re.search(r"#define KID_LOCI_MAX_ORGS \(1u << 24\)", header)
    from kmer_id_amd import LOCUS_DTYPE, KmerDB
    assert LOCUS_DTYPE.itemsize == 40 and LOCUS_DTYPE.names == FIELDS and all(LOCUS_DTYPE.fields[f][1] == 4 * i for i, f in enumerate(FIELDS))
    for method in ("set_sites", "clear_sites", "read_loci", "read_loci_fastq", "loci_from_hits_device", "read_loci_time"):
        assert callable(getattr(KmerDB, method)), method
    api = open(os.path.join(ROOT, "kmer_id_amd", "csrc", "kid_api_loci.h")).read()
    assert re.search(r"static_assert\(sizeof\(kid_locus\) == sizeof\(KidLocus\) && sizeof\(KidLocus\) == 40", api)
    lib = _lib.lib_path()
    if os.path.exists(lib):  # the built library exports them (nm: no device needed)
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, check=True).stdout.decode()
        for name in FUNCTIONS:
            assert re.search(r" T %s\b" % name, syms), name
