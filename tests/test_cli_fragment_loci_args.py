"""--fragment-loci W[:MAX_SPAN] without a GPU: a missing or malformed value is a usage error with exit code 2 and the option's
name on stderr (also with --dry-run, which otherwise ignores the option: no fragment_loci file, the same dump and stdout);
of several malformed options it is reported behind --pileup; kmer_read_vf6 and kmer_read_m3 refuse it, and so does nk10
with --fasta; the C ABI of the feature is declared and bound."""
import os
import re
import subprocess

import pytest

from helpers import ROOT
from kmer_id_amd import _lib
from test_cli_host import make_db_dir, nk10  # noqa: F401  (nk10: fixture)
from test_cli_vf6_m3 import bins, setup_m3, setup_vf6  # noqa: F401  (bins: fixture)

OPT = "--fragment-loci"
BAD = [[OPT, v] for v in ("0", "x", "-5", "7x", "", ":", "1:", ":5", "1:2:3", "1:x", "1:-1", "+7", "1.5", "2147483648", "1:2147483648", "0:5",
                          "99999999999999999999", "1:99999999999999999999")] + [[OPT]]
GOOD = [[OPT, v] for v in ("1", "7", "1:0", "1:1000", "100:5000", "2147483647", "2147483647:2147483647")] + [[OPT, "9", OPT, "5:3"], [OPT, "3", "--hits"]]
FUNCTIONS = {"kid_db_read_fragment_loci": 9, "kid_db_read_fragment_loci_fastq": 11, "kid_db_fragment_loci_from_hits_device": 9,
             "kid_db_read_fragment_loci_time": 4, "kid_pileup_add_fragments": 6, "kid_pileup_add_fragments_device": 7}
FIELDS = ("org", "orient", "mates", "n_chain", "n_chain_1", "n_chain_2", "n_org", "n_other", "n_hits", "n_kmers", "lo", "hi", "pos_first_1",
          "pos_last_1", "pos_first_2", "pos_last_2")


def side_files(top):
    return [f for _, _, fs in os.walk(top) for f in fs if "fragment_loci" in f]


def run(cmd, cwd):
    return subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


@pytest.fixture()
def nk10_cmd(nk10, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    make_db_dir(cwd, 2e-5)
    fq = os.path.join(cwd, "fq")
    os.makedirs(fq)
    return [nk10, fq + "/", "--dry-run", os.path.join(cwd, "dry.txt")], cwd


def test_every_malformed_value_is_a_usage_error(nk10_cmd):
    cmd, cwd = nk10_cmd
    for bad in BAD:
        r = run(cmd + bad, cwd)
        assert r.returncode == 2 and OPT.encode() in r.stderr, bad


def test_it_is_reported_behind_the_options_before_it(nk10_cmd):
    cmd, cwd = nk10_cmd
    for both in ([OPT, "0", "--pileup", "x"], ["--pileup", "x", OPT, "0"], [OPT, "1:", "--loci", "0"], [OPT, "0", "--low-complexity", "x"]):
        r = run(cmd + both, cwd)
        other = [w for w in both if w.startswith("--") and w != OPT][0]
        assert r.returncode == 2 and other.encode() in r.stderr and OPT.encode() not in r.stderr, both


def test_good_values_change_nothing_and_leave_no_file(nk10_cmd):
    cmd, cwd = nk10_cmd
    plain = subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, check=True).stdout
    ref = open(cmd[-1], "rb").read()
    for good in GOOD:
        r = subprocess.run(cmd + good, cwd=cwd, stdout=subprocess.PIPE, check=True)
        assert r.stdout == plain and open(cmd[-1], "rb").read() == ref and not side_files(cwd), good


def test_not_with_fasta(nk10_cmd):
    cmd, cwd = nk10_cmd
    r = run(cmd + ["--fasta", OPT, "1"], cwd)
    assert r.returncode == 2 and OPT.encode() in r.stderr and b"--fasta" in r.stderr
    assert run(cmd + ["--fasta"], cwd).returncode == 0


@pytest.mark.parametrize("prog", ["kmer_read_vf6", "kmer_read_m3"])
def test_vf6_and_m3_refuse_it(bins, tmp_path, prog):  # noqa: F811
    cwd = str(tmp_path)
    if prog == "kmer_read_vf6":
        setup_vf6(cwd)
        args = ["-name", "DB", "-jname", "J"]
    else:
        src, params, wd = setup_m3(cwd)
        f1, f2 = sorted(params["runs"].values())[0]
        args = ["-wdir", wd, "-f1", wd + f1, "-f2", (wd + f2) if f2 != "none" else "none"]
    cmd = [bins[prog]] + args + ["--dry-run", os.path.join(cwd, "dry.txt")]
    assert run(cmd, cwd).returncode == 0
    for value in (["1"], ["7:500"], ["x"], []):
        r = run(cmd + [OPT] + value, cwd)
        assert r.returncode == 2 and OPT.encode() in r.stderr and not side_files(cwd), value
    r = run(cmd + [OPT, "1"], cwd)
    assert b"nk10 alone" in r.stderr


def test_the_header_declares_and_the_binding_binds_the_functions():
    header = open(os.path.join(ROOT, "include", "kmer_id_amd.h")).read()
    for name, nargs in FUNCTIONS.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == nargs, name
    m = re.search(r"typedef struct kid_fragment_locus \{(.*?)\} kid_fragment_locus;", header, re.S)
    names = re.sub(r"/\*.*?\*/", "", m.group(1)).replace("uint32_t", "").replace(";", "").replace("\n", " ")
    assert tuple(w.strip() for w in names.split(",")) == FIELDS
    from kmer_id_amd import FRAGMENT_LOCUS_DTYPE, KmerDB, Pileup
    assert FRAGMENT_LOCUS_DTYPE.itemsize == 64 and FRAGMENT_LOCUS_DTYPE.names == FIELDS
    assert all(FRAGMENT_LOCUS_DTYPE.fields[f][1] == 4 * i for i, f in enumerate(FIELDS))
    for method in ("read_fragment_loci", "read_fragment_loci_fastq", "fragment_loci_from_hits_device", "read_fragment_loci_time"):
        assert callable(getattr(KmerDB, method)), method
    assert callable(Pileup.add_fragments) and callable(Pileup.add_fragments_device)
    api = open(os.path.join(ROOT, "kmer_id_amd", "csrc", "kid_api_fragment_loci.h")).read()
    assert re.search(r"static_assert\(sizeof\(kid_fragment_locus\) == sizeof\(KidFragmentLocus\) && sizeof\(KidFragmentLocus\) == 64", api)
