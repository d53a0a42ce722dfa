"""--fragments and --block-bytes of nk10 without a GPU: --fragments is a flag without a value that --dry-run checks and then
ignores (the same stdout, the same dump, no fragments file), it is refused with --fasta and by the two front-ends that
read their inputs one file after the other, --block-bytes takes digits >= 1; and the C ABI of the feature is declared,
bound with the declared arity and exported."""
import os
import re
import subprocess

import pytest

from helpers import ROOT
from kmer_id_amd import _lib
from test_cli_host import make_db_dir, nk10  # noqa: F401  (nk10: fixture)
from test_cli_vf6_m3 import bins, setup_m3, setup_vf6  # noqa: F401  (bins: fixture)

FUNCTIONS = {"kid_db_read_fragments": 10, "kid_db_read_fragments_fastq": 12, "kid_db_fragments_from_hits_device": 9, "kid_db_read_fragments_time": 4}


def fragment_files(top):
    return [f for _, _, fs in os.walk(top) for f in fs if "fragments" in f]


def run(cmd, cwd):
    return subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def test_nk10_fragments_and_block_bytes_under_dry_run(nk10, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    make_db_dir(cwd, 2e-5)
    fq = os.path.join(cwd, "fq")
    os.makedirs(fq)
    dump = os.path.join(cwd, "dry.txt")
    plain = subprocess.run([nk10, fq + "/", "--dry-run", dump], cwd=cwd, stdout=subprocess.PIPE, check=True).stdout
    ref = open(dump, "rb").read()
    for way in (["--fragments"], ["--fragments", "--min-hits", "2", "--confidence", "0.025"], ["--fragments", "--block-bytes", "32768"],
                ["--block-bytes", "1"]):
        cut = 1 if way[0] == "--fragments" else 0  # (a flag in front of --dry-run, the options with a value behind it)
        r = subprocess.run([nk10, fq + "/"] + way[:cut] + ["--dry-run", dump] + way[cut:], cwd=cwd, stdout=subprocess.PIPE, check=True)
        assert r.stdout == plain and open(dump, "rb").read() == ref and not fragment_files(cwd), way
    # it takes no value: the word behind it is read as an argument of its own
    assert run([nk10, fq + "/", "--dry-run", dump, "--fragments", "--no-such-option"], cwd).returncode == 2


@pytest.mark.parametrize("words", [["--fasta", "--fragments"], ["--block-bytes", "0"], ["--block-bytes", "x"], ["--block-bytes", "12k"],
                                   ["--block-bytes"]])
def test_nk10_usage_errors(nk10, tmp_path, words):  # noqa: F811
    cwd = str(tmp_path)
    make_db_dir(cwd, 2e-5)
    fq = os.path.join(cwd, "fq")
    os.makedirs(fq)
    r = run([nk10, fq + "/", "--dry-run", os.path.join(cwd, "dry.txt")] + words, cwd)
    assert r.returncode == 2 and (b"--block-bytes" if "--block-bytes" in words else b"--fragments") in r.stderr, r.stderr
    assert r.stderr.count(b"\n") == 1 and not os.path.exists(os.path.join(cwd, "dry.txt"))


@pytest.mark.parametrize("prog", ["kmer_read_vf6", "kmer_read_m3"])
def test_vf6_and_m3_refuse_fragments(bins, tmp_path, prog):  # noqa: F811
    cwd = str(tmp_path)
    if prog == "kmer_read_vf6":
        setup_vf6(cwd)
        args = ["-name", "DB", "-jname", "J"]
    else:
        src, params, wd = setup_m3(cwd)
        f1, f2 = sorted(params["runs"].values())[0]
        args = ["-wdir", wd, "-f1", wd + f1, "-f2", (wd + f2) if f2 != "none" else "none"]
    dump = os.path.join(cwd, "dry.txt")
    r = run([bins[prog]] + args + ["--dry-run", dump, "--fragments"], cwd)
    assert r.returncode == 2 and b"--fragments" in r.stderr and r.stderr.count(b"\n") == 1
    assert not os.path.exists(dump) and not fragment_files(cwd)


def test_the_header_declares_and_the_binding_binds_the_fragment_functions():
    header = open(os.path.join(ROOT, "include", "kmer_id_amd.h")).read()
    assert re.search(r"typedef struct kid_fragment \{\s*uint32_t final, confident, n_kmers[^;]*final_1, final_2;\s*\} kid_fragment;", header)
    for name, arity in FUNCTIONS.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, name
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == arity == m.group(1).count(",") + 1, name
    lib = _lib.lib_path()
    if os.path.exists(lib):  # the built library exports them (nm: no device needed)
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, check=True).stdout.decode()
        for name in FUNCTIONS:
            assert re.search(r" T %s\b" % name, syms), name
