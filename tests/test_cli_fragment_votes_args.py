"""--fragment-votes of nk10 without a GPU: a flag without a value that --dry-run checks and then ignores (the same stdout,
the same dump, no fragment_votes file), refused with --fasta and by the two front-ends that read their inputs one file
after the other; and the C ABI of the feature is declared, bound with the declared arity and exported."""
import os
import re
import subprocess

import pytest

from helpers import ROOT
from kmer_id_amd import FRAGMENT_VOTE_DTYPE, VOTE_DTYPE, KmerDB, _lib
from test_cli_host import make_db_dir, nk10  # noqa: F401  (nk10: fixture)
from test_cli_vf6_m3 import bins, setup_m3, setup_vf6  # noqa: F401  (bins: fixture)

FUNCTIONS = {"kid_db_read_fragment_votes": 10, "kid_db_read_fragment_votes_fastq": 12, "kid_db_fragment_votes_from_hits_device": 9,
             "kid_db_read_fragment_votes_time": 4}


def side_files(top):
    return [f for _, _, fs in os.walk(top) for f in fs if "fragment" in f or "votes" in f]


def run(cmd, cwd):
    return subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def test_nk10_fragment_votes_under_dry_run(nk10, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    make_db_dir(cwd, 2e-5)
    fq = os.path.join(cwd, "fq")
    os.makedirs(fq)
    dump = os.path.join(cwd, "dry.txt")
    plain = subprocess.run([nk10, fq + "/", "--dry-run", dump], cwd=cwd, stdout=subprocess.PIPE, check=True).stdout
    ref = open(dump, "rb").read()
    for way in (["--fragment-votes"], ["--fragment-votes", "--min-hits", "2", "--confidence", "0.025"], ["--fragment-votes", "--fragments", "--votes"],
                ["--fragment-votes", "--block-bytes", "32768"]):
        r = subprocess.run([nk10, fq + "/"] + way[:1] + ["--dry-run", dump] + way[1:], cwd=cwd, stdout=subprocess.PIPE, check=True)
        assert r.stdout == plain and open(dump, "rb").read() == ref and not side_files(cwd), way
    # it takes no value: the word behind it is read as an argument of its own
    for word in ("1", "--no-such-option"):
        r = run([nk10, fq + "/", "--dry-run", dump, "--fragment-votes", word], cwd)
        assert r.returncode == 2 and word.encode() in r.stderr, r.stderr
    # ... and the rule's options are still checked beside it
    assert run([nk10, fq + "/", "--dry-run", dump, "--fragment-votes", "--confidence", "2"], cwd).returncode == 2


def test_nk10_refuses_fragment_votes_with_fasta(nk10, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    make_db_dir(cwd, 2e-5)
    fq = os.path.join(cwd, "fq")
    os.makedirs(fq)
    for words in (["--fasta", "--fragment-votes"], ["--fragment-votes", "--fasta"]):
        r = run([nk10, fq + "/", "--dry-run", os.path.join(cwd, "dry.txt")] + words, cwd)
        assert r.returncode == 2 and b"--fragment-votes" in r.stderr and b"--fasta" in r.stderr, r.stderr
        assert r.stderr.count(b"\n") == 1 and not os.path.exists(os.path.join(cwd, "dry.txt"))


@pytest.mark.parametrize("prog", ["kmer_read_vf6", "kmer_read_m3"])
def test_vf6_and_m3_refuse_fragment_votes(bins, tmp_path, prog):  # noqa: F811
    cwd = str(tmp_path)
    if prog == "kmer_read_vf6":
        setup_vf6(cwd)
        args = ["-name", "DB", "-jname", "J"]
    else:
        src, params, wd = setup_m3(cwd)
        f1, f2 = sorted(params["runs"].values())[0]
        args = ["-wdir", wd, "-f1", wd + f1, "-f2", (wd + f2) if f2 != "none" else "none"]
    dump = os.path.join(cwd, "dry.txt")
    r = run([bins[prog]] + args + ["--dry-run", dump, "--fragment-votes"], cwd)
    assert r.returncode == 2 and b"--fragment-votes" in r.stderr and b"nk10 alone" in r.stderr and r.stderr.count(b"\n") == 1
    assert not os.path.exists(dump) and not side_files(cwd)


def test_the_header_declares_and_the_binding_binds_the_fragment_vote_functions():
    header = open(os.path.join(ROOT, "include", "kmer_id_amd.h")).read()
    assert re.search(r"typedef struct kid_fragment_vote \{\s*uint32_t call, confident, n_kmers[^;]*s_call, s_confident, call_1, call_2;\s*\} "
                     r"kid_fragment_vote;", header)
    for name, arity in FUNCTIONS.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, name
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == arity == m.group(1).count(",") + 1, name
    # argument for argument the fragment calls
    for name in FUNCTIONS:
        twin = name.replace("fragment_votes", "fragments")
        assert [a for a in _lib.PROTOTYPES[name][1]] == [a for a in _lib.PROTOTYPES[twin][1]], name
    lib = _lib.lib_path()
    if os.path.exists(lib):  # the built library exports them (nm: no device needed)
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, check=True).stdout.decode()
        for name in FUNCTIONS:
            assert re.search(r" T %s\b" % name, syms), name


def test_the_python_layer_has_the_record_and_the_four_methods():
    assert FRAGMENT_VOTE_DTYPE.itemsize == 40 and FRAGMENT_VOTE_DTYPE.names == VOTE_DTYPE.names + ("call_1", "call_2")
    import inspect
    for name in ("read_fragment_votes", "read_fragment_votes_fastq", "fragment_votes_from_hits_device", "read_fragment_votes_time"):
        twin = name.replace("fragment_votes", "fragments")
        assert str(inspect.signature(getattr(KmerDB, name))) == str(inspect.signature(getattr(KmerDB, twin))), name
