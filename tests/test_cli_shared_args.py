"""--seen of the three front-ends and the arguments of kmer_shared, without a GPU: --seen is a flag without a value that
--dry-run ignores; kmer_shared decides usage errors (2), files that cannot be opened (255) and files that are no seen files
or do not agree (3) before it opens a probes file or a device; the C ABI of the feature is declared and bound."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import shared_kmers_model as sm
from helpers import ROOT
from kmer_id_amd import _build, _lib, write_seen_file
from test_cli_host import make_db_dir, nk10  # noqa: F401  (nk10: fixture)
from test_cli_vf6_m3 import bins, setup_m3, setup_vf6  # noqa: F401  (bins: fixture)

WAYS = [["--seen"], ["--seen", "--min-hits", "2", "--confidence", "0.02"], ["--hits", "--seen", "--depth", "--seen"]]


def seen_files(top):
    return [f for _, _, fs in os.walk(top) for f in fs if "seen" in f]


@pytest.fixture(scope="module")
def kmer_shared():
    _build.build_cli()
    return _build.cli_path("kmer_shared")


def test_nk10_seen_under_dry_run(nk10, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    make_db_dir(cwd, 2e-5)
    fq = os.path.join(cwd, "fq")
    os.makedirs(fq)
    dump = os.path.join(cwd, "dry.txt")
    plain = subprocess.run([nk10, fq + "/", "--dry-run", dump], cwd=cwd, stdout=subprocess.PIPE, check=True).stdout
    ref = open(dump, "rb").read()
    for way in WAYS:
        r = subprocess.run([nk10, fq + "/"] + way[:1] + ["--dry-run", dump] + way[1:], cwd=cwd, stdout=subprocess.PIPE, check=True)
        assert r.stdout == plain and open(dump, "rb").read() == ref and not seen_files(cwd), way
    # it takes no value: the word behind it is read as an argument of its own
    r = subprocess.run([nk10, fq + "/", "--dry-run", dump, "--seen", "--no-such-option"], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 2


@pytest.mark.parametrize("prog", ["kmer_read_vf6", "kmer_read_m3"])
def test_vf6_m3_seen_under_dry_run(bins, tmp_path, prog):  # noqa: F811
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
        assert r.stdout == plain and open(dump, "rb").read() == ref and not seen_files(cwd), way


def run(kmer_shared, cwd, args):  # noqa: F811
    r = subprocess.run([kmer_shared] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.stdout == b"", args  # nothing is printed by a run that fails
    return r.returncode, r.stderr


def test_kmer_shared_usage_errors(kmer_shared, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    good = os.path.join(cwd, "a_seen.bin")
    write_seen_file(good, np.zeros(16, np.uint8), 40, 12, 30)
    for args in ([], ["--ntar", "12"], [good] * 65, [good, "--ntar"], [good, "--min-shared"], ["--probes"], [good, "--k", "x"],
                 [good, "--min-shared", "-1"], [good, "--no-such-option"]):
        code, err = run(kmer_shared, cwd, args)
        assert code == 2 and err.count(b"\n") == 1, args


def test_kmer_shared_files_it_refuses(kmer_shared, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    path = lambda name: os.path.join(cwd, name)  # noqa: E731
    bitmap = sm.pack(np.arange(40) % 3 == 0)
    write_seen_file(path("a_seen.bin"), bitmap, 40, 12, 30)
    write_seen_file(path("b_seen.bin"), bitmap, 40, 12, 30)
    write_seen_file(path("other_entries.bin"), bitmap, 41, 12, 30)
    write_seen_file(path("other_ntar.bin"), bitmap, 40, 13, 30)
    write_seen_file(path("other_k.bin"), bitmap, 40, 12, 29)
    raw = open(path("a_seen.bin"), "rb").read()
    open(path("magic.bin"), "wb").write(b"KIDSEEN0" + raw[8:])
    open(path("cut.bin"), "wb").write(raw[:-3])
    open(path("head.bin"), "wb").write(raw[:31])
    open(path("size.bin"), "wb").write(raw[:8] + struct.pack("<QiiQ", 40, 12, 30, 32) + raw[32:] * 2)
    base = ["--ntar", "12", "--probes", path("no_such_probes.txt.gz")]  # (never opened: every case below ends before)
    code, err = run(kmer_shared, cwd, base + [path("a_seen.bin"), path("missing_seen.bin")])
    assert code == 255 and b"missing_seen.bin" in err and err.count(b"\n") == 1
    for bad in ("magic.bin", "cut.bin", "head.bin", "size.bin", "other_entries.bin", "other_ntar.bin", "other_k.bin"):
        code, err = run(kmer_shared, cwd, base + [path("a_seen.bin"), path("b_seen.bin"), path(bad)])
        assert code == 3 and bad.encode() in err and err.count(b"\n") == 1, bad
    for against in (["--ntar", "13"], ["--ntar", "12", "--k", "29"], []):  # (the defaults are 5982 and 30)
        code, err = run(kmer_shared, cwd, against + ["--probes", path("no_such_probes.txt.gz"), path("a_seen.bin")])
        assert code == 3 and b"a_seen.bin" in err and err.count(b"\n") == 1, against


def test_the_header_declares_and_the_binding_binds_the_shared_functions():
    header = open(os.path.join(ROOT, "include", "kmer_id_amd.h")).read()
    assert re.search(r"#define\s+KID_SHARED_MAX_SAMPLES\s+64\b", header) and _lib.KID_SHARED_MAX_SAMPLES == 64
    for name, arity in {"kid_db_shared_kmers": 5, "kid_shared_kmers": 8}.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, name
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == arity == m.group(1).count(",") + 1, name
    lib = _lib.lib_path()
    if os.path.exists(lib):  # the built library exports them (nm: no device needed)
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, check=True).stdout.decode()
        for name in ("kid_db_shared_kmers", "kid_shared_kmers"):
            assert re.search(r" T %s\b" % name, syms), name
