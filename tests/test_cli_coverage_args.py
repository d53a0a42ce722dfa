"""The arguments of kmer_coverage, without a GPU: it decides usage errors (2), files that cannot be opened (255) and files
that are no seen files or do not agree, a probes file with another entry count and a probe line without a site (3)
before it opens a device; the C ABI of the feature is declared and bound; the site columns come through the loader and
through read_probe_sites alike."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import shared_kmers_model as sm
from helpers import ROOT
from kmer_id_amd import COVERAGE_DTYPE, _build, _lib, read_probe_sites, write_seen_file


@pytest.fixture(scope="module")
def kmer_coverage():
    _build.build_cli()
    return _build.cli_path("kmer_coverage")


def run(kmer_coverage, cwd, args):
    r = subprocess.run([kmer_coverage] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.stdout == b"", args  # nothing is printed by a run that fails
    return r.returncode, r.stderr


def write_probes(path, lines):
    with gzip.open(path, "wb") as fh:
        fh.write(b"".join(lines))


SEQ = b"ACGTTGCAAGCTTAGCCATGGATCCGATTACAGGTC"  # 36 bases: 7 entries at k = 30


def test_kmer_coverage_usage_errors(kmer_coverage, tmp_path):
    cwd = str(tmp_path)
    good = os.path.join(cwd, "a_seen.bin")
    write_seen_file(good, np.zeros(16, np.uint8), 40, 12, 30)
    for args in ([], ["--k", "30"], [good] * 65, [good, "--k"], [good, "--min-seen"], [good, "--bin-width"], [good, "--bins"], ["--probes"],
                 [good, "--k", "x"], [good, "--min-seen", "-1"], [good, "--bin-width", "0"], [good, "--bin-width", "1e3"], [good, "--bins", "b"],
                 [good, "--k", "0"], [good, "--no-such-option"], [good, "--ntar", "12"]):
        code, err = run(kmer_coverage, cwd, args)
        assert code == 2 and err.count(b"\n") == 1, args


def test_kmer_coverage_files_it_refuses(kmer_coverage, tmp_path):
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
    base = ["--probes", path("no_such_probes.txt.gz")]  # (never opened: every case below ends before)
    code, err = run(kmer_coverage, cwd, base + [path("a_seen.bin"), path("missing_seen.bin")])
    assert code == 255 and b"missing_seen.bin" in err and err.count(b"\n") == 1
    for bad in ("magic.bin", "cut.bin", "head.bin", "other_entries.bin", "other_ntar.bin", "other_k.bin"):
        code, err = run(kmer_coverage, cwd, base + [path("a_seen.bin"), path("b_seen.bin"), path(bad)])
        assert code == 3 and bad.encode() in err and err.count(b"\n") == 1, bad
    code, err = run(kmer_coverage, cwd, base + ["--k", "29", path("a_seen.bin")])  # the files agree with each other, not with --k
    assert code == 3 and b"a_seen.bin" in err and err.count(b"\n") == 1
    # the seen files are in order: now the probes file is opened, and one that is not there is a file that cannot be opened
    code, err = run(kmer_coverage, cwd, base + [path("a_seen.bin")])
    assert code == 255 and b"no_such_probes" in err


def test_kmer_coverage_probes_it_refuses(kmer_coverage, tmp_path):
    cwd = str(tmp_path)
    path = lambda name: os.path.join(cwd, name)  # noqa: E731
    write_seen_file(path("a_seen.bin"), np.zeros(16, np.uint8), 14, 12, 30)
    write_probes(path("fewer.txt.gz"), [SEQ + b",3,0,100,F,1\n"])  # 7 entries where the file was written for 14
    code, err = run(kmer_coverage, cwd, ["--probes", path("fewer.txt.gz"), path("a_seen.bin")])
    assert code == 3 and b"fewer.txt.gz" in err and err.count(b"\n") == 1
    for tag, second in (("negative_position", b",3,1,-5,F,1\n"), ("negative_org", b",3,-1,5,F,1\n")):
        write_probes(path(tag + ".txt.gz"), [SEQ + b",3,0,100,F,1\n", SEQ + second])
        code, err = run(kmer_coverage, cwd, ["--probes", path(tag + ".txt.gz"), "--threads", "2", path("a_seen.bin")])
        assert code == 3 and SEQ in err and err.count(b"\n") == 1, tag  # the line is named


def test_read_probe_sites_gives_every_entry_its_lines_site(tmp_path):
    p = os.path.join(str(tmp_path), "p.txt.gz")
    write_probes(p, [SEQ + b",3,0,100,F,1\n", SEQ[:30] + b",4,2,2147483647,R,1\r\n", b"ACGT,5,9,9,F,1\n", SEQ[:20] + b"N" + SEQ[:31] + b",6,7,8,F,2\n",
                     b"not a probe line\n", SEQ + b",3,1,4000000000,F,1\n", SEQ + b",3,0,100,F,1"])
    # (a line shorter than k, one with an N, garbage, a position no int holds: no entries, as in the front-ends; an unterminated tail)
    org, pos = read_probe_sites(p)
    assert org.dtype == pos.dtype == np.uint32
    assert org.tolist() == [0] * 7 + [2] + [7] * 2 and pos.tolist() == [100] * 7 + [2147483647] + [8] * 2
    org31, _ = read_probe_sites(p, k=31)
    assert org31.tolist() == [0] * 6 + [7]


def test_the_header_declares_and_the_binding_binds_the_coverage_functions():
    header = open(os.path.join(ROOT, "include", "kmer_id_amd.h")).read()
    assert re.search(r"#define\s+KID_COVERAGE_MAX_BINS\s+\(1ull << 28\)", header) and _lib.KID_COVERAGE_MAX_BINS == 1 << 28
    m = re.search(r"typedef struct kid_coverage \{([^}]*)\} kid_coverage;", header)
    assert m and [f.strip() for f in m.group(1).replace("uint32_t", "").strip(" ;\n").split(",")] == list(COVERAGE_DTYPE.names)
    assert COVERAGE_DTYPE.itemsize == 32
    for name, arity in {"kid_seen_coverage": 9, "kid_seen_coverage_bins": 13, "kid_seen_coverage_time": 2}.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, name
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == arity == m.group(1).count(",") + 1, name
    lib = _lib.lib_path()
    if os.path.exists(lib):  # the built library exports them (nm: no device needed)
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, check=True).stdout.decode()
        for name in ("kid_seen_coverage", "kid_seen_coverage_bins", "kid_seen_coverage_time"):
            assert re.search(r" T %s\b" % name, syms), name
