"""kmer_coverage end to end on a database with real sites: a probes file whose lines are the k-mers of three seeded
genomes at their true positions, reads cut from all of genome A and from one 2 kb stretch of genome B (none from C)
classified by nk10 --seen, and kmer_coverage on the seen files: stdout is exactly the model's lines, A is covered
everywhere, B at one locus, C not at all."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import seen_coverage_model as cm
from helpers import K
from kmer_id_amd import _build, read_probe_sites, read_seen_file, synth, write_seen_file
from test_cli_host import nk10, write_tree  # noqa: F401  (nk10: fixture)

pytestmark = pytest.mark.gpu

COMP = bytes.maketrans(b"ACGT", b"TGCA")
# genome -> (target, org, length): organisms 0 and 2 have no probe
GENOMES = {"A": (10, 1, 6000), "B": (20, 3, 8000), "C": (30, 4, 5000)}
STRETCH = (3000, 5000)  # of B


def revcomp(s):
    return s.translate(COMP)[::-1]


def make_database(cwd):
    """bact10/ with the tree, the data file and the probes of the three genomes -> (genomes, org, pos per entry)"""
    rng = np.random.default_rng(4242)
    parent, _ = synth.load_taxonomy("bact10")
    os.makedirs(os.path.join(cwd, "bact10"))
    write_tree(os.path.join(cwd, "bact10", "btree_10.txt"), parent)
    with open(os.path.join(cwd, "bact10", "bData10.txt"), "w") as fh:
        fh.write("4\tCP000828\r\n")
    genomes, org, pos, lines = {}, [], [], []
    for name, (target, g, length) in GENOMES.items():
        seq = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), length))
        genomes[name] = seq
        for p in range(length - K + 1):
            kmer = seq[p:p + K]
            rc = revcomp(kmer)
            lines.append(b"%s,%d,%d,%d,%s,1\n" % (min(kmer, rc), target, g, p, b"F" if kmer <= rc else b"R"))  # the canonical form, as a builder writes it
            org.append(g)
            pos.append(p)
    with gzip.open(os.path.join(cwd, "bact10", "probes10.txt.gz"), "wb") as fh:
        fh.write(b"".join(lines))
    return genomes, np.array(org, np.uint32), np.array(pos, np.uint32)


def write_reads(path, seq, lo, hi, tag):
    """reads of 150 bases every 50 over seq[lo:hi], every other one from the reverse strand"""
    with gzip.open(path, "wb") as fh:
        for i, at in enumerate(list(range(lo, hi - 150, 50)) + [hi - 150]):
            r = seq[at:at + 150]
            fh.write(b"@%s_%d\n%s\n+\n%s\n" % (tag, at, revcomp(r) if i & 1 else r, b"I" * 150))


def run(tool, cwd, args):
    r = subprocess.run([tool] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, (args, r.stderr)
    return r.stdout


def test_kmer_coverage_on_three_genomes(nk10, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    genomes, org, pos = make_database(cwd)
    probes = os.path.join(cwd, "bact10", "probes10.txt.gz")
    file_org, file_pos = read_probe_sites(probes)
    assert np.array_equal(file_org, org) and np.array_equal(file_pos, pos)
    fq = os.path.join(cwd, "fq")
    os.makedirs(fq)
    # S1: all of A and the stretch of B; S2: all of C and the front of A
    write_reads(os.path.join(fq, "S1_R1_tr.fastq.gz"), genomes["A"], 0, 6000, b"a")
    write_reads(os.path.join(fq, "S1_R2_tr.fastq.gz"), genomes["B"], STRETCH[0], STRETCH[1], b"b")
    write_reads(os.path.join(fq, "S2_R1_tr.fastq.gz"), genomes["C"], 0, 5000, b"c")
    write_reads(os.path.join(fq, "S2_R2_tr.fastq.gz"), genomes["A"], 0, 2500, b"a")
    subprocess.run([nk10, fq + "/", "--log2-slots", "18", "--seen"], cwd=cwd, stdout=subprocess.PIPE, check=True, timeout=300)
    paths = [os.path.join(fq, p + "_seen.bin") for p in ("S1", "S2")]
    maps = []
    for p in paths:
        bitmap, n_entries, ntar, k = read_seen_file(p)
        assert (n_entries, k) == (org.size, K)
        maps.append(bitmap)
    _build.build_cli()
    tool = _build.cli_path("kmer_coverage")
    base = ["--probes", probes]
    n_orgs = 5
    # ---- one file
    recs = cm.coverage(org, pos, maps[:1], 1000, n_orgs)
    plain = cm.cli_lines(paths[:1], recs)
    assert run(tool, cwd, base + paths[:1]) == plain == run(tool, cwd, base + ["--min-seen", "1", "--bin-width", "1000", "--threads", "2"] + paths[:1])
    a, b, c = (recs[0, GENOMES[name][1]] for name in "ABC")
    assert a["n_probes"] == 6000 - K + 1 and a["bins"] == 6 and a["bins_seen"] == a["bins"] and a["max_gap"] == 0
    assert b["bins"] == 8 and b["max_gap"] > 0 and b["bins_seen"] < b["bins"] and STRETCH[0] // 1000 <= b["max_bin"] < STRETCH[1] // 1000
    assert c["n_probes"] == 5000 - K + 1 and c["n_seen"] == 0
    lines = plain.split(b"\n")
    assert [l.split(b",")[1] for l in lines[1:-1]] == [b"1", b"3"]  # A and B have a line, C and the organisms without probes none
    # ---- a threshold (a copy of S1's bitmap with four bits of C set gives it something to drop), another width, the bins of B
    few = maps[0].copy()
    first_c = int(np.flatnonzero(org == 4)[0])
    for o in range(first_c + 8, first_c + 12):
        few[o >> 3] |= 1 << (o & 7)
    few_path = os.path.join(cwd, "few_seen.bin")
    write_seen_file(few_path, few, org.size, 5982, K)
    recs_few = cm.coverage(org, pos, [few], 1000, n_orgs)
    assert recs_few[0, 4]["n_seen"] == 4
    with_c, without_c = cm.cli_lines([few_path], recs_few), cm.cli_lines([few_path], recs_few, 5)
    assert with_c.count(b"\n") == without_c.count(b"\n") + 1
    assert run(tool, cwd, base + [few_path]) == with_c and run(tool, cwd, base + ["--min-seen", "5", few_path]) == without_c
    assert run(tool, cwd, base + ["--bin-width", "500"] + paths[:1]) == cm.cli_lines(paths[:1], cm.coverage(org, pos, maps[:1], 500, n_orgs))
    e_base, e_probes, e_seen = cm.bins_model(org, pos, maps[:1], 1000, n_orgs)
    bins_lines = cm.cli_bins_lines(paths[:1], e_base, e_probes, e_seen, 3)
    assert run(tool, cwd, base + ["--bins", "3"] + paths[:1]) == bins_lines and bins_lines.count(b"\n") == 1 + 8
    # ---- two files, and a file named twice
    for order in ([0, 1], [1, 0, 1]):
        fp, fm = [paths[f] for f in order], [maps[f] for f in order]
        assert run(tool, cwd, base + fp) == cm.cli_lines(fp, cm.coverage(org, pos, fm, 1000, n_orgs)), order
        e_base, e_probes, e_seen = cm.bins_model(org, pos, fm, 500, n_orgs)
        assert run(tool, cwd, base + ["--bins", "1", "--bin-width", "500"] + fp) == cm.cli_bins_lines(fp, e_base, e_probes, e_seen, 1), order
    # ---- an organism the probes do not have; the probes of another database
    r = subprocess.run([tool] + base + ["--bins", "5"] + paths[:1], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 3 and r.stdout == b"" and r.stderr.count(b"\n") == 1, r.stderr
    fewer = os.path.join(cwd, "fewer_probes.txt.gz")
    with gzip.open(fewer, "wb") as fh:
        fh.write(b"".join(gzip.open(probes).read().splitlines(True)[:-1]))
    r = subprocess.run([tool, "--probes", fewer] + paths, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 3 and r.stdout == b"" and r.stderr.count(b"\n") == 1, r.stderr
