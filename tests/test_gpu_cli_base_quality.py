"""--min-base-quality of the front-ends on FASTQ input (.fastq.gz blocks; kmer_read_vf6: a plain .fastq file too): with the option, the result, hits and confident files and
stdout are what the same program writes WITHOUT it on files whose masked bases numpy replaced by N; the reads file lists
the same reads under the same targets with the sequences as they are in the input; nothing depends on --batch-reads,
--threads or --devices.  (nk10 prints its samples in directory order, which is the file system's: stdout is compared as
its first three lines and the sorted rest, as the other front-end tests compare it.)"""
import gzip
import os
import subprocess

import pytest

from base_quality_cases import np_mask
from helpers import K, synth
from test_cli_host import make_db_dir, nk10  # noqa: F401  (nk10: fixture)
from test_cli_vf6_m3 import bins, setup_vf6  # noqa: F401  (bins: fixture)

pytestmark = pytest.mark.gpu

Q = 20
L = 150
OPTS = ["--hits", "--min-hits", "2"]


def write_pair_files(cum, parent, plain_dir, masked_dir, names, n, r0, tag):
    """names: the files of one sample (mates); the same records into plain_dir as they are and into masked_dir with the
    bases below Q replaced by N -> {header: sequence} of the plain files"""
    orig = {}
    for mate, name in enumerate(names, 1):
        bases = synth.reads(cum, parent, n, L, K, r0=r0 + mate * n)
        quals = synth.qualities(n, L, r0=r0 + mate * n)
        quals[::3, 75] = ord("2")   # not trimmed by process_qual, masked at Q = 20
        quals[1::3, 40] = ord("+")
        masked, cnt = np_mask(bases, quals.reshape(-1), Q)
        assert cnt > n
        for d, text in ((plain_dir, bases), (masked_dir, masked)):
            gz = os.path.join(d, name if name.endswith(".gz") else name + ".gz")
            synth.write_fastq_gz(gz, text, quals, L, names_prefix="@%s_" % tag, mate=mate)
            if not name.endswith(".gz"):  # a plain FASTQ file: tokenised and trimmed on the host, masked through kid_mask_batch
                open(os.path.join(d, name), "wb").write(gzip.open(gz).read())
                os.remove(gz)
        lines = open(os.path.join(plain_dir, name), "rb").read().split(b"\n") if not name.endswith(".gz") else \
            gzip.open(os.path.join(plain_dir, name)).read().split(b"\n")
        orig.update({lines[i]: lines[i + 1] for i in range(0, len(lines) - 3, 4)})
    return orig


def saved_reads(blob):
    lines = blob.split(b"\n")
    assert lines[-1] == b"" and len(lines) % 2 == 1
    return [(lines[i], lines[i + 1]) for i in range(0, len(lines) - 1, 2)]


def check_reads_file(on, ref, orig):
    """the same reads under the same targets; `on` prints the input's sequence where `ref` (masked input) prints N
    (orig: the FASTQ records by header; a read of another file, a FASTA, is printed as it is by both)"""
    a, b = saved_reads(on), saved_reads(ref)
    assert [h for h, _ in a] == [h for h, _ in b] and len(a) > 20
    differ = 0
    for (head, s), (_, m) in zip(a, b):
        acc = head.split(b":", 1)[1]
        if acc not in orig:
            assert s == m, head
            continue
        assert len(s) == len(m) and s in orig[acc], head
        assert all(x == y or y == ord("N") for x, y in zip(s, m)), head
        differ += s != m
    assert differ > 0


def test_nk10_with_the_option_equals_nk10_on_masked_files(nk10, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    parent, cum, _, _ = make_db_dir(cwd, 1e-3)
    fq, fqm = os.path.join(cwd, "fq"), os.path.join(cwd, "fqm")
    os.makedirs(fq); os.makedirs(fqm)
    orig = {}
    for i, p in enumerate(("S1", "S2")):
        orig.update(write_pair_files(cum, parent, fq, fqm, [p + "_R1_tr.fastq.gz", p + "_R2_tr.fastq.gz"], 1200 + 77 * i, 50000 * (i + 1), p))

    def run(d, extra):
        for f in os.listdir(d):
            if f.endswith(".txt"):
                os.remove(os.path.join(d, f))
        r = subprocess.run([nk10, d + "/", "--log2-slots", "22"] + OPTS + extra, cwd=cwd, stdout=subprocess.PIPE, check=True)
        out = r.stdout.decode().replace(d + "/", "<DIR>").splitlines()
        return (out[:3], sorted(out[3:])), {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if f.endswith(".txt")}

    opt = ["--min-base-quality", str(Q)]
    out_on, on = run(fq, opt)
    out_ref, ref = run(fqm, [])
    out_plain, plain = run(fq, [])
    assert sorted(on) == sorted(ref) == sorted(p + s for p in ("S1", "S2") for s in ("_confident.txt", "_hits.txt", "_reads.txt", "_result.txt"))
    assert out_on == out_ref
    for name in on:
        if name.endswith("_reads.txt"):
            check_reads_file(on[name], ref[name], orig)
        else:
            assert on[name] == ref[name], name
    for p in ("S1", "S2"):
        assert on[p + "_result.txt"] != plain[p + "_result.txt"] and on[p + "_hits.txt"] != plain[p + "_hits.txt"]
    assert run(fq, ["--min-base-quality", "0"]) == (out_plain, plain)
    for extra in (["--batch-reads", "257"], ["--threads", "3"], ["--devices", "0,0"], ["--samples-in-flight", "2"]):
        assert run(fq, opt + extra) == (out_on, on), extra


def test_vf6_with_the_option_equals_vf6_on_masked_files(bins, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    src, params = setup_vf6(cwd)
    parent, cnt = synth.load_taxonomy("bact10")
    cum = synth.cumulative(synth.scaled_counts(cnt, params["scale"]))
    os.makedirs(os.path.join(cwd, "inm")); os.makedirs(os.path.join(cwd, "M"))
    orig = write_pair_files(cum, parent, os.path.join(cwd, "in"), os.path.join(cwd, "inm"), ["x_1.fastq.gz", "x_2.fastq.gz", "x_3.fastq"], 1100, 70000, "x")
    os.symlink(os.path.join(cwd, "in", "b.fasta.gz"), os.path.join(cwd, "inm", "b.fasta.gz"))  # FASTA: no qualities, no effect
    for jname, d in (("J", "in"), ("M", "inm")):
        open(os.path.join(cwd, jname, jname + ".txt"), "w").write("jobQ 4\n%s/x_1.fastq.gz\n%s/x_2.fastq.gz\n%s/x_3.fastq\n%s/b.fasta.gz\n" % (d, d, d, d))

    def run(jname, extra):
        r = subprocess.run([bins["kmer_read_vf6"], "-name", "DB", "-jname", jname, "--log2-slots", "22"] + OPTS + extra, cwd=cwd,
                           stdout=subprocess.PIPE, check=True)
        d = os.path.join(cwd, jname)
        return r.stdout.decode().replace("inm/", "in/"), {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if f.startswith("jobQ_")}

    opt = ["--min-base-quality", str(Q)]
    out_on, on = run("J", opt)
    out_ref, ref = run("M", [])
    assert sorted(on) == sorted(ref) == ["jobQ_confident.txt", "jobQ_hits.txt", "jobQ_reads.txt", "jobQ_result.txt"]
    assert out_on == out_ref
    for name in on:
        if name.endswith("_reads.txt"):
            check_reads_file(on[name], ref[name], orig)
        else:
            assert on[name] == ref[name], name
    out_plain, plain = run("J", [])
    assert on["jobQ_result.txt"] != plain["jobQ_result.txt"]
    for extra in (["--batch-reads", "257"], ["--threads", "3"], ["--devices", "0,0"]):
        assert run("J", opt + extra) == (out_on, on), extra

