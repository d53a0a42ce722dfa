"""--low-complexity of the front-ends on .fastq.gz blocks, a plain .fastq file and FASTA input: with the option, the
result and hits files and stdout are what the same program writes WITHOUT it on files whose low-complexity bases the
Python model (low_complexity_model.py) replaced by N; the reads file lists the same reads under the same targets with
the sequences as they are in the input; nothing depends on --batch-reads or --block-bytes.  A few hundred reads with
planted repeats.  (nk10 prints its samples in directory order, which is the file system's: stdout is compared as its
first three lines and the sorted rest, as the other front-end tests compare it.)"""
import gzip
import os
import subprocess

import numpy as np
import pytest

from helpers import K, synth
from low_complexity_model import mask_reads
from test_cli_host import make_db_dir, nk10  # noqa: F401  (nk10: fixture)
from test_cli_vf6_m3 import bins, setup_vf6  # noqa: F401  (bins: fixture)

pytestmark = pytest.mark.gpu

T = 20
L = 150
OPTS = ["--hits", "--min-hits", "2"]
PERIODS = [b"A", b"CA", b"GAT", b"t", b"G"]


def planted_reads(cum, parent, n, r0, length=L):
    """n synthetic reads of `length` bases, two in three with a run of period 1, 2 or 3 planted -> (bases, model-masked)"""
    rng = np.random.default_rng(r0)
    bases = synth.reads(cum, parent, n, length, K, r0=r0).copy()
    for i in range(n):
        if i % 3 == 0:
            continue
        a, run, per = i * length + int(rng.integers(0, length - 30)), int(rng.integers(20, 55)), PERIODS[i % len(PERIODS)]
        for j in range(a, min((i + 1) * length, a + run)):
            bases[j] = per[(j - a) % len(per)]
    masked, cnt = mask_reads(bases, synth.fixed_offsets(n, length), T)
    assert cnt > 10 * n
    return bases, masked


def write_fastq(plain_dir, masked_dir, name, bases, masked, n, r0, tag, mate, u_is_t=False):
    """the same records into plain_dir as they are and into masked_dir masked; name without .gz: a plain FASTQ file,
    tokenised and trimmed on the host and masked through kid_lowc_batch"""
    quals = synth.qualities(n, L, r0=r0)
    for d, text in ((plain_dir, bases), (masked_dir, masked)):
        gz = os.path.join(d, name if name.endswith(".gz") else name + ".gz")
        synth.write_fastq_gz(gz, text, quals, L, names_prefix="@%s_" % tag, mate=mate)
        if not name.endswith(".gz"):
            open(os.path.join(d, name), "wb").write(gzip.open(gz).read())
            os.remove(gz)


def write_fasta(plain_dir, masked_dir, name, cum, parent, r0, u_is_t=False):
    """records of many lengths, one line each -- the longest is split among lanes by the kernel -> the original sequences"""
    lens = [31, 64, 150, 150, 333, 511, 512, 513, 1500, 5000] * 3
    bases, _ = planted_reads(cum, parent, (sum(lens) + L - 1) // L, r0)
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    masked = mask_reads(bases, off, T, u_is_t)[0]  # (a record is one line of the rule, whatever reads it was made of)
    assert int((masked != bases).sum()) > 1000
    for d, text in ((plain_dir, bases), (masked_dir, masked)):
        with open(os.path.join(d, name), "wb") as f:
            for i in range(len(lens)):
                f.write(b">rec%d\n" % i + text[int(off[i]):int(off[i + 1])].tobytes() + b"\n")
    return [bases[int(off[i]):int(off[i + 1])].tobytes() for i in range(len(lens))]


def saved_reads(blob):
    lines = blob.split(b"\n")
    assert lines[-1] == b"" and len(lines) % 2 == 1
    return [(lines[i], lines[i + 1]) for i in range(0, len(lines) - 1, 2)]


def check_reads_file(on, ref, originals):
    """the same reads under the same targets; `on` prints the input's sequence (originals: all of them; a read may be
    printed trimmed) where `ref` (masked input) prints N"""
    a, b = saved_reads(on), saved_reads(ref)
    originals = b"\n".join(sorted(originals))
    assert [h for h, _ in a] == [h for h, _ in b] and len(a) >= 8  # (30 FASTA records save fewer reads than 600 FASTQ ones)
    differ = 0
    for (head, s), (_, m) in zip(a, b):
        assert len(s) == len(m) and s in originals, head
        assert all(x == y or y == ord("N") for x, y in zip(s, m)), head
        differ += s != m
    assert differ > 0


def compare(on, ref, plain, originals, changed):
    assert sorted(on) == sorted(ref) == sorted(plain)
    for name in on:
        if name.endswith("_reads.txt"):
            check_reads_file(on[name], ref[name], originals)
        else:
            assert on[name] == ref[name], name
    for name in changed:
        assert on[name] != plain[name], name


def test_nk10_fastq_gz_and_fasta(nk10, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    parent, cum, _, _ = make_db_dir(cwd, 1e-3)
    dirs = {}
    for d in ("fq", "fqm", "fa", "fam"):
        dirs[d] = os.path.join(cwd, d)
        os.makedirs(dirs[d])
    originals = set()
    n = 300
    for mate in (1, 2):
        bases, masked = planted_reads(cum, parent, n, 50000 + mate * n)
        write_fastq(dirs["fq"], dirs["fqm"], "S1_R%d_tr.fastq.gz" % mate, bases, masked, n, 50000 + mate * n, "S1", mate)
        originals.update(bases.reshape(n, L)[i].tobytes() for i in range(n))
    originals.update(write_fasta(dirs["fa"], dirs["fam"], "X_R1.fasta", cum, parent, 61000))

    def run(d, extra):
        for f in os.listdir(d):
            if f.endswith(".txt"):
                os.remove(os.path.join(d, f))
        r = subprocess.run([nk10, d + "/", "--log2-slots", "22"] + OPTS + extra, cwd=cwd, stdout=subprocess.PIPE, check=True)
        out = r.stdout.decode().replace(d + "/", "<DIR>").splitlines()
        return (out[:3], sorted(out[3:])), {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if f.endswith(".txt")}

    opt = ["--low-complexity", str(T)]
    out_on, on = run(dirs["fq"], opt)
    out_ref, ref = run(dirs["fqm"], [])
    out_plain, plain = run(dirs["fq"], [])
    assert sorted(on) == ["S1_confident.txt", "S1_hits.txt", "S1_reads.txt", "S1_result.txt"] and out_on == out_ref
    compare(on, ref, plain, originals, ["S1_hits.txt"])
    assert run(dirs["fq"], ["--low-complexity", "0"]) == (out_plain, plain)
    for extra in (["--batch-reads", "257"], ["--block-bytes", "40000"]):
        assert run(dirs["fq"], opt + extra) == (out_on, on), extra

    fasta = ["--fasta", "--r1", "_R1.fasta"]
    out_on, on = run(dirs["fa"], fasta + opt)
    out_ref, ref = run(dirs["fam"], fasta)
    out_plain, plain = run(dirs["fa"], fasta)
    assert "X_hits.txt" in on and out_on == out_ref
    compare(on, ref, plain, originals, ["X_hits.txt"])
    assert run(dirs["fa"], fasta + opt + ["--batch-reads", "7"]) == (out_on, on)


def test_vf6_fastq_gz_plain_fastq_and_fasta(bins, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    src, params = setup_vf6(cwd)
    parent, cnt = synth.load_taxonomy("bact10")
    cum = synth.cumulative(synth.scaled_counts(cnt, params["scale"]))
    os.makedirs(os.path.join(cwd, "inm")); os.makedirs(os.path.join(cwd, "M"))
    plain_dir, masked_dir = os.path.join(cwd, "in"), os.path.join(cwd, "inm")
    originals = set()
    n = 300
    for mate, name in enumerate(("x_1.fastq.gz", "x_3.fastq"), 1):
        bases, masked = planted_reads(cum, parent, n, 70000 + mate * n)
        write_fastq(plain_dir, masked_dir, name, bases, masked, n, 70000 + mate * n, "x", mate)
        originals.update(bases.reshape(n, L)[i].tobytes() for i in range(n))
    originals.update(write_fasta(plain_dir, masked_dir, "y.fasta", cum, parent, 81000, u_is_t=True))
    for jname, d in (("J", "in"), ("M", "inm")):
        open(os.path.join(cwd, jname, jname + ".txt"), "w").write("jobT 3\n%s/x_1.fastq.gz\n%s/x_3.fastq\n%s/y.fasta\n" % (d, d, d))

    def run(jname, extra):
        r = subprocess.run([bins["kmer_read_vf6"], "-name", "DB", "-jname", jname, "--log2-slots", "22"] + OPTS + extra, cwd=cwd,
                           stdout=subprocess.PIPE, check=True)
        d = os.path.join(cwd, jname)
        return r.stdout.decode().replace("inm/", "in/"), {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if f.startswith("jobT_")}

    opt = ["--low-complexity", str(T)]
    out_on, on = run("J", opt)
    out_ref, ref = run("M", [])
    out_plain, plain = run("J", [])
    assert sorted(on) == ["jobT_confident.txt", "jobT_hits.txt", "jobT_reads.txt", "jobT_result.txt"] and out_on == out_ref
    compare(on, ref, plain, originals, ["jobT_hits.txt"])
    assert run("J", opt + ["--batch-reads", "257"]) == (out_on, on)
