"""--hits of the three front-ends: the hits file beside the result file equals, byte for byte, the file the model of
tests/read_hits_model.py writes from the same probes and reads; every other output equals the committed goldens with
and without the option; the file does not depend on --batch-reads, --devices or --samples-in-flight; a sample that
fails leaves no hits file.

nk10 (FASTQ only): the model reads the FASTQ files itself and trims with the oracle's process_qual.  kmer_read_vf6 and
kmer_read_m3 also read FASTA and plain text: there the model takes the reads as handed to the GPU (header, start,
stop, sequence) from the front-end's own --dry-run dump, which the CPU tests pin against the goldens; the database
entries come from helpers.parse_probes_text and the hit logic is the model's own."""
import filecmp
import gzip
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import K, concat_reads, ob, oracle_db, parse_probes_text
from read_hits_model import HitModel
from test_cli_host import make_db_dir, nk10  # noqa: F401  (nk10: fixture)
from test_cli_vf6_m3 import bins, m3_reference_result, parse_dump, setup_m3, setup_vf6  # noqa: F401  (bins: fixture)

pytestmark = pytest.mark.gpu


def model_hits_file(odb, keys, targets, reads, u_is_t=False):
    """reads: [(header, start, stop, sequence)] in the reference's order, each one handed to process_read"""
    model = HitModel(odb, keys, targets, K, u_is_t=u_is_t)
    bases, off = concat_reads([r[3] for r in reads])
    start = np.array([r[1] for r in reads], np.int32)
    stop = np.array([r[2] for r in reads], np.int32)
    hits = model.batch(bases, off, start, stop)
    final = ob.OracleSample(odb).classify(bases, off, start, stop)
    out = []
    for r, (acc, st, sp, seq) in enumerate(reads):
        pos, tgt, ent = hits.of(r)
        if pos.size == 0:
            continue
        assert model.fold(tgt) == int(final[r])
        triples = b" ".join(b"%d:%d:%d" % (p, t, e) for p, t, e in zip(pos.tolist(), tgt.tolist(), ent.tolist()))
        out.append(b"%d\t%d\t%d\t%d\t%s\t%s\n" % (int(final[r]), sp - st + 1, int(hits.n_kmers[r]), pos.size, triples, acc))
    return b"".join(out)


def probes_of(path):
    return parse_probes_text(gzip.open(path).read(), K)


def fastq_reads(path):
    """the records of a FASTQ.gz file that the reference hands to process_read, trimmed by the oracle's process_qual"""
    lines = gzip.open(path).read().split(b"\n")[:-1]
    lines = [l[:-1] if l.endswith(b"\r") else l for l in lines]
    lines = [l for l in lines if l]
    out = []
    for i in range(0, len(lines) - 3, 4):
        acc, seq, qual = lines[i], lines[i + 1], lines[i + 3]
        called, st, sp = ob.process_qual(qual, len(seq), K)
        assert called >= 0
        if called:
            out.append((acc, st, sp, seq))
    return out


# ------------------------------------------------------------------ nk10
def stage_small(gold_dir, cwd):
    src = os.path.join(gold_dir, "e2e_small")
    params = json.load(open(os.path.join(src, "params.json")))
    parent, cum, _, _ = make_db_dir(cwd, params["scale"])
    fq = os.path.join(cwd, "fq")
    os.makedirs(fq)
    for f in os.listdir(src):
        if f.endswith(".fastq.gz"):
            shutil.copy(os.path.join(src, f), fq)
    return src, fq, parent


def run_small(nk10, src, fq, cwd, extra):
    for f in os.listdir(fq):
        if f.endswith(".txt"):
            os.remove(os.path.join(fq, f))
    r = subprocess.run([nk10, fq + "/", "--log2-slots", "22"] + extra, cwd=cwd, stdout=subprocess.PIPE, check=True)
    for prefix in ("S1", "S2"):
        for suffix in ("_result.txt", "_reads.txt"):
            assert filecmp.cmp(os.path.join(fq, prefix + suffix), os.path.join(src, prefix + suffix), shallow=False), (extra, prefix + suffix)
    got = r.stdout.decode().replace(fq + "/", "<DIR>").splitlines()
    exp = open(os.path.join(src, "stdout.txt")).read().splitlines()
    assert sorted(got) == sorted(exp) and got[:3] == exp[:3], extra
    return {p: open(os.path.join(fq, p + "_hits.txt"), "rb").read() for p in ("S1", "S2") if os.path.exists(os.path.join(fq, p + "_hits.txt"))}


def test_nk10_hits_file_equals_the_model_for_any_way_of_running(nk10, gold_dir, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    src, fq, parent = stage_small(gold_dir, cwd)
    keys, targets = probes_of(os.path.join(cwd, "bact10", "probes10.txt.gz"))
    odb = oracle_db(parent, keys, targets, 22)
    exp = {p: model_hits_file(odb, keys, targets, fastq_reads(os.path.join(fq, p + "_R1_tr.fastq.gz")) +
                              fastq_reads(os.path.join(fq, p + "_R2_tr.fastq.gz"))) for p in ("S1", "S2")}
    assert all(e.count(b"\n") > 50 for e in exp.values())
    assert any(int(l.split(b"\t")[3]) >= 2 for l in exp["S1"].splitlines())
    assert run_small(nk10, src, fq, cwd, []) == {}  # without the option: the goldens, and no hits file
    cache = os.path.join(cwd, "db.kidx")
    for extra in ([], ["--batch-reads", "7"], ["--devices", "0,0", "--batch-reads", "53"], ["--samples-in-flight", "2"],
                  ["--threads", "1", "--samples-in-flight", "1"], ["--db-cache", cache], ["--db-cache", cache]):
        got = run_small(nk10, src, fq, cwd, ["--hits"] + extra)
        assert sorted(got) == ["S1", "S2"], extra
        for p in ("S1", "S2"):
            assert got[p] == exp[p], (extra, p)


def test_nk10_hits_with_dry_run_is_ignored(nk10, gold_dir, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    src, fq, parent = stage_small(gold_dir, cwd)
    dump = os.path.join(cwd, "dry.txt")
    subprocess.run([nk10, fq + "/", "--dry-run", dump, "--hits"], cwd=cwd, check=True, stdout=subprocess.PIPE)
    assert os.path.getsize(dump) > 0 and not [f for f in os.listdir(fq) if f.endswith("_hits.txt")]


@pytest.mark.parametrize("options, words", [(["--hits"], ["hits"]),
                                            (["--hits", "--min-hits", "2", "--segments", "40:20"], ["hits", "confident", "segments"])],
                         ids=["hits", "all-side-files"])
def test_nk10_failing_sample_leaves_no_hits_file(nk10, gold_dir, tmp_path, options, words):  # noqa: F811
    cwd = str(tmp_path)
    src, fq, parent = stage_small(gold_dir, cwd)
    p = os.path.join(fq, "S2_R2_tr.fastq.gz")
    raw = open(p, "rb").read()
    open(p, "wb").write(raw[:len(raw) * 2 // 3])  # cut off: everything in front is read, then "failed gzclose", exit 255
    for prefix in ("S1", "S2"):
        for word in words:
            open(os.path.join(fq, "%s_%s.txt" % (prefix, word)), "w").write("left by an earlier run\n")
    r = subprocess.run([nk10, fq + "/", "--log2-slots", "22", "--samples-in-flight", "1"] + options, cwd=cwd, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE)
    assert r.returncode == 255 and b"failed gzclose" in r.stderr
    for word in words + ["result"]:
        assert not os.path.exists(os.path.join(fq, "S2_%s.txt" % word)), word
    # S1 is whole if the directory order put it first, and was never started (or was taken back) otherwise
    whole = os.path.exists(os.path.join(fq, "S1_result.txt"))
    for word in words:
        s1 = os.path.join(fq, "S1_%s.txt" % word)
        assert os.path.exists(s1) == whole, word
        if whole:
            assert b"left by an earlier run" not in open(s1, "rb").read(), word
    if whole:
        assert filecmp.cmp(os.path.join(fq, "S1_result.txt"), os.path.join(src, "S1_result.txt"), shallow=False)


# ------------------------------------------------------------------ kmer_read_vf6
@pytest.mark.parametrize("extra", [[], ["--devices", "0,0"], ["--batch-reads", "7"]])
def test_vf6_hits_file_equals_the_model(bins, tmp_path, extra):  # noqa: F811
    cwd = str(tmp_path)
    src, params = setup_vf6(cwd)
    dump = os.path.join(cwd, "dry.txt")
    subprocess.run([bins["kmer_read_vf6"], "-name", "DB", "-jname", "J", "--dry-run", dump, "--hits"], cwd=cwd, check=True,
                   stdout=subprocess.PIPE)
    par, _, _, files = parse_dump(dump)
    assert not [f for f in os.listdir(os.path.join(cwd, "J")) if f.endswith("_hits.txt")]  # --dry-run: no GPU, no hits file
    keys, targets = probes_of(os.path.join(cwd, "DB", "DB_probes.txt.gz"))
    odb = oracle_db(par, keys, targets, 22, flags=ob.KO_FLAG_U_IS_T)
    exp = {"jobA": model_hits_file(odb, keys, targets, files[0][1] + files[1][1], u_is_t=True),
           "jobB": model_hits_file(odb, keys, targets, files[2][1] + files[3][1], u_is_t=True)}
    assert all(e.count(b"\n") > 5 for e in exp.values())
    args = ["--batch-reads", "37"] if "--batch-reads" not in extra else []
    r = subprocess.run([bins["kmer_read_vf6"], "-name", "DB", "-jname", "J", "--log2-slots", "22", "--hits"] + args + extra, cwd=cwd,
                       check=True, stdout=subprocess.PIPE)
    assert r.stdout.decode() == open(os.path.join(src, "plain", "stdout.txt")).read()
    produced = sorted(f for f in os.listdir(os.path.join(cwd, "J")) if f != "J.txt")
    golden = sorted(f for f in os.listdir(os.path.join(src, "plain")) if f != "stdout.txt")
    assert produced == sorted(golden + ["jobA_hits.txt", "jobB_hits.txt"])
    for f in golden:
        assert filecmp.cmp(os.path.join(cwd, "J", f), os.path.join(src, "plain", f), shallow=False), f
    for job in ("jobA", "jobB"):
        assert open(os.path.join(cwd, "J", job + "_hits.txt"), "rb").read() == exp[job], job


# ------------------------------------------------------------------ kmer_read_m3
@pytest.mark.parametrize("devices", [None, "0,0"])
def test_m3_hits_file_equals_the_model(bins, tmp_path, devices):  # noqa: F811
    cwd = str(tmp_path)
    src, params, wd = setup_m3(cwd)
    keys, targets = probes_of(wd + "mitochondria_probes.txt.gz")
    some = 0
    for tag, (f1, f2) in params["runs"].items():
        files_args = ["-wdir", wd, "-f1", wd + f1, "-f2", (wd + f2) if f2 != "none" else "none"]
        dump = os.path.join(cwd, "dry_%s.txt" % tag)
        subprocess.run([bins["kmer_read_m3"]] + files_args + ["--dry-run", dump], cwd=cwd, check=True, stdout=subprocess.PIPE)
        par, _, _, files = parse_dump(dump)
        odb = oracle_db(par, keys, targets, params["log2_slots"], max_probes=16)
        exp = model_hits_file(odb, keys, targets, [r for f in files for r in f[1]])
        some += exp.count(b"\n")
        if os.path.exists(wd + "hits.txt"):
            os.remove(wd + "hits.txt")
        r = subprocess.run([bins["kmer_read_m3"]] + files_args + ["--log2-slots", str(params["log2_slots"]), "--batch-reads", "53", "--hits"] +
                           (["--devices", devices] if devices else []), cwd=cwd, check=True, stdout=subprocess.PIPE)
        got = r.stdout.decode().replace(wd, "<WD>").splitlines()
        ref = open(os.path.join(src, tag + "_stdout.txt")).read().splitlines()
        assert [l for i, l in enumerate(got) if i != 6] == [l for i, l in enumerate(ref) if i != 6], tag
        assert open(wd + "result.txt", "rb").read() == m3_reference_result(os.path.join(src, tag + "_result.txt"), 17227), tag
        assert open(wd + "hits.txt", "rb").read() == exp, tag
    assert some > 20
