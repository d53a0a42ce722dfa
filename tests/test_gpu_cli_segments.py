"""--segments LEN[:STEP] of the three front-ends: the segments file beside the result file equals, byte for byte, the
file the model of tests/read_segments_model.py writes from the same probes and reads; it does not depend on
--batch-reads, --threads, --devices or --samples-in-flight; every other output is what it is without the option; the
rule is that of --min-hits / --confidence; --min-base-quality applies as to the hits file; a stale file goes and a
sample that fails leaves none."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from helpers import K, concat_reads, ob, oracle_db, synth
from read_hits_model import HitModel, windows
from read_segments_model import SegmentModel, segments_line
from read_support_model import SupportModel
from test_cli_host import make_db_dir, nk10, write_tree  # noqa: F401  (nk10: fixture)
from test_cli_vf6_m3 import GOLD, bins, parse_dump, setup_m3  # noqa: F401  (bins: fixture)
from test_gpu_cli_base_quality import write_pair_files
from test_gpu_cli_hits import fastq_reads, probes_of, stage_small

pytestmark = pytest.mark.gpu


def model_segments_file(odb, keys, targets, parent, reads, seg, rule, u_is_t=False):
    """reads: [(header, start, stop, sequence)] in the reference's order, each one handed to process_read"""
    sm = SupportModel(HitModel(odb, keys, targets, K, u_is_t=u_is_t), parent)
    bases, off = concat_reads([r[3] for r in reads])
    start = np.array([r[1] for r in reads], np.int32)
    stop = np.array([r[2] for r in reads], np.int32)
    so, rec = SegmentModel(sm, bases, off, start, stop).direct(seg[0], seg[1], rule)
    final = ob.OracleSample(odb).classify(bases, off, start, stop)
    return b"".join(segments_line(int(final[r]), sp - st + 1, rec[int(so[r]):int(so[r + 1])], acc) for r, (acc, st, sp, _) in enumerate(reads))


def run_dir(prog, d, cwd, extra, clean=True):
    """-> (stdout: its first three lines and the sorted rest, {file name: bytes} of the .txt files in the directory)"""
    for f in os.listdir(d):
        if f.endswith(".txt") and clean:
            os.remove(os.path.join(d, f))
    r = subprocess.run([prog, d + "/", "--log2-slots", "22"] + extra, cwd=cwd, stdout=subprocess.PIPE, check=True)
    out = r.stdout.decode().replace(d + "/", "<DIR>").splitlines()
    return (out[:3], sorted(out[3:])), {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if f.endswith(".txt")}


def test_nk10_segments_file_equals_the_model_for_any_way_of_running(nk10, gold_dir, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    src, fq, parent = stage_small(gold_dir, cwd)
    keys, targets = probes_of(os.path.join(cwd, "bact10", "probes10.txt.gz"))
    odb = oracle_db(parent, keys, targets, 22)
    reads = {p: fastq_reads(os.path.join(fq, p + "_R1_tr.fastq.gz")) + fastq_reads(os.path.join(fq, p + "_R2_tr.fastq.gz")) for p in ("S1", "S2")}
    seg = (40, 20)
    exp00 = {p: model_segments_file(odb, keys, targets, parent, reads[p], seg, (0, 0)) for p in reads}
    exp = {p: model_segments_file(odb, keys, targets, parent, reads[p], seg, (2, 20)) for p in reads}
    assert all(e.count(b"\n") > 50 for e in exp.values()) and exp != exp00
    cols = [c.split(b":") for e in exp00.values() for l in e.splitlines() for c in l.split(b"\t")[4].split(b" ")]
    assert all(c[4] == c[5] for c in cols)  # without a rule confident = final
    rule = ["--min-hits", "2", "--confidence", "0.02"]
    base_out, base = run_dir(nk10, fq, cwd, ["--hits"] + rule)
    assert sorted(base) == sorted(p + s for p in ("S1", "S2") for s in ("_confident.txt", "_hits.txt", "_reads.txt", "_result.txt"))
    for p in ("S1", "S2"):  # a file an earlier run left is removed when its sample starts
        open(os.path.join(fq, p + "_segments.txt"), "w").write("left by an earlier run\n")
    opt = ["--segments", "40:20"]
    for extra in ([], ["--batch-reads", "7"], ["--batch-reads", "53", "--devices", "0,0"], ["--threads", "1", "--samples-in-flight", "1"],
                  ["--threads", "3"], ["--samples-in-flight", "2"]):
        out, got = run_dir(nk10, fq, cwd, ["--hits"] + rule + opt + extra, clean=bool(extra))  # (the first run meets the stale files)
        assert out == base_out, extra
        for p in ("S1", "S2"):
            assert got.pop(p + "_segments.txt") == exp[p], (extra, p)
        assert got == base, extra  # every other output is byte for byte what it is without the option
    out, got = run_dir(nk10, fq, cwd, opt)
    assert {p: got[p + "_segments.txt"] for p in ("S1", "S2")} == exp00 and sorted(got) == sorted(
        p + s for p in ("S1", "S2") for s in ("_reads.txt", "_result.txt", "_segments.txt"))


def test_nk10_min_base_quality_applies_as_to_the_hits_file(nk10, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    parent, cum, _, _ = make_db_dir(cwd, 1e-3)
    fq, fqm = os.path.join(cwd, "fq"), os.path.join(cwd, "fqm")
    os.makedirs(fq); os.makedirs(fqm)
    write_pair_files(cum, parent, fq, fqm, ["S1_R1_tr.fastq.gz", "S1_R2_tr.fastq.gz"], 1200, 50000, "S1")
    opt = ["--segments", "40:20", "--min-hits", "2"]
    on = run_dir(nk10, fq, cwd, opt + ["--min-base-quality", "20"])[1]["S1_segments.txt"]
    ref = run_dir(nk10, fqm, cwd, opt)[1]["S1_segments.txt"]
    plain = run_dir(nk10, fq, cwd, opt)[1]["S1_segments.txt"]
    assert on == ref and on != plain and on.count(b"\n") > 50


def test_nk10_failing_sample_leaves_no_segments_file(nk10, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    make_db_dir(cwd, 2e-5)
    fq = os.path.join(cwd, "fq"); os.makedirs(fq)
    with gzip.open(os.path.join(fq, "L_R1_tr.fastq.gz"), "wb") as fh:
        fh.write(b"@a\n" + b"ACGT" * 10 + b"\n+\n" + b"I" * 39 + b"\n")  # a quality line shorter than its sequence
    with gzip.open(os.path.join(fq, "L_R2_tr.fastq.gz"), "wb") as fh:
        fh.write(b"@b\nACGT\n+\nIIII\n")
    open(os.path.join(fq, "L_segments.txt"), "w").write("left by an earlier run\n")
    r = subprocess.run([nk10, fq + "/", "--log2-slots", "16", "--segments", "10"], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 134, (r.returncode, r.stderr[-500:])
    assert b"quality line shorter than the sequence" in r.stderr
    assert not os.path.exists(os.path.join(fq, "L_segments.txt")) and not os.path.exists(os.path.join(fq, "L_result.txt"))


def chimera_db(rng, parent):
    """two random 10 kb genomes, every window a probe: the first under 8 (5 -> 6 -> 8), the second under a node of another
    top-level lineage -> genome a, genome b, x, keys, targets"""
    x = next(t for t in range(2, parent.size) if parent[t] == 1 and t != 5)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    ga, gb = rng.choice(acgt, 10000).tobytes(), rng.choice(acgt, 10000).tobytes()
    ka, kb = windows(ga, 0, len(ga) - 1, K)[0], windows(gb, 0, len(gb) - 1, K)[0]
    return ga, gb, x, np.concatenate([ka, kb]), np.concatenate([np.full(ka.size, 8, np.uint32), np.full(kb.size, x, np.uint32)])


def test_vf6_shows_the_lineage_change_of_a_chimeric_contig(bins, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    parent, _ = synth.load_taxonomy("bact10")
    assert parent[8] == 6 and parent[6] == 5 and parent[5] == 1
    rng = np.random.default_rng(20000)
    ga, gb, x, keys, targets = chimera_db(rng, parent)
    os.makedirs(os.path.join(cwd, "DB")); os.makedirs(os.path.join(cwd, "J")); os.makedirs(os.path.join(cwd, "in"))
    write_tree(os.path.join(cwd, "DB", "DB_tree.txt"), parent)
    open(os.path.join(cwd, "DB", "DB_data.txt"), "wb").write(open(os.path.join(GOLD, "e2e_vf6", "DB_data.txt"), "rb").read())
    synth.write_probes_gz(os.path.join(cwd, "DB", "DB_probes.txt.gz"), keys, targets, K)
    other = rng.choice(np.frombuffer(b"ACGT", np.uint8), 500).tobytes()
    open(os.path.join(cwd, "in", "c.fasta"), "wb").write(b">plain\n" + other + b"\n>chimera\n" + ga + gb + b"\n>tail\n" + gb[:300] + b"\n")
    open(os.path.join(cwd, "J", "J.txt"), "w").write("jobC 1\nin/c.fasta\n")
    prog = bins["kmer_read_vf6"]
    dump = os.path.join(cwd, "dry.txt")
    subprocess.run([prog, "-name", "DB", "-jname", "J", "--dry-run", dump, "--segments", "1000:500"], cwd=cwd, check=True, stdout=subprocess.PIPE)
    par, _, _, files = parse_dump(dump)
    assert not [f for f in os.listdir(os.path.join(cwd, "J")) if "segments" in f]
    odb = oracle_db(par, keys, targets, 18, flags=ob.KO_FLAG_U_IS_T)
    exp = model_segments_file(odb, keys, targets, par, files[0][1], (1000, 500), (0, 0), u_is_t=True)
    plain = subprocess.run([prog, "-name", "DB", "-jname", "J", "--log2-slots", "18"], cwd=cwd, check=True, stdout=subprocess.PIPE).stdout
    before = {f: open(os.path.join(cwd, "J", f), "rb").read() for f in os.listdir(os.path.join(cwd, "J"))}
    r = subprocess.run([prog, "-name", "DB", "-jname", "J", "--log2-slots", "18", "--segments", "1000:500"], cwd=cwd, check=True, stdout=subprocess.PIPE)
    after = {f: open(os.path.join(cwd, "J", f), "rb").read() for f in os.listdir(os.path.join(cwd, "J"))}
    got = after.pop("jobC_segments.txt")
    assert r.stdout == plain and after == before and got == exp
    lines = got.splitlines()
    assert len(lines) == 2 and b"chimera" in lines[0].split(b"\t")[5] and b"tail" in lines[1].split(b"\t")[5]
    cells = [tuple(int(v) for v in c.split(b":")) for c in lines[0].split(b"\t")[4].split(b" ")]
    assert lines[0].split(b"\t")[2] == b"39" and len(cells) == 39  # 1 + ceil((19971 - 1000) / 500) segments, every one with a hit
    for pos, n_pos, n_kmers, n_hits, final, confident in cells:
        assert n_kmers == n_pos
        if pos + n_pos <= 10000:  # windows of the first genome, at its end the 29 that reach into the second
            assert (final, confident, n_hits) == (8, 8, min(pos + n_pos, 10000 - K + 1) - pos), pos
        elif pos >= 10000:
            assert (final, confident, n_hits) == (x, x, n_pos), pos
        else:  # the one segment that holds both: msca keeps the deeper node of a lineage once the fold has met the root
            assert pos == 9500 and (final, confident, n_hits) == (x, x, n_pos - (K - 1)), pos
    assert min(c[0] for c in cells if c[4] == x) == 9500  # the lineage changes at the right pos
    assert [c[0] for c in cells] == list(range(0, 19500, 500))


def test_m3_runs_once(bins, tmp_path):  # noqa: F811
    cwd = str(tmp_path)
    src, params, wd = setup_m3(cwd)
    keys, targets = probes_of(wd + "mitochondria_probes.txt.gz")
    tag, (f1, f2) = sorted(params["runs"].items())[0]
    files_args = ["-wdir", wd, "-f1", wd + f1, "-f2", (wd + f2) if f2 != "none" else "none"]
    dump = os.path.join(cwd, "dry.txt")
    subprocess.run([bins["kmer_read_m3"]] + files_args + ["--dry-run", dump], cwd=cwd, check=True, stdout=subprocess.PIPE)
    par, _, _, files = parse_dump(dump)
    odb = oracle_db(par, keys, targets, params["log2_slots"], max_probes=16)
    exp = model_segments_file(odb, keys, targets, par, [r for f in files for r in f[1]], (50, 25), (2, 0))
    assert exp.count(b"\n") > 5
    open(wd + "segments.txt", "w").write("left by an earlier run\n")
    subprocess.run([bins["kmer_read_m3"]] + files_args + ["--log2-slots", str(params["log2_slots"]), "--batch-reads", "53", "--segments", "50:25",
                                                          "--min-hits", "2"], cwd=cwd, check=True, stdout=subprocess.PIPE)
    assert open(wd + "segments.txt", "rb").read() == exp
