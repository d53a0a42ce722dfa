"""kmer_build_vf6 on the GPU: the command-line program against the reference's recorded outputs, the library's table
against the Python model (tests/build_model.py), the device's entropy test against Python's, the reference table size,
and a database round trip through kmer_read_vf6."""
import gzip
import json
import math
import os
import random
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import build_model  # noqa: E402

from kmer_id_amd import _build  # noqa: E402
from kmer_id_amd.builder import ProbeBuilder, device_mem_info  # noqa: E402

pytestmark = pytest.mark.gpu

CONFIGS = json.load(open(os.path.join(build_model.GOLD, "configs.json")))
BUILD = _build.cli_path("kmer_build_vf6")


def read(path):
    return open(path, "rb").read().decode() if os.path.exists(path) else None


def run_cli(cwd, name, args, timeout=600):
    r = subprocess.run([BUILD, "-name", name] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    return r.returncode, r.stdout.decode(), r.stderr.decode()


def cfg_args(c):
    return ["-fadir", c["fadir"], "--genbank-dir", c["genbank_dir"], "--log2-cells", str(c["log2_cells"]), "--max-probes", str(c["max_probes"])]


@pytest.mark.parametrize("batch", [0, 4096])
@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_cli_matches_reference(cfg, batch, tmp_path):
    c = CONFIGS[cfg]
    build_model.unpack_fixtures(str(tmp_path))
    work = tmp_path / "in"
    args = cfg_args(c) + (["--batch-bases", str(batch)] if batch else [])
    status, out, err = run_cli(str(work), c["name"], args)
    gold = str(tmp_path / "out" / cfg)
    assert status == int(read(os.path.join(gold, "exit.txt"))), err
    assert out == read(os.path.join(gold, "stdout.txt"))
    assert err == read(os.path.join(gold, "stderr.txt"))
    name = c["name"]
    assert read(str(work / name / (name + "_probes.txt"))) == read(os.path.join(gold, "probes.txt"))
    assert read(str(work / name / (name + "_count.txt"))) == read(os.path.join(gold, "count.txt"))


# ---- library level: random genomes and trees ------------------------------------------------------------------------
def random_case(seed):
    rng = random.Random(seed)
    nrng = np.random.default_rng(seed)
    ntar = rng.randrange(6, 14)
    parent = [1] * ntar
    for v in range(3, ntar):
        parent[v] = rng.randrange(1, v) if rng.random() < 0.8 else 1
    parent[2] = 1
    root = nrng.integers(0, 4, 6000)
    seqs = []
    for _ in range(rng.randrange(4, 9)):
        t = rng.randrange(2, ntar)
        g = root.copy()
        g[nrng.random(g.size) < rng.choice([0.002, 0.02, 0.1])] = nrng.integers(0, 4)
        s = "".join("ACGT"[x] for x in g)
        if rng.random() < 0.3:
            s = s[:100] + "N" + s[100:3000] + "RYN" + s[3000:]
        seqs.append((t, s))
    if seed % 3 == 0:  # a 30-mer past the count limit
        rep = "".join(rng.choice("ACGT") for _ in range(30))
        seqs.append((seqs[0][0], "N".join([rep] * 2100)))
    outs = ["".join(rng.choice("ACGT") for _ in range(800)) + seqs[i % len(seqs)][1][500:1500] for i in range(2)]
    return parent, seqs, outs, 12 + seed % 9


def compare(model, cells):
    idx = np.fromiter(model.cells.keys(), np.int64, len(model.cells))
    val = np.fromiter(model.cells.values(), np.int64, len(model.cells))
    dense = np.zeros(cells.size, np.int64)
    dense[idx] = val
    live = (dense >> 11) > 1
    assert np.array_equal(cells[live], dense[live])
    assert np.array_equal(cells == 0, dense == 0)
    assert not np.any((cells[~live] >> 11) > 1)


@pytest.mark.parametrize("seed", range(20))
def test_library_matches_model(seed):
    parent, seqs, outs, log2 = random_case(seed)
    tree = build_model.Tree(len(parent))
    tree.parent = list(parent)
    model = build_model.Table(log2, tree)
    with ProbeBuilder(parent, log2_cells=log2, batch_bases=1 << (10 + seed % 8)) as b:
        for t, s in seqs:
            build_model.add_seq(model, s, t)
            b.add(s, t)
        assert b.size() == model.size
        compare(model, b.export())
        for s in outs:
            build_model.remove_seq(model, s)
            b.remove(s)
        compare(model, b.export())
        ntargorgs = [0] * len(parent)
        for t, _ in seqs:
            ntargorgs[t] += 1
        b.set_minct([build_model.minct(n) for n in ntargorgs])
        for org, (t, s) in enumerate(seqs):
            got = b.claim(s)
            exp = []
            for gpos, f, r in build_model.kmers(s):
                key = min(f, r)
                tt, c = model.take(key)
                if tt > 1 and c >= build_model.minct(ntargorgs[tt]):
                    ok, bad = build_model.entropy_flags(key)
                    exp.append((key, gpos, tt, c, int(f >= r), int(ok) | (2 if bad else 0)))
            assert [tuple(int(x) for x in row) for row in got[["key", "gpos", "target", "count", "strand_r", "flags"]].tolist()] == exp


# ---- the entropy test -------------------------------------------------------------------------------------------------
def entropy_numpy(keys):
    """check_entropy vectorised: the same p*log10(p) values (math.log10) and the same order of operations"""
    n = keys.size
    bases = np.stack([(keys >> np.uint64(2 * (29 - i))) & np.uint64(3) for i in range(30)], 1).astype(np.int64)
    run = np.ones(n, np.int64)
    maxrow = np.zeros(n, np.int64)
    for i in range(1, 30):
        same = bases[:, i] == bases[:, i - 1]
        run = np.where(same, run + 1, 1)
        maxrow = np.where(same, np.maximum(maxrow, run), maxrow)
    ent = []
    for mod, tot in ((2, 19), (3, 14), (5, 10)):
        term = np.array([0.0] + [(v / tot) * math.log10(v / tot) for v in range(1, tot + 1)])
        for fr in range(mod):
            cols = bases[:, fr::mod]
            cnt = [1 + (cols == b).sum(1) for b in range(4)]
            e = -term[cnt[0]]
            e = e - term[cnt[1]]
            e = e - term[cnt[2]]
            e = e - term[cnt[3]]
            ent.append(e)
    l4 = math.log10(4.0)
    e2 = (ent[0] + ent[1]) / 2.0 / l4
    e3 = (ent[2] + ent[3] + ent[4]) / 3.0 / l4
    e5 = (ent[5] + ent[6] + ent[7] + ent[8] + ent[9]) / 5.0 / l4
    ok = (maxrow <= 11) & (e2 >= 0.80) & (e3 >= 0.80) & (e5 >= 0.80)
    bad = ((keys & np.uint64(0x3333333333333333)) == 0) | ((keys & np.uint64(0xCCCCCCCCCCCCCCCC)) == 0)
    return ok.astype(np.uint8) | ((ok & bad).astype(np.uint8) << 1)


def entropy_keys(n, seed=7):
    rng = np.random.default_rng(seed)
    parts = [rng.integers(0, 1 << 60, n // 3, dtype=np.uint64)]
    # low complexity: biased alphabets, short periods with some mutations
    probs = rng.dirichlet([0.4] * 4, n // 3)
    cum = probs.cumsum(1)
    u = rng.random((n // 3, 30))
    b = (u[:, :, None] > cum[:, None, :3]).sum(2).astype(np.uint64)
    per = rng.integers(1, 7, n - 2 * (n // 3))
    unit = rng.integers(0, 4, (per.size, 6))
    rep = unit[np.arange(per.size)[:, None], np.arange(30)[None, :] % per[:, None]]
    mut = rng.random(rep.shape) < 0.12
    rep = np.where(mut, rng.integers(0, 4, rep.shape), rep).astype(np.uint64)
    keys = []
    for arr in (b, rep):
        k = np.zeros(arr.shape[0], np.uint64)
        for i in range(30):
            k = (k << np.uint64(2)) | arr[:, i]
        keys.append(k)
    return np.concatenate(parts + keys)


def test_entropy_flags_match_python():
    keys = entropy_keys(1_050_000)
    exp = entropy_numpy(keys)
    sub = keys[:: 997]
    assert [build_model.entropy_flags(int(k)) for k in sub.tolist()] == [(bool(v & 1), bool(v & 2)) for v in exp[:: 997].tolist()]
    assert 0.05 < (exp & 1).mean() < 0.95  # both sides of the edge are exercised
    with ProbeBuilder([1, 1, 1], log2_cells=10) as b:
        got = b.entropy(keys)
    assert np.array_equal(got, exp)


# ---- the reference's table size -------------------------------------------------------------------------------------
def write_genome_set(d, seed, n_orgs, length):
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(d, "fs", "fa"), exist_ok=True)
    edges = [(1, 2), (1, 3), (2, 4), (2, 5), (3, 6), (3, 7)]
    node = {1: rng.integers(0, 4, length)}
    for p, c in edges:
        g = node[p].copy()
        m = rng.random(length) < 0.01
        g[m] = rng.integers(0, 4, int(m.sum()))
        node[c] = g
    data = []
    for o in range(n_orgs):
        t = 4 + o % 4
        g = node[t].copy()
        m = rng.random(length) < 0.003
        g[m] = rng.integers(0, 4, int(m.sum()))
        s = np.frombuffer(b"ACGT", np.uint8)[g].tobytes()
        lines = b"\n".join(s[i:i + 80] for i in range(0, len(s), 80))
        acc = "S%02d" % o
        with open(os.path.join(d, "fs", "fa", acc + ".fasta.gz"), "wb") as f:
            f.write(gzip.compress(b">" + acc.encode() + b"\n" + lines + b"\n", 1))
        data.append((t, acc))
    open(os.path.join(d, "fs", "fs_data.txt"), "w").write("".join("%d %s\n" % x for x in data))
    open(os.path.join(d, "fs", "fs_tree.txt"), "w").write("".join("%d %d\n" % e for e in edges))
    return data


def test_reference_table_size(tmp_path):
    free, total = device_mem_info(0)
    if free < 136 << 30:
        pytest.skip("2^35 cells need 128 GiB of device memory; %.1f GiB free" % (free / 2**30))
    d = str(tmp_path)
    write_genome_set(d, 35, 10, 500_000)
    status, out, err = run_cli(d, "fs", ["-fadir", "fs/fa/", "--genbank-dir", "nowhere/"], timeout=900)
    assert status == 0, err
    probes = read(os.path.join(d, "fs", "fs_probes.txt"))
    counts = read(os.path.join(d, "fs", "fs_count.txt"))
    os.makedirs(os.path.join(d, "m"))
    shutil.copytree(os.path.join(d, "fs"), os.path.join(d, "m", "fs"))
    mstatus, mout, _ = build_model.run(os.path.join(d, "m"), name="fs", fadir=os.path.join(d, "fs", "fa") + "/", genbank_dir="nowhere/",
                                       log2_cells=35)
    assert mstatus == 0
    assert out == mout
    assert probes == read(os.path.join(d, "m", "fs", "fs_probes.txt"))
    assert counts == read(os.path.join(d, "m", "fs", "fs_count.txt"))
    assert len(probes) > 1000


# ---- round trip: genomes -> database -> classification ----------------------------------------------------------------
def test_round_trip_through_kmer_read_vf6(tmp_path):
    d = str(tmp_path)
    data = write_genome_set(d, 6, 8, 40_000)
    parent = {2: 1, 3: 1, 4: 2, 5: 2, 6: 3, 7: 3}
    status, out, err = run_cli(d, "fs", ["-fadir", "fs/fa/", "--log2-cells", "24"])
    assert status == 0, err
    with open(os.path.join(d, "fs", "fs_probes.txt"), "rb") as f, gzip.open(os.path.join(d, "fs", "fs_probes.txt.gz"), "wb") as g:
        g.write(f.read())
    # error-free reads sampled from the ingroup genomes
    rng = random.Random(3)
    reads = []
    for o, (t, acc) in enumerate(data[:4]):
        g = build_model.read_gz(os.path.join(d, "fs", "fa", acc + ".fasta.gz")).replace("N", "")
        for r in range(40):
            a = rng.randrange(0, len(g) - 150)
            reads.append(">o%d_%d\n%s\n" % (o, r, g[a:a + 150]))
    os.makedirs(os.path.join(d, "J", "in"))
    open(os.path.join(d, "J", "in", "r.fasta"), "w").write("".join(reads))
    open(os.path.join(d, "J", "J.txt"), "w").write("job 1\nJ/in/r.fasta\n")
    r = subprocess.run([_build.cli_path("kmer_read_vf6"), "-name", "fs", "-jname", "J", "--log2-slots", "22"], cwd=d,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()

    def anc(t):
        out = {t}
        while t in parent:
            t = parent[t]
            out.add(t)
        return out

    allowed = set().union(*(anc(t) for t, _ in data[:4])) | {0, 1}
    for line in open(os.path.join(d, "J", "job_result.txt")):
        t, g, _ = (int(x) for x in line.split(","))
        if g > 0:
            assert t in allowed, line
    hit = set()
    text = open(os.path.join(d, "J", "job_reads.txt")).read()
    for m in re.finditer(r"^>(\d+):\S*?o(\d+)_\d+", text, re.M):
        t, o = int(m.group(1)), int(m.group(2))
        assert t in anc(data[o][0]) | {0, 1}
        if t > 1:
            hit.add(o)
    assert hit == set(range(4))
