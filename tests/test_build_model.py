"""The Python model of kmer_build_vf6 (tests/build_model.py) reproduces every recorded output of the reference byte for
byte: probes file, count file, stdout, stderr and exit status (tests/golden/build_vf6/README.md)."""
import json
import os

import pytest

import build_model

CONFIGS = json.load(open(os.path.join(build_model.GOLD, "configs.json")))


def read(path):
    return open(path, "rb").read().decode() if os.path.exists(path) else None


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_model_matches_reference(cfg, tmp_path):
    c = CONFIGS[cfg]
    build_model.unpack_fixtures(str(tmp_path))
    work = tmp_path / "in"
    status, out, err = build_model.run(str(work), name=c["name"], fadir=c["fadir"], genbank_dir=c["genbank_dir"],
                                       log2_cells=c["log2_cells"], max_probes=c["max_probes"])
    gold = str(tmp_path / "out" / cfg)
    assert status == int(read(os.path.join(gold, "exit.txt")))
    assert out == read(os.path.join(gold, "stdout.txt"))
    assert err == read(os.path.join(gold, "stderr.txt"))
    name = c["name"]
    assert read(str(work / name / (name + "_probes.txt"))) == read(os.path.join(gold, "probes.txt"))
    assert read(str(work / name / (name + "_count.txt"))) == read(os.path.join(gold, "count.txt"))


def test_entropy_rules():
    key = lambda s: int("".join("%d" % "ACGT".index(c) for c in s), 4)
    assert build_model.entropy_flags(key("A" * 12 + "CGTACGTAGCTAGCTGAT")) == (False, False)  # run of 12
    assert build_model.entropy_flags(key("ACGTTGCAGTCATGACCGTAGCTAGCATGC")) == (True, False)
    assert build_model.entropy_flags(key("AC" * 15)) == (False, False)
    assert build_model.minct(0) == 2 and build_model.minct(1) == 1 and build_model.minct(9) == 7 and build_model.minct(10) == 3
