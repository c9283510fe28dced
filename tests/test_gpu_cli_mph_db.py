"""kmers-build-signatures --perfect-hash-source: the perfect hash and its data file written from the
BDZ DB built on the device from the build's resident kept k-mers (skm_build_mph_db) are the host
path's, byte for byte, and so is every other output -- alone and together with --recall-db device."""
import os
import subprocess

import pytest

from conftest import ROOT
from test_gpu_cli_kept_db import OUTPUTS, _read, _tree

BIN = os.path.join(ROOT, "bin", "kmers-build-signatures")
pytestmark = pytest.mark.gpu


def _build(args, out, extra):
    cmd = [BIN] + args + ["--kmer-data-dir", out, "--final-kmers", "final.kmers", "--perfect-hash", "kmer_data.mph",
                          "--perfect-hash-data", "kmer_data.dat", "--mph-seed", "5"] + extra
    p = subprocess.run(cmd, capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return p.stdout


@pytest.mark.parametrize("kind", ["c1", "edge"])
def test_perfect_hash_source_device_writes_the_same_files(gpu, tmp_path, kind):
    args = _tree(kind, str(tmp_path))
    modes = {"host": ["--perfect-hash-source", "host"], "device": ["--perfect-hash-source", "device"],
             "both": ["--perfect-hash-source", "device", "--recall-db", "device"]}
    outs, stdout = {}, {}
    for mode, extra in modes.items():
        outs[mode] = str(tmp_path / ("kd_" + mode))
        stdout[mode] = _build(args, outs[mode], extra)
    names = sorted(os.listdir(os.path.join(outs["host"], "recall.report.d")))
    assert names
    for mode in ("device", "both"):
        assert stdout[mode] == stdout["host"], mode
        for name in OUTPUTS:
            a, b = _read(os.path.join(outs["host"], name)), _read(os.path.join(outs[mode], name))
            assert a == b, (mode, name)
            assert len(a) > 0, name
        assert names == sorted(os.listdir(os.path.join(outs[mode], "recall.report.d")))
        for n in names:
            assert _read(os.path.join(outs["host"], "recall.report.d", n)) == \
                _read(os.path.join(outs[mode], "recall.report.d", n)), (mode, n)


def test_perfect_hash_source_argument_errors(gpu, tmp_path):
    args = _tree("edge", str(tmp_path))
    ph = ["--perfect-hash", "kmer_data.mph", "--perfect-hash-data", "kmer_data.dat"]
    for extra in (ph + ["--perfect-hash-source", "device", "--n-gpus", "2"], ph + ["--perfect-hash-source", "gpu"],
                  ["--perfect-hash-source", "device"]):
        p = subprocess.run([BIN] + args + ["--kmer-data-dir", str(tmp_path / "kd"), "--final-kmers", "final.kmers"] + extra,
                           capture_output=True, timeout=120)
        assert p.returncode != 0, extra
        assert b"--perfect-hash-source" in p.stderr, p.stderr[-500:]
        assert not os.path.exists(str(tmp_path / "kd" / "final.kmers"))
