"""kmers-build-signatures --recall-db: the recall pass over the DB built on the device from the
build's resident kept k-mers (skm_build_kept_db) writes the same files as the host path."""
import os
import subprocess

import pytest

import front_data
from conftest import ROOT

BIN = os.path.join(ROOT, "bin", "kmers-build-signatures")
pytestmark = pytest.mark.gpu

OUTPUTS = ("final.kmers", "function.index", "distinct_functions", "kmer_data.mph", "kmer_data.dat")


def _tree(kind, root):
    """The input trees of tests/test_gpu_cli.py: its C1 tree (1000 proteins, 40 families, 10 genome
    files) and front_data's edge-case directories."""
    if kind == "c1":
        from signature_kmers_amd import synth
        info = synth.write_dirs(os.path.join(root, "in"), 1000, 40, per_file=100, extras=True)
        return ["-D", info["ann_dir"], "-F", info["seqs_dir"]]
    return front_data.front_args(front_data.write_edge_dirs(os.path.join(root, "in")))


def _build(args, out, mode):
    cmd = [BIN] + args + ["--kmer-data-dir", out, "--final-kmers", "final.kmers", "--perfect-hash", "kmer_data.mph",
                          "--perfect-hash-data", "kmer_data.dat"]
    if mode is not None:
        cmd += ["--recall-db", mode]
    p = subprocess.run(cmd, capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return p.stdout


def _read(path):
    with open(path, "rb") as fh:
        return fh.read()


@pytest.mark.parametrize("kind", ["c1", "edge"])
def test_recall_db_device_writes_the_same_files(gpu, tmp_path, kind):
    args = _tree(kind, str(tmp_path))
    outs = {}
    for mode in ("host", "device"):
        outs[mode] = str(tmp_path / ("kd_" + mode))
        stdout = _build(args, outs[mode], mode)
        outs[mode + "_stdout"] = stdout
    assert outs["host_stdout"] == outs["device_stdout"]
    for name in OUTPUTS:
        a, b = _read(os.path.join(outs["host"], name)), _read(os.path.join(outs["device"], name))
        assert a == b, name
        assert len(a) > 0, name
    rh, rd = (os.path.join(outs[m], "recall.report.d") for m in ("host", "device"))
    names = sorted(os.listdir(rh))
    assert names and names == sorted(os.listdir(rd))
    for n in names:
        assert _read(os.path.join(rh, n)) == _read(os.path.join(rd, n)), n


def test_recall_db_argument_errors(gpu, tmp_path):
    args = _tree("edge", str(tmp_path))
    for extra in (["--recall-db", "device", "--n-gpus", "2"], ["--recall-db", "gpu"]):
        p = subprocess.run([BIN] + args + ["--kmer-data-dir", str(tmp_path / "kd")] + extra, capture_output=True,
                           timeout=120)
        assert p.returncode != 0, extra
        assert b"--recall-db" in p.stderr, p.stderr[-500:]
        assert not os.path.exists(str(tmp_path / "kd" / "final.kmers"))
