"""kmers-build-signatures --final-kmers-source: final.kmers sorted, formatted and streamed out by
the GPU from the build's resident kept k-mers (skm_build_write_final_kmers) is the host writer's
file byte for byte, every other output is unchanged, and with all three sources on `device` the
kept set never comes to the host."""
import os
import subprocess

import pytest

import front_data
from conftest import ROOT

BIN = os.path.join(ROOT, "bin", "kmers-build-signatures")
pytestmark = pytest.mark.gpu

OUTPUTS = ("final.kmers", "function.index", "distinct_functions", "kmer_data.mph", "kmer_data.dat")


def _tree(kind, root):
    """The input trees of tests/test_gpu_cli_kept_db.py: the C1 tree (1000 proteins, 40 families, 10
    genome files) and front_data's edge-case directories."""
    if kind == "c1":
        from signature_kmers_amd import synth
        info = synth.write_dirs(os.path.join(root, "in"), 1000, 40, per_file=100, extras=True)
        return ["-D", info["ann_dir"], "-F", info["seqs_dir"]]
    return front_data.front_args(front_data.write_edge_dirs(os.path.join(root, "in")))


def _build(args, out, extra):
    cmd = [BIN] + args + ["--kmer-data-dir", out, "--final-kmers", "final.kmers", "--perfect-hash", "kmer_data.mph",
                          "--perfect-hash-data", "kmer_data.dat"] + extra
    p = subprocess.run(cmd, capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    phases = [ln for ln in p.stderr.decode().splitlines() if ln.startswith("phases: ")][-1].split()[1:]
    return p.stdout, dict(zip(phases[0::2], phases[1::2]))


def _read(path):
    with open(path, "rb") as fh:
        return fh.read()


def _assert_same_outputs(a_dir, b_dir, a_stdout, b_stdout):
    assert a_stdout == b_stdout
    for name in OUTPUTS:
        a, b = _read(os.path.join(a_dir, name)), _read(os.path.join(b_dir, name))
        assert a == b, name
        assert len(a) > 0, name
    ra, rb = (os.path.join(d, "recall.report.d") for d in (a_dir, b_dir))
    names = sorted(os.listdir(ra))
    assert names and names == sorted(os.listdir(rb))
    for n in names:
        assert _read(os.path.join(ra, n)) == _read(os.path.join(rb, n)), n


MODES = {
    "host": ["--final-kmers-source", "host"],
    "device": ["--final-kmers-source", "device"],
    "all_device": ["--final-kmers-source", "device", "--recall-db", "device", "--perfect-hash-source", "device"],
}


@pytest.mark.parametrize("kind", ["c1", "edge"])
def test_final_kmers_source_device_writes_the_same_files(gpu, tmp_path, kind):
    args = _tree(kind, str(tmp_path))
    out, stdout, phases = {}, {}, {}
    for mode, extra in MODES.items():
        out[mode] = str(tmp_path / ("kd_" + mode))
        stdout[mode], phases[mode] = _build(args, out[mode], extra)
    for mode in ("device", "all_device"):
        _assert_same_outputs(out["host"], out[mode], stdout["host"], stdout[mode])
    # the host copy of the kept set: 8 + 10 bytes per kept k-mer, or none at all
    kept = int([ln for ln in stdout["host"].decode().splitlines() if ln.startswith("Kept ")][0].split()[1])
    assert kept == _read(os.path.join(out["host"], "final.kmers")).count(b"\n") and kept > 0
    assert list(phases["all_device"])[-1] == "kept_host_bytes"
    assert phases["all_device"]["kept_host_bytes"] == "0"
    assert phases["host"]["kept_host_bytes"] == phases["device"]["kept_host_bytes"] == str(18 * kept)


def test_final_kmers_source_argument_errors(gpu, tmp_path):
    args = _tree("edge", str(tmp_path))
    kd = str(tmp_path / "kd")
    for extra in (["--final-kmers-source", "device"],
                  ["--final-kmers", "final.kmers", "--final-kmers-source", "device", "--n-gpus", "2"],
                  ["--final-kmers", "final.kmers", "--final-kmers-source", "gpu"]):
        p = subprocess.run([BIN] + args + ["--kmer-data-dir", kd] + extra, capture_output=True, timeout=120)
        assert p.returncode != 0, extra
        assert b"--final-kmers-source" in p.stderr, p.stderr[-500:]
        assert not os.path.exists(os.path.join(kd, "final.kmers"))
