"""kmers-build-signatures --recall-source: the recall pass over the build's resident sequences
(skm_build_recall), with only the records the selection left out uploaded, writes the same files
and the same stdout as the host path that uploads every protein again."""
import os
import subprocess

import pytest

from conftest import ROOT

BIN = os.path.join(ROOT, "bin", "kmers-build-signatures")
pytestmark = pytest.mark.gpu

OUTPUTS = ("final.kmers", "function.index", "distinct_functions", "kmer_data.mph", "kmer_data.dat")
ALL_DEVICE = ["--recall-db", "device", "--perfect-hash-source", "device", "--final-kmers-source", "device"]
N_GAPS = 600


def _tree(kind, root):
    """c1: the C1 tree of tests/test_gpu_cli.py (1000 proteins, 40 families, 10 genome files).
    gaps: 600 proteins in 6 files where every seventh record has no definition line and one fid is
    in the deleted-features file -- records the build's selection leaves out."""
    from signature_kmers_amd import synth
    if kind == "c1":
        info = synth.write_dirs(os.path.join(root, "in"), 1000, 40, per_file=100, extras=True)
        return ["-D", info["ann_dir"], "-F", info["seqs_dir"]]
    info = synth.write_dirs(os.path.join(root, "in"), N_GAPS, 30, per_file=100, seed=11)
    deleted = None
    for g in info["files"]:
        path = os.path.join(info["ann_dir"], g)
        with open(path) as fh:
            lines = fh.readlines()
        kept = [ln for k, ln in enumerate(lines) if k % 7 != 3]
        if deleted is None:
            deleted = kept[5].split("\t")[0]  # a record that has a definition
        with open(path, "w") as fh:
            fh.writelines(kept)
    dpath = os.path.join(root, "deleted.fids")
    with open(dpath, "w") as fh:
        fh.write(deleted + "\n")
    return ["-D", info["ann_dir"], "-F", info["seqs_dir"], "--deleted-features-file", dpath]


def _build(args, out, source, extra):
    cmd = [BIN] + args + ["--kmer-data-dir", out, "--final-kmers", "final.kmers", "--perfect-hash", "kmer_data.mph",
                          "--perfect-hash-data", "kmer_data.dat", "--recall-source", source] + extra
    p = subprocess.run(cmd, capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    phases = [ln for ln in p.stderr.decode().splitlines() if ln.startswith("phases: ")]
    assert len(phases) == 1
    w = phases[0].split()[1:]
    return p.stdout, dict(zip(w[0::2], w[1::2]))


def _read(path):
    with open(path, "rb") as fh:
        return fh.read()


@pytest.mark.parametrize("others", ["defaults", "all_device"])
@pytest.mark.parametrize("kind", ["c1", "gaps"])
def test_recall_source_device_writes_the_same_files(gpu, tmp_path, kind, others):
    args = _tree(kind, str(tmp_path))
    extra = ALL_DEVICE if others == "all_device" else []
    outs, stdout, phases = {}, {}, {}
    for source in ("host", "device"):
        outs[source] = str(tmp_path / ("kd_" + source))
        stdout[source], phases[source] = _build(args, outs[source], source, extra)
    assert stdout["host"] == stdout["device"]
    for name in OUTPUTS:
        a, b = _read(os.path.join(outs["host"], name)), _read(os.path.join(outs["device"], name))
        assert a == b, name
        assert len(a) > 0, name
    rh, rd = (os.path.join(outs[m], "recall.report.d") for m in ("host", "device"))
    names = sorted(os.listdir(rh))
    assert names and names == sorted(os.listdir(rd))
    for n in names:
        assert _read(os.path.join(rh, n)) == _read(os.path.join(rd, n)), n
    assert sorted(os.listdir(outs["host"])) == sorted(os.listdir(outs["device"]))
    res, up = int(phases["device"]["recall_resident_seqs"]), int(phases["device"]["recall_uploaded_seqs"])
    assert int(phases["device"]["recall_batches"]) >= 1
    assert "recall_resident_seqs" not in phases["host"]  # host mode's line is as it was
    assert list(phases["device"])[-3:] == ["recall_resident_seqs", "recall_uploaded_seqs", "recall_batches"]
    if kind == "gaps":
        assert res > 0 and up > 0
        assert res + up == N_GAPS
        assert up >= N_GAPS // 7  # the records without a definition and the deleted one, at least
    else:
        assert res > 0


def test_recall_source_argument_errors(gpu, tmp_path):
    args = _tree("gaps", str(tmp_path))
    for extra in (["--recall-source", "device", "--n-gpus", "2"], ["--recall-source", "gpu"]):
        p = subprocess.run([BIN] + args + ["--kmer-data-dir", str(tmp_path / "kd"), "--final-kmers", "final.kmers"] + extra,
                           capture_output=True, timeout=120)
        assert p.returncode != 0, extra
        assert b"--recall-source" in p.stderr, p.stderr[-500:]
        assert not os.path.exists(str(tmp_path / "kd" / "final.kmers"))
