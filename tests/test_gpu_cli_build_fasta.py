"""kmers-build-signatures --fasta-parse device: the training files go to the GPU as raw bytes, the
selected records are parsed into the build there (skm_build_add_fasta) and the host parses residues
only for the records the selection left out; every output file and stdout are those of the host
parse."""
import os
import struct
import subprocess

import pytest

import oracle.front_ref as fr
from conftest import ROOT

BIN = os.path.join(ROOT, "bin", "kmers-build-signatures")
pytestmark = pytest.mark.gpu

OUTPUTS = ("final.kmers", "function.index", "distinct_functions", "kmer_data.mph", "kmer_data.dat")
ALL_DEVICE = ["--recall-db", "device", "--perfect-hash-source", "device", "--final-kmers-source", "device"]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """the `gaps` tree of tests/test_gpu_cli_recall_source.py (every seventh record without a
    definition line, one deleted fid) and a keep-dir of two more genome files"""
    from signature_kmers_amd import synth
    root = str(tmp_path_factory.mktemp("build_fasta_cli"))
    info = synth.write_dirs(os.path.join(root, "in"), 600, 30, per_file=100, seed=11)
    deleted = None
    for g in info["files"]:
        path = os.path.join(info["ann_dir"], g)
        with open(path) as fh:
            lines = fh.readlines()
        kept = [ln for k, ln in enumerate(lines) if k % 7 != 3]
        if deleted is None:
            deleted = kept[5].split("\t")[0]
        with open(path, "w") as fh:
            fh.writelines(kept)
    dpath = os.path.join(root, "deleted.fids")
    with open(dpath, "w") as fh:
        fh.write(deleted + "\n")
    keep = synth.write_dirs(os.path.join(root, "keep"), 200, 30, per_file=100, seed=11, genome_base=200000)
    args = ["-D", info["ann_dir"], "-D", keep["ann_dir"], "-F", info["seqs_dir"], "-K", keep["seqs_dir"],
            "--deleted-features-file", dpath]
    fasta = [os.path.join(d["seqs_dir"], g) for d in (info, keep) for g in d["files"]]
    return dict(root=root, args=args, fasta=fasta)


def _run(tree, out, extra, env=None):
    cmd = [BIN] + tree["args"] + ["--kmer-data-dir", out, "--final-kmers", "final.kmers", "--perfect-hash", "kmer_data.mph",
                                  "--perfect-hash-data", "kmer_data.dat"] + extra
    return subprocess.run(cmd, capture_output=True, timeout=300, env=dict(os.environ, **(env or {})))


def _phases(p):
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = [ln for ln in p.stderr.decode().splitlines() if ln.startswith("phases: ")]
    assert len(lines) == 1
    w = lines[0].split()[1:]
    return dict(zip(w[0::2], w[1::2]))


def _read(path):
    with open(path, "rb") as fh:
        return fh.read()


@pytest.fixture(scope="module")
def left_out_residues(tree):
    """the residues of the records the selection leaves out: every record's (the pinned parser
    restatement over the files) less those of the build input the host path dumps"""
    total = sum(len(s) for path in tree["fasta"] for _, _, s in fr.parse_fasta(_read(path)))
    dump = os.path.join(tree["root"], "extract.bin")
    p = subprocess.run([BIN] + tree["args"] + ["--dump-extract", dump], capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    n_seqs, n_res = struct.unpack("<QQ", _read(dump)[:16])
    assert 0 < n_res < total and n_seqs > 0
    return total - n_res


@pytest.mark.parametrize("others", ["defaults", "all_device"])
def test_fasta_parse_device_writes_the_same_files(gpu, tree, tmp_path, left_out_residues, others):
    extra = ["--recall-source", "device"] + (ALL_DEVICE if others == "all_device" else [])
    outs, stdout, phases = {}, {}, {}
    # 0.05 MB a group: the eight files (about 30 KB each) go in several skm_build_add_fasta calls
    for mode, more in (("host", []), ("device", ["--fasta-parse", "device", "--fasta-group-mb", "0.05"])):
        outs[mode] = str(tmp_path / ("kd_" + mode))
        p = _run(tree, outs[mode], extra + more)
        phases[mode] = _phases(p)
        stdout[mode] = p.stdout
    assert stdout["host"] == stdout["device"] and len(stdout["host"]) > 0
    for name in OUTPUTS:
        a, b = _read(os.path.join(outs["host"], name)), _read(os.path.join(outs["device"], name))
        assert a == b, name
        assert len(a) > 0, name
    rh, rd = (os.path.join(outs[m], "recall.report.d") for m in ("host", "device"))
    names = sorted(os.listdir(rh))
    assert len(names) == len(tree["fasta"]) and names == sorted(os.listdir(rd))
    for n in names:
        assert _read(os.path.join(rh, n)) == _read(os.path.join(rd, n)), n
    assert sorted(os.listdir(outs["host"])) == sorted(os.listdir(outs["device"]))
    d, h = phases["device"], phases["host"]
    assert "add_fasta" not in h and "host_residue_bytes" not in h  # host mode's line is as it was
    assert float(d["add_fasta"]) > 0
    assert int(d["host_residue_bytes"]) == left_out_residues
    assert (d["recall_resident_seqs"], d["recall_uploaded_seqs"]) == (h["recall_resident_seqs"], h["recall_uploaded_seqs"])
    assert int(d["recall_uploaded_seqs"]) >= 600 // 7


def test_fasta_parse_argument_errors(gpu, tree, tmp_path):
    out = str(tmp_path / "kd")
    p = _run(tree, out, ["--fasta-parse", "device"])
    assert p.returncode == 1 and b"--fasta-parse device needs one GPU and --recall-source device" in p.stderr
    p = _run(tree, out, ["--fasta-parse", "device", "--recall-source", "device", "--n-gpus", "2"])
    assert p.returncode == 1 and b"needs one GPU" in p.stderr  # (--recall-source device says so first)
    p = _run(tree, out, ["--fasta-parse", "gpu"])
    assert p.returncode == 1 and b"--fasta-parse must be host or device" in p.stderr
    assert not os.path.exists(os.path.join(out, "final.kmers"))
    p = subprocess.run([BIN, "--help"], capture_output=True, timeout=60)
    assert b"--fasta-parse" in p.stdout and b"--fasta-group-mb" in p.stdout


def test_a_differing_device_record_count_names_the_file(gpu, tree, tmp_path):
    out = str(tmp_path / "kd")
    p = _run(tree, out, ["--fasta-parse", "device", "--recall-source", "device"], env={"SKM_CLI_FASTA_EXTRA_RECORD": "2"})
    err = p.stderr.decode()
    assert p.returncode == 1, err[-2000:]
    line = [ln for ln in err.splitlines() if ln.startswith("device FASTA parse of ")]
    assert len(line) == 1 and "101 records, the host parse has 100" in line[0]
    assert any(path in line[0] for path in tree["fasta"])
    assert not os.path.exists(os.path.join(out, "final.kmers"))
