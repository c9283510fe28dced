"""kmers-call-functions and kmers-annotate-seqs with --fasta-parse device against --fasta-parse
host (today's path): the same output files, the same parse error reports, the same exit status."""
import os
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "bin")


def _run(cmd):
    p = subprocess.run(cmd, capture_output=True, timeout=300)
    return p.returncode, p.stdout, p.stderr


@pytest.fixture(scope="module")
def data_and_queries(tmp_path_factory, gpu):
    from signature_kmers_amd import synth
    tmp = tmp_path_factory.mktemp("cli_fasta")
    info = synth.write_dirs(str(tmp / "in"), 1000, 40, per_file=100, extras=True)
    kd = str(tmp / "kd")
    rc, _, err = _run([os.path.join(BIN, "kmers-build-signatures"), "-D", info["ann_dir"], "-F", info["seqs_dir"],
                       "--kmer-data-dir", kd, "--final-kmers", "final.kmers", "--perfect-hash", "kmer_data.mph",
                       "--perfect-hash-data", "kmer_data.dat"])
    assert rc == 0, err.decode()[-2000:]
    # a few hundred query sequences in several files, and the awkward files beside them
    qdir = synth.write_dirs(str(tmp / "q"), 300, 40, per_file=100, seed=5, extras=True, genome_base=200000)["seqs_dir"]
    plain = sorted(os.listdir(qdir))
    body = open(os.path.join(qdir, plain[0]), "rb").read()
    with open(os.path.join(qdir, "300000.1"), "wb") as f:  # CRLF line ends
        f.write(body.replace(b"\n", b"\r\n"))
    open(os.path.join(qdir, "300001.1"), "wb").close()      # empty
    recs = [r for r in body.split(b">")[1:] if len(r) > 150][:3]
    assert len(recs) == 3
    mid = recs[0].index(b"\n") + 11  # inside the first sequence line
    with open(os.path.join(qdir, "300002.1"), "wb") as f:  # junk before the first '>', a bad data character
        f.write(b"no header here\nMKV\n>" + recs[0][:mid] + b"7" + recs[0][mid:] + b">" + recs[1])
    with open(os.path.join(qdir, "300003.1"), "wb") as f:  # a record with an empty id between two others
        f.write(b">" + recs[0] + b"> no id\n" + recs[1].split(b"\n", 1)[1] + b">" + recs[2].rstrip(b"\n"))
    return kd, qdir


def _error_lines(stderr: bytes):
    return sorted(ln for ln in stderr.splitlines() if ln.startswith(b"Error found"))


def test_call_functions_device_parse_equals_host_parse(data_and_queries, tmp_path):
    kd, qdir = data_and_queries
    inputs = sorted(os.path.join(qdir, f) for f in os.listdir(qdir))
    got = {}
    for mode in ("host", "device"):
        out = str(tmp_path / f"calls.{mode}")
        rc, _, err = _run([os.path.join(BIN, "kmers-call-functions"), kd] + inputs + ["-o", out, "--fasta-parse", mode])
        got[mode] = (rc, open(out, "rb").read(), _error_lines(err))
    assert got["host"][0] == 0, got["host"]
    assert got["device"] == got["host"]
    calls, errors = got["host"][1], got["host"][2]
    assert calls.count(b"\n") > 400 and b"\tfunction " in calls
    assert any(b"Missing >" in e for e in errors) and any(b"Bad data character '7'" in e for e in errors)
    # the default is the host parse
    out = str(tmp_path / "calls.default")
    rc, _, err = _run([os.path.join(BIN, "kmers-call-functions"), kd] + inputs + ["-o", out])
    assert (rc, open(out, "rb").read(), _error_lines(err)) == got["host"]


def test_annotate_seqs_device_parse_equals_host_parse(data_and_queries, tmp_path):
    kd, qdir = data_and_queries
    got = {}
    for mode in ("host", "device"):
        calls, unc = str(tmp_path / f"calls.{mode}"), str(tmp_path / f"uncalled.{mode}")
        rc, _, err = _run([os.path.join(BIN, "kmers-annotate-seqs"), kd, str(tmp_path / "genus"), qdir, calls, unc,
                           "--fasta-parse", mode])
        assert rc == 0, err.decode()[-2000:]
        got[mode] = (rc, open(calls, "rb").read(), open(unc, "rb").read(), _error_lines(err))
    assert got["device"] == got["host"]  # the uncalled ids in the order the host parse gives
    assert got["host"][1].count(b"\n") > 100 and got["host"][2].count(b"\n") > 0
    assert len(got["host"][3]) > 0
