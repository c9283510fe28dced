"""kmers-call-functions, kmers-annotate-seqs and kmers-build-signatures (its recall pass) with
--best-call device against --best-call host (today's path): the same output files, the same parse
error reports, the same exit status; leaving the option out is host."""
import hashlib
import os
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "bin")


def _run(cmd):
    p = subprocess.run(cmd, capture_output=True, timeout=300)
    return p.returncode, p.stdout, p.stderr


def _build(info, kd, *extra):
    return _run([os.path.join(BIN, "kmers-build-signatures"), "-D", info["ann_dir"], "-F", info["seqs_dir"],
                 "--kmer-data-dir", kd, "--final-kmers", "final.kmers", "--perfect-hash", "kmer_data.mph",
                 "--perfect-hash-data", "kmer_data.dat", *extra])


@pytest.fixture(scope="module")
def data_and_queries(tmp_path_factory, gpu):
    """The small generated directories of test_gpu_cli_fasta_device.py: a built data directory, and
    query files with CRLF line ends, an empty file, junk, a bad character and an empty id."""
    from signature_kmers_amd import synth
    tmp = tmp_path_factory.mktemp("cli_best")
    info = synth.write_dirs(str(tmp / "in"), 1000, 40, per_file=100, extras=True)
    kd = str(tmp / "kd")
    rc, _, err = _build(info, kd)
    assert rc == 0, err.decode()[-2000:]
    qdir = synth.write_dirs(str(tmp / "q"), 300, 40, per_file=100, seed=5, extras=True, genome_base=200000)["seqs_dir"]
    plain = sorted(os.listdir(qdir))
    body = open(os.path.join(qdir, plain[0]), "rb").read()
    with open(os.path.join(qdir, "300000.1"), "wb") as f:
        f.write(body.replace(b"\n", b"\r\n"))
    open(os.path.join(qdir, "300001.1"), "wb").close()
    recs = [r for r in body.split(b">")[1:] if len(r) > 150][:3]
    mid = recs[0].index(b"\n") + 11
    with open(os.path.join(qdir, "300002.1"), "wb") as f:
        f.write(b"no header here\nMKV\n>" + recs[0][:mid] + b"7" + recs[0][mid:] + b">" + recs[1])
    with open(os.path.join(qdir, "300003.1"), "wb") as f:
        f.write(b">" + recs[0] + b"> no id\n" + recs[1].split(b"\n", 1)[1] + b">" + recs[2].rstrip(b"\n"))
    return info, kd, qdir


def _error_lines(stderr: bytes):
    return sorted(ln for ln in stderr.splitlines() if ln.startswith(b"Error found"))


def _phases(stderr: bytes) -> dict:
    f = [ln for ln in stderr.decode().splitlines() if ln.startswith("phases: ")][-1].split()[1:]
    return {f[i]: float(f[i + 1]) for i in range(0, len(f) - 1, 2)}


MODES = {"host": ["--best-call", "host"], "device": ["--best-call", "device"], "default": [],
         "device+parse": ["--best-call", "device", "--fasta-parse", "device"]}


def test_call_functions(data_and_queries, tmp_path):
    _, kd, qdir = data_and_queries
    inputs = sorted(os.path.join(qdir, f) for f in os.listdir(qdir))
    got = {}
    for mode, opts in MODES.items():
        out = str(tmp_path / f"calls.{mode}")
        rc, _, err = _run([os.path.join(BIN, "kmers-call-functions"), kd] + inputs + ["-o", out] + opts)
        got[mode] = (rc, open(out, "rb").read(), _error_lines(err))
        assert rc == 0 and _phases(err)["deferred"] == 0, err.decode()[-2000:]
    for mode in MODES:
        assert got[mode] == got["host"], mode
    calls, errors = got["host"][1], got["host"][2]
    assert calls.count(b"\n") > 400 and b"\tfunction " in calls and b" ?? " in calls
    assert any(b"Missing >" in e for e in errors) and any(b"Bad data character '7'" in e for e in errors)
    rc, _, err = _run([os.path.join(BIN, "kmers-call-functions"), kd] + inputs[:1] + ["--best-call", "gpu"])
    assert rc == 1 and b"--best-call must be host or device" in err


def test_call_functions_debug_hits_keeps_working(data_and_queries, tmp_path):
    _, kd, qdir = data_and_queries
    inputs = sorted(os.path.join(qdir, f) for f in os.listdir(qdir))[:2]
    got = {}
    for mode in ("host", "device"):
        out = str(tmp_path / f"calls.{mode}")
        rc, stdout, err = _run([os.path.join(BIN, "kmers-call-functions"), kd] + inputs +
                               ["-o", out, "--debug-hits", "--ignore-hypo", "--best-call", mode])
        assert rc == 0, err.decode()[-2000:]
        got[mode] = (stdout, open(out, "rb").read())
    assert got["device"] == got["host"] and got["host"][0].count(b"\n") > 1000


def test_annotate_seqs(data_and_queries, tmp_path):
    _, kd, qdir = data_and_queries
    got = {}
    for mode, opts in MODES.items():
        calls, unc = str(tmp_path / f"calls.{mode}"), str(tmp_path / f"uncalled.{mode}")
        rc, _, err = _run([os.path.join(BIN, "kmers-annotate-seqs"), kd, str(tmp_path / "genus"), qdir, calls, unc] + opts)
        assert rc == 0, err.decode()[-2000:]
        got[mode] = (rc, open(calls, "rb").read(), open(unc, "rb").read(), _error_lines(err))
    for mode in MODES:
        assert got[mode] == got["host"], mode
    assert got["host"][1].count(b"\n") > 100 and got["host"][2].count(b"\n") > 0 and len(got["host"][3]) > 0


def _tree(d):
    out = {}
    for root, _, files in os.walk(d):
        for f in files:
            p = os.path.join(root, f)
            out[os.path.relpath(p, d)] = hashlib.sha256(open(p, "rb").read()).hexdigest()
    return out


def test_build_signatures_recall(data_and_queries, tmp_path):
    info, kd, _ = data_and_queries          # kd: built without the option
    want = _tree(kd)
    reports = [k for k in want if k.startswith("recall.report.d" + os.sep)]
    assert len(reports) == 10 and any(os.path.getsize(os.path.join(kd, r)) > 0 for r in reports)
    for mode in ("host", "device"):
        out = str(tmp_path / f"kd.{mode}")
        rc, _, err = _build(info, out, "--best-call", mode)
        assert rc == 0 and _phases(err)["recall_deferred"] == 0, err.decode()[-2000:]
        assert _tree(out) == want, mode
