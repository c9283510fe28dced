"""The device FASTA parser's boundary on the CPU: the entry points exist and are declared, the
chunk geometry is sane, argument errors are reported before any device is touched, and both CLIs
know --fasta-parse."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fasta_device_util as fu
from conftest import ROOT

BIN = os.path.join(ROOT, "bin")
ENTRY_POINTS = ("skm_fasta_parse_device", "skm_query_create_fasta", "skm_annotate_fasta", "skm_fasta_table_free",
                "skm_fasta_parse_info")
E_ARG = -1


def test_entry_points_exported_and_declared(skm):
    lib = skm.lib()
    header = open(os.path.join(ROOT, "include", "skm.h")).read()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in skm._SIGS
    assert "typedef struct skm_fasta_table" in header


def test_parse_info_geometry(skm):
    thread, wave, tile = skm.fasta_parse_info()
    for v in (thread, wave, tile):
        assert v > 0 and v & (v - 1) == 0
    assert thread <= wave <= tile


def test_rules_text_records_are_the_restatements():
    assert fu.expected(fu.RULES_TEXT) == fu.RULES_RECORDS


def _parse(skm, data, off, n_files, out=True):
    t = skm._FastaTable()
    rc = skm.lib().skm_fasta_parse_device(None if data is None else skm._ptr(data), None if off is None else skm._ptr(off),
                                          n_files, 0, 0, C.byref(t) if out else None)
    return rc, skm.lib().skm_last_error()


@pytest.mark.parametrize("case", ["null_bytes", "null_file_off", "first_not_zero", "descending", "null_out"])
def test_argument_errors_without_a_device(skm, case):
    data = np.frombuffer(b">a\nACDEFGHIK\n", dtype=np.uint8)
    off = np.array([0, 4, len(data)], np.uint64)
    if case == "null_bytes":
        rc, msg = _parse(skm, None, off, 2)
    elif case == "null_file_off":
        rc, msg = _parse(skm, data, None, 2)
    elif case == "first_not_zero":
        rc, msg = _parse(skm, data, np.array([1, 4, len(data)], np.uint64), 2)
    elif case == "descending":
        rc, msg = _parse(skm, data, np.array([0, 9, 4], np.uint64), 2)
    else:
        rc, msg = _parse(skm, data, off, 2, out=False)
    assert rc == E_ARG and len(msg) > 0


def test_query_and_annotate_argument_errors(skm):
    lib = skm.lib()
    data = np.frombuffer(b">a\nACDEFGHIK\n", dtype=np.uint8)
    off = np.array([0, len(data)], np.uint64)
    h = C.c_void_p()
    assert lib.skm_query_create_fasta(C.byref(h), None, skm._ptr(data), skm._ptr(off), 1, None) == E_ARG
    assert lib.skm_query_create_fasta(None, None, skm._ptr(data), skm._ptr(off), 1, None) == E_ARG
    opts, calls = skm._AnnotOpts(5, 200, 0, 0, 0, 0), skm._Calls()
    assert lib.skm_annotate_fasta(None, skm._ptr(data), skm._ptr(off), 1, C.byref(opts), C.byref(calls), None) == E_ARG
    assert len(lib.skm_last_error()) > 0


@pytest.mark.parametrize("tool", ["kmers-call-functions", "kmers-annotate-seqs"])
def test_cli_knows_fasta_parse(skm, tool, tmp_path):
    exe = os.path.join(BIN, tool)
    p = subprocess.run([exe, "--help"], capture_output=True, timeout=60)
    assert p.returncode == 0 and b"--fasta-parse" in p.stdout
    # a bad value is refused while the options are read: no data directory, no device needed
    args = [str(tmp_path / "kd"), str(tmp_path / "in.fa")] if tool == "kmers-call-functions" else \
        [str(tmp_path / "kd"), str(tmp_path / "genus"), str(tmp_path / "seqs"), str(tmp_path / "c"), str(tmp_path / "u")]
    p = subprocess.run([exe, "--fasta-parse", "bogus"] + args, capture_output=True, timeout=60)
    assert p.returncode == 1 and b"--fasta-parse must be host or device" in p.stderr
