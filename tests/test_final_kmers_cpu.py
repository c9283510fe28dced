"""The final.kmers line formatter on the CPU (csrc/skm_finalkmers.h through
skm_debug_final_kmers_host): the function the device kernels k_fk_len / k_fk_emit run, against the
line of kmers-build-signatures.cc:212-216 restated with numpy and str."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WIDTHS = (0, 9, 10, 99, 100, 999, 1000, 9999, 10000, 65535)


def expected(keys, data) -> bytes:
    """KMER \\t avg_from_end \\t function_index \\t \\n: key bytes via .view(np.uint8), decimals via str."""
    kb = np.ascontiguousarray(keys, dtype="<u8").view(np.uint8).reshape(-1, 8)
    return b"".join(kb[i].tobytes() + b"\t" + str(int(data["avg_from_end"][i])).encode() + b"\t" +
                    str(int(data["function_index"][i])).encode() + b"\t\n" for i in range(len(keys)))


def records(skm, avg, fi, seed=3):
    d = np.zeros(len(avg), skm.STORED_DTYPE)
    d["avg_from_end"], d["function_index"] = avg, fi
    rng = np.random.default_rng(seed)
    for f in ("mean", "median", "var"):  # never printed
        d[f] = rng.integers(0, 65536, len(avg))
    return d


def test_every_pair_of_digit_widths(skm):
    pairs = list(itertools.product(WIDTHS, WIDTHS))
    assert len(pairs) == 100
    d = records(skm, [a for a, _ in pairs], [f for _, f in pairs])
    keys = np.frombuffer(b"".join(b"ACDEFGH" + bytes([65 + i % 26]) for i in range(100)), "<u8")
    got = skm.final_kmers_host(keys, d)
    want = expected(keys, d)
    assert got == want
    lines = got.split(b"\n")[:-1]
    assert len(lines) == 100 and {len(x) + 1 for x in lines} == set(range(14, 23))
    assert got.startswith(b"ACDEFGHA\t0\t0\t\nACDEFGHB\t0\t9\t\n")
    assert got.endswith(b"\t65535\t65535\t\n")


def test_key_bytes_are_copied_not_validated(skm):
    raw = [b"acdefghi", b"MKVLaagi", b"ACDEFG\x80\xff", b"\x01\t\n\x00ABCD", b"XXXXXXXX", b"\xff" * 8]
    keys = np.frombuffer(b"".join(raw), "<u8")
    d = records(skm, [1, 22, 333, 4444, 55555, 7], [7, 55555, 4444, 333, 22, 1])
    got = skm.final_kmers_host(keys, d)
    assert got == expected(keys, d)
    at = 0
    for k, a, f in zip(raw, d["avg_from_end"], d["function_index"]):
        line = k + b"\t%d\t%d\t\n" % (a, f)
        assert got[at:at + len(line)] == line
        at += len(line)
    assert at == len(got)


def test_length_only_call_and_short_buffers(skm):
    pairs = list(itertools.product(WIDTHS, WIDTHS))
    d = records(skm, [a for a, _ in pairs], [f for _, f in pairs])
    keys = np.arange(100, dtype=np.uint64) + np.uint64(0x4141414141414141)
    want = expected(keys, d)
    n = C.c_uint64(0)
    fn = skm.lib().skm_debug_final_kmers_host
    assert fn(keys.ctypes.data, d.ctypes.data, 100, None, 0, C.byref(n)) == 0
    assert n.value == len(want) == sum(12 + len(str(a)) + len(str(f)) for a, f in pairs)
    # a buffer that is too small: the total is returned all the same, whole lines only are written
    cap = 14 + 14 + 7
    buf = np.full(cap + 8, 0xEE, np.uint8)
    n.value = 0
    assert fn(keys.ctypes.data, d.ctypes.data, 100, buf.ctypes.data, cap, C.byref(n)) == 0
    assert n.value == len(want)
    assert buf[:28].tobytes() == want[:28] and (buf[28:] == 0xEE).all()
    # nothing in, nothing out
    assert fn(None, None, 0, None, 0, C.byref(n)) == 0 and n.value == 0
    assert skm.final_kmers_host(np.zeros(0, np.uint64), np.zeros(0, skm.STORED_DTYPE)) == b""
    assert fn(keys.ctypes.data, d.ctypes.data, 100, None, 0, None) == -1


def test_formatter_against_snprintf_under_sanitizers(tmp_path):
    """tests/native/finalkmers_check.cpp: the header alone, every u16 in each column against snprintf,
    each line in a heap block of exactly its announced length; built with the address and
    undefined-behaviour sanitizers (a stand-alone program: it needs no preloading) and run as it is."""
    src = os.path.join(ROOT, "tests", "native", "finalkmers_check.cpp")
    exe = str(tmp_path / "finalkmers_check_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "signature_kmers_amd", "csrc"), src, "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "lines 131172 " in p.stdout and p.stdout.rstrip().endswith("bad 0"), p.stdout + p.stderr


def test_geometry_without_a_device(skm):
    lines, threads, longest, reserved = skm.final_kmers_info()
    assert lines > 0 and threads > 0 and lines % threads == 0
    assert longest == 22 and reserved == 0
    assert skm.lib().skm_final_kmers_info(None) == -1
