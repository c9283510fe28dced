"""Host-only parts of the device-built exact DB (skm_build_kept_db): the table plan and the slot
function of its range-reduced table, against a Python restatement.  No GPU work is issued."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "skm.h")
NEW = ("skm_build_kept_db", "skm_kept_db_plan", "skm_debug_kept_slot", "skm_db_lookup_fm", "skm_db_table_info")
M64 = (1 << 64) - 1


def declared_functions():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"^\s*(?:const\s+)?[A-Za-z_][\w\s\*]*?\b(skm_\w+)\s*\(", txt, flags=re.M))


def fmix64(k: int) -> int:
    """MurmurHash3's 64-bit finaliser."""
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & M64
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & M64
    k ^= k >> 33
    return k


def py_slot(key: int, T: int) -> int:
    return (fmix64(key) * T) >> 64


def test_plan_sizes(skm):
    # slots = max(16, ceil(100 n / load_pct)); at load 60 %:
    for n in (0, 1, 9):
        assert skm.kept_db_plan(n, load_pct=60) == (16, 256)
    # n = 10: ceil(1000 / 60) = 17 by the formula the header states (16 slots for 10 keys would be
    # load 62.5 %, above the 60 asked for)
    assert skm.kept_db_plan(10, load_pct=60) == (17, 272)
    # the default load is 40 % (chosen from the measured recall times, profiles/kept_db_ab.json)
    assert [skm.kept_db_plan(n)[0] for n in (0, 1, 6, 7, 9, 10)] == [16, 16, 16, 18, 23, 25]
    assert skm.kept_db_plan(12345) == skm.kept_db_plan(12345, load_pct=40) == (30863, 16 * 30863)
    assert skm.kept_db_plan(1000, load_pct=50) == (2000, 32000)
    assert skm.kept_db_plan(1000, slots=1001) == (1001, 16016)


def test_plan_headline_size(skm):
    slots, nbytes = skm.kept_db_plan(2_890_000_000, load_pct=60)
    assert slots == 4_816_666_667 and nbytes == 77_066_666_672
    assert slots > 2**32 and nbytes < 137_438_953_472  # the power-of-two table of the host path
    slots, nbytes = skm.kept_db_plan(2_890_000_000)    # the default, load 40 %
    assert slots == 7_225_000_000 and nbytes == 115_600_000_000
    assert slots > 2**32 and nbytes < 137_438_953_472


@pytest.mark.parametrize("kw", [dict(n=1000, slots=1000), dict(n=1000, slots=999), dict(n=5, load_pct=9),
                                dict(n=5, load_pct=96), dict(n=2**32 - 1)])
def test_plan_refusals(skm, kw):
    with pytest.raises(skm.SkmError, match="error -1"):
        skm.kept_db_plan(**kw)


@pytest.mark.parametrize("T", [16, 17, 1000, 2**32 - 1, 2**32, 2**32 + 12345, 4_816_666_667])
def test_slot_function_matches_restatement(skm, T):
    import ctypes as C
    rng = np.random.default_rng(T % 1000003)
    keys = rng.integers(1, 2**64 - 1, size=100_000, dtype=np.uint64)
    fn = skm.lib().skm_debug_kept_slot
    v = C.c_uint64()
    got = np.empty(len(keys), np.uint64)
    for i, k in enumerate(keys.tolist()):
        assert fn(k, T, C.byref(v)) == 0
        got[i] = v.value
    want = np.array([py_slot(k, T) for k in keys.tolist()], np.uint64)
    np.testing.assert_array_equal(got, want)
    assert int(got.max()) < T
    if T > 1000:  # the reduction spreads over the whole table
        assert int(got.max()) > T - T // 1000 and int(got.min()) < T // 1000


def test_slot_function_edges(skm):
    assert skm.kept_slot(0, 1009) == 0            # fmix64(0) == 0
    for T in (1, 16, 2**32 + 12345):
        assert skm.kept_slot(M64, T) == py_slot(M64, T) < T
    with pytest.raises(skm.SkmError):
        skm.kept_slot(5, 0)


def test_header_declares_and_library_exports_the_new_names(skm):
    names = declared_functions()
    for n in NEW:
        assert n in names, n
        assert n in skm._SIGS, n
    txt = open(HEADER).read()
    assert re.search(r"typedef struct skm_kept_db_opts \{[^}]*load_pct[^}]*release_work[^}]*slots[^}]*\}", txt, re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", skm.lib()._name], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT\s+(\w+)$", out, flags=re.M))
    assert set(NEW) <= exported
