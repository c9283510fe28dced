"""Host-only parts of the BDZ DB built on the device from a finished build (skm_build_mph_db): the
plan against a Python restatement of the geometry, and the new names in the header, the bindings
and the library.  No GPU work is issued."""
import math
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "skm.h")
NEW = ("skm_build_mph_db", "skm_mph_db_plan")
SIZES = (0, 1, 2, 1023, 1024, 168_700_000, 2_889_174_825)


def first_r(n: int) -> int:
    """r of the first attempt: ceil(1.23 n / 3) made odd (perfect_hash.h:29-33 through cmph's bdz_new)."""
    r = math.ceil((1.23 * n) / 3)
    return r + 1 if r % 2 == 0 else r


@pytest.mark.parametrize("n", SIZES)
def test_plan_geometry_and_bounds(skm, n):
    r, nv, db_bytes, peak = skm.mph_db_plan(n)
    assert (r, nv) == (first_r(n), 3 * first_r(n))
    assert r % 2 == 1 and nv < 2**32 - 2**12
    # the open DB holds at least the records (10 B), the record words (4 B) and g (2 bits a vertex)
    assert peak >= db_bytes >= 14 * n + math.ceil(3 * r / 4)


def test_plan_sizes_spelled_out(skm):
    # g padded to a 64-byte multiple plus a line, the rank table, records, record words, pair lines
    def db_bytes(n):
        nv = 3 * first_r(n)
        g = -(-(-(-nv // 4)) // 64) * 64 + 64
        return g + 4 * max(-(-nv // 128), 1) + max(10 * n, 16) + 4 * max(n, 1) + 64 * (nv // 128 + 2)
    for n in SIZES + (1025, 1300, 4099, 411_363):
        assert skm.mph_db_plan(n)[2] == db_bytes(n), n
    # from 1024 keys on the peel state is the peak: 16 bytes per vertex, 5 per key, the counters
    for n in (1024, 4099, 168_700_000, 2_889_174_825):
        assert skm.mph_db_plan(n)[3] == 16 * 3 * first_r(n) + 5 * n + 64, n
    # the headline kept set: about 71 GB of peel state, a 43 GB DB
    _, _, db, peak = skm.mph_db_plan(2_889_174_825)
    assert 43.0e9 < db < 43.5e9 and 71.0e9 < peak < 71.5e9


def test_plan_refuses_more_keys_than_one_bdz_holds(skm):
    assert skm.mph_db_plan(3_400_000_000)[1] < 2**32 - 2**12
    with pytest.raises(skm.SkmError, match="error -1"):
        skm.mph_db_plan(3_400_000_001)


def test_header_declares_and_library_exports_the_new_names(skm):
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = set(re.findall(r"^\s*(?:const\s+)?[A-Za-z_][\w\s\*]*?\b(skm_\w+)\s*\(", txt, flags=re.M))
    for n in NEW:
        assert n in names, n
        assert n in skm._SIGS, n
    assert re.search(r"typedef struct skm_mph_db_opts \{[^}]*seed[^}]*release_work[^}]*verify[^}]*pad[^}]*"
                     r"mph_path[^}]*dat_path[^}]*\}", txt, re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", skm.lib()._name], capture_output=True, text=True).stdout
    assert set(NEW) <= set(re.findall(r"\bT\s+(\w+)$", out, flags=re.M))
    assert hasattr(skm.SignatureBuilder, "mph_db")
    import ctypes as C
    assert C.sizeof(skm._MphDbOpts) == 32 and skm._MphDbOpts.mph_path.offset == 16
