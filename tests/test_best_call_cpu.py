"""The batched best call on the host (skm_fidx_create with device < 0, skm_best_calls_host,
skm_best_call_name): the id-based core of csrc/skm_bestcall.h against the two string forms of
find_best_call (call_functions.tcc:347-659) -- skm_find_best_call and the oracle -- per sequence,
field for field, floats as bits, names as bytes.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bestcall_cases as bc
from conftest import ROOT


@pytest.fixture(scope="module")
def host_results(skm):
    """name -> (BestCalls, names), each batch through skm_best_calls_host once."""
    cache = {}

    def get(name):
        if name not in cache:
            funcs, off, calls = bc.batch(name)
            tb = skm.FunctionIndexTables(funcs, device=-1)
            r = skm.best_calls_host(off, calls, tb, n_threads=8)
            cache[name] = (r, r.names())
        return cache[name]
    return get


@pytest.mark.parametrize("which", ["skm", "oracle"])
@pytest.mark.parametrize("name", bc.SMALL)
def test_restated_and_planted_cases(host_results, name, which):
    """test_host_cpu.py's KATs and random cases as batches, the planted merge / fusion / tie /
    pair_offset / name-order cases: equal to find_best_call, nothing deferred."""
    r, names = host_results(name)
    assert r.n_seqs == len(bc.batch(name)[1]) - 1 and r.n_deferred == 0
    bc.assert_equal_to_reference(r.best, names, bc.reference(name, which), (name, which))


def test_planted_cases_take_the_paths_they_are_named_for(skm, host_results):
    """The planted cases are not vacuous: the boundary fusion is refused, its neighbour accepted,
    pair_offset 2 gives no call and 3 gives the pair, and the name order decides f1."""
    i = {f: k for k, f in enumerate(bc.FUNCS)}
    f1, f3, f5, f13 = (i["function 00001"], i["function 00003"], i["function 00005"],
                       i["function 00001 / function 00003"])
    tb = skm.FunctionIndexTables(bc.FUNCS, device=-1)

    def one(rows):
        off, c = bc.to_batch([rows])
        r = skm.best_calls_host(off, c, tb, n_threads=1)
        return r.best[0], r.names()[0]
    b, n = one([(f1, 6, 400), (f13, 9, 1000), (f3, 6, 500)])           # frac_dif = 0.1f, not < 0.1
    assert b["fi"] != f13 or b["offset"] != 0.0
    b, n = one([(f1, 6, 400), (f13, 9, 1000), (f3, 6, 501)])
    assert b["fi"] == f13 and b["score"] == 21.0 and b["offset"] == 0.0 and n == bc.FUNCS[f13]
    b, n = one([(f13, 6, 500), (f1, 6, 200), (f13, 9, 500), (f3, 6, 300), (f13, 3, 500)])   # W A W B W
    assert b["fi"] == f13 and b["score"] == 30.0
    b, n = one([(f1, 9, 300), (f3, 8, 300), (f5, 6, 300)])
    assert b["flags"] == 0 and b["fi"] == 0xFFFF and n == "" and b["score"] == 0.0 and b["offset"] == 1.0
    b, n = one([(f1, 9, 300), (f3, 8, 300), (f5, 5, 300)])
    assert b["flags"] == skm.BEST_PAIR and n == "function 00003 ?? function 00001" and b["offset"] == 3.0
    assert (b["fi_a"], b["fi_b"]) == (f3, f1)
    b, n = one([(f1, 5, 300), (f3, 4, 300), (f1, 5, 300), (f3, 4, 300), (f1, 1, 300)])   # both F2 absorbed
    assert b["fi"] == f1 and b["score"] == 11.0 and b["offset"] == 11.0
    tr = skm.FunctionIndexTables(bc.FUNCS_REV, device=-1)
    off, c = bc.to_batch([[(0, 6, 300), (2, 5, 300)], [(2, 6, 300), (0, 5, 300)]])
    r = skm.best_calls_host(off, c, tr)
    assert r.names() == ["zeta ?? alpha", "zeta ?? alpha"] and list(r.best["fi_a"]) == [0, 0]


@pytest.mark.parametrize("name", bc.FUZZ)
def test_fuzz_equals_find_best_call(host_results, name):
    """200,000+ sequences of 0-12 calls over FUNCS, FUNCS_SPLIT and the larger index (duplicated
    names, names that are other names' parts, 8-part names, indices past the table and 0xFFFF,
    counts 1-24, medians up to 2^25): equal to both string forms, and -- every sequence within 64
    calls and 8 parts -- nothing deferred."""
    r, names = host_results(name)
    assert r.n_deferred == 0
    for which in ("skm", "oracle"):
        bc.assert_equal_to_reference(r.best, names, bc.reference(name, which), (name, which))
    # the fuzz reaches every outcome
    b = r.best
    assert (b["flags"] & 1).sum() > 1000 and ((b["fi"] != 0xFFFF) & (b["offset"] == 0)).sum() > 100


def test_fuzz_is_large_enough():
    assert sum(len(bc.batch(n)[1]) - 1 for n in bc.FUZZ) >= 200000
    assert 200 <= len(bc.FUNCS_BIG) <= 999 and len(set(bc.FUNCS_BIG)) < len(bc.FUNCS_BIG)
    assert any(len(f.split(" / ")) == 8 for f in bc.FUNCS_BIG)


def test_thread_count_does_not_change_the_result(skm):
    funcs, off, calls = bc.batch("fuzz_funcs")
    tb = skm.FunctionIndexTables(funcs, device=-1)
    a = skm.best_calls_host(off, calls, tb, n_threads=1)
    b = skm.best_calls_host(off, calls, tb, n_threads=16)
    assert a.best.tobytes() == b.best.tobytes() and a.n_calls == b.n_calls == len(calls)


def test_deferred_sequences_are_counted_and_still_right(skm, host_results):
    """More than 64 calls, or a name of more than 8 parts: deferred (and only those), resolved by
    skm_find_best_call -- the results still equal it, the "f1 ?? f2" pair included."""
    r, names = host_results("defer")
    funcs, seqs, expect = bc.defer_seqs()
    assert r.n_deferred == int(expect.sum()) > 0
    for which in ("skm", "oracle"):
        bc.assert_equal_to_reference(r.best, names, bc.reference("defer", which), ("defer", which))
    assert names[0] == "bb ?? aa" and r.best["flags"][0] == skm.BEST_PAIR
    assert (r.best["fi_a"][0], r.best["fi_b"][0]) == (1, 0)
    assert names[7] == funcs[4]      # the 8-part fusion is decided by the core itself


def test_empty_batch_and_argument_errors(skm):
    tb = skm.FunctionIndexTables(bc.FUNCS, device=-1)
    r = skm.best_calls_host(np.zeros(1, np.uint64), np.zeros(0, skm.CALL_DTYPE), tb)
    assert r.n_seqs == 0 and len(r.best) == 0 and r.n_deferred == 0
    lib = skm.lib()
    out = skm._BestCalls()
    assert lib.skm_best_calls_host(None, tb._h, 1, C.byref(out)) == -1
    h = C.c_void_p()
    assert lib.skm_fidx_create(C.byref(h), None, 3, -1) == -1
    assert lib.skm_best_call_name(None, None, None, 0) == -1
    with pytest.raises(skm.SkmError):    # offsets that do not span the calls
        skm.best_calls_host(np.array([0, 5], np.uint64), np.zeros(3, skm.CALL_DTYPE), tb)
    # a NULL name is the name "", as fname() has it
    arr = (C.c_char_p * 2)(b"x", None)
    assert lib.skm_fidx_create(C.byref(h), arr, 2, -1) == 0
    lib.skm_fidx_destroy(h)
    assert skm.BEST_DTYPE.itemsize == 16


def test_name_is_truncated_to_the_buffer(skm):
    tb = skm.FunctionIndexTables(bc.FUNCS, device=-1)
    rec = np.zeros(1, skm.BEST_DTYPE)
    rec["fi"] = 1
    buf = C.create_string_buffer(8)
    n = skm.lib().skm_best_call_name(tb._h, rec.ctypes.data, buf, 8)
    assert n == len(bc.FUNCS[1]) and buf.value == bc.FUNCS[1].encode()[:7]


def test_top_two_selection_matches_std_partial_sort(tmp_path):
    """tests/native/bestcall_check.cpp: BestTop against std::partial_sort itself on 10^6 tie-heavy
    vectors of 1-12 entries; built a second time with the address and undefined-behaviour
    sanitizers (a stand-alone program: it needs no preloading) and run as it is."""
    src = os.path.join(ROOT, "tests", "native", "bestcall_check.cpp")
    inc = ["-I", os.path.join(ROOT, "signature_kmers_amd", "csrc")]
    exe = str(tmp_path / "bestcall_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *inc, src, "-o", exe])
    p = subprocess.run([exe, "1000000"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "vectors 1000000 bad 0" in p.stdout, p.stdout + p.stderr
    san = str(tmp_path / "bestcall_check_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", *inc, src, "-o", san])
    p = subprocess.run([san, "200000"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "vectors 200000 bad 0" in p.stdout, p.stdout + p.stderr
