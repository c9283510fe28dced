"""CPU tests of the recall pass's batch cut rule (csrc/skm_recallplan.h through recall_plan /
skm_recall_plan, host only): the rule restated here, its edge cases, and the shared header alone
under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = 1 << 29


def py_plan(seq_len, batch_residues=0, first_seq=0, n_seqs=0):
    """The rule restated: a batch is a run of whole sequences whose packed bytes (len + 1 each) do not
    exceed batch_residues; a sequence that alone exceeds it is a batch of its own; the view's base
    is the first sequence's packed start rounded down to 16."""
    lim = min(batch_residues or DEFAULT, 1 << 31)
    lens = [int(v) for v in seq_len]
    stop = first_seq + n_seqs if n_seqs else len(lens)
    pstart = [0]
    for v in lens:
        pstart.append(pstart[-1] + v + 1)
    out, s = [], first_seq
    while s < stop:
        e, size = s + 1, lens[s] + 1
        while e < stop and size + lens[e] + 1 <= lim:
            size += lens[e] + 1
            e += 1
        out.append(dict(first=s, n=e - s, base=pstart[s] & ~15, pstart=pstart[s], end=pstart[e],
                        windows=sum(max(v - 7, 0) for v in lens[s:e])))
        s = e
    return out


def check_cover(plan, seq_len, first, stop):
    """The cuts cover [first, stop) exactly once, in order, and every base is pstart & ~15."""
    pstart = np.concatenate([[0], np.cumsum(np.asarray(seq_len, np.int64) + 1)])
    at = first
    for b in plan:
        assert b["first"] == at and b["n"] >= 1
        assert b["pstart"] == pstart[b["first"]] and b["end"] == pstart[b["first"] + b["n"]]
        assert b["base"] == b["pstart"] & ~15 and b["base"] % 16 == 0 and 0 <= b["pstart"] - b["base"] < 16
        at += b["n"]
    assert at == stop


LENS = [0, 7, 8, 9, 0, 0, 23, 24, 25, 300, 1, 15, 16, 17, 0, 40, 5000, 3, 0]


@pytest.mark.parametrize("batch", [1, 2, 16, 17, 26, 100, 301, 302, 4096, 0, 1 << 40])
def test_rule_against_restatement(skm, batch):
    got = skm.recall_plan(LENS, batch)
    assert got == py_plan(LENS, batch)
    check_cover(got, LENS, 0, len(LENS))
    lim = min(batch or DEFAULT, 1 << 31)
    for b in got:  # within the limit, or one sequence that alone exceeds it; and no batch could take one more
        size = b["end"] - b["pstart"]
        assert size <= lim or b["n"] == 1
        nxt = b["first"] + b["n"]
        if nxt < len(LENS):
            assert size + LENS[nxt] + 1 > lim


def test_batch_residues_one_is_one_sequence_per_batch(skm):
    got = skm.recall_plan(LENS, 1)
    assert [b["n"] for b in got] == [1] * len(LENS)
    assert [b["first"] for b in got] == list(range(len(LENS)))
    assert [b["windows"] for b in got] == [max(v - 7, 0) for v in LENS]


def test_long_sequence_is_its_own_batch(skm):
    got = skm.recall_plan([3, 3, 5000, 3, 3], 100)
    assert [(b["first"], b["n"]) for b in got] == [(0, 2), (2, 1), (3, 2)]
    assert got[1]["end"] - got[1]["pstart"] == 5001


@pytest.mark.parametrize("first,n", [(0, 0), (0, 1), (3, 0), (3, 5), (18, 1), (18, 0), (19, 0), (5, 14)])
def test_ranges(skm, first, n):
    for batch in (1, 40, 0):
        got = skm.recall_plan(LENS, batch, first, n)
        assert got == py_plan(LENS, batch, first, n)
        check_cover(got, LENS, first, first + n if n else len(LENS))
    if first == 19:
        assert got == []


def test_all_sixteen_alignments(skm):
    lens = list(range(0, 40))
    got = skm.recall_plan(lens, 1)
    assert {b["pstart"] - b["base"] for b in got} == set(range(16))


def test_random_vectors(skm):
    rng = np.random.default_rng(7)
    for _ in range(200):
        n = int(rng.integers(0, 60))
        lens = rng.integers(0, 50, size=n).astype(np.uint32)
        batch = int(rng.choice([0, 1, 9, 33, 64, 200, 10_000]))
        first = int(rng.integers(0, n + 1))
        cnt = int(rng.integers(0, n - first + 1))
        assert skm.recall_plan(lens, batch, first, cnt) == py_plan(lens, batch, first, cnt)


def test_refusals_and_empties(skm):
    assert skm.recall_plan([], 0) == []
    assert skm.recall_plan(np.zeros(0, np.uint32), 5) == []
    with pytest.raises(skm.SkmError, match="first_seq"):
        skm.recall_plan([1, 2, 3], 0, 4, 0)
    with pytest.raises(skm.SkmError, match="n_seqs"):
        skm.recall_plan([1, 2, 3], 0, 2, 2)
    n = C.c_uint64(7)
    assert skm.lib().skm_recall_plan(None, 0, 0, 0, 0, None, 0, C.byref(n)) == 0 and n.value == 0
    assert skm.lib().skm_recall_plan(None, 3, 0, 0, 0, None, 0, C.byref(n)) == -1
    lens = np.array([1, 2, 3], np.uint32)
    assert skm.lib().skm_recall_plan(lens.ctypes.data, 3, 0, 0, 0, None, 0, None) == -1
    # a small cap: the count is returned all the same, only the first cap rows are written
    out = np.full((2, 6), 0xEE, np.uint64)
    assert skm.lib().skm_recall_plan(lens.ctypes.data, 3, 1, 0, 0, out.ctypes.data, 1, C.byref(n)) == 0
    assert n.value == 3 and out[0].tolist() == [0, 1, 0, 0, 2, 0] and (out[1] == 0xEE).all()


def test_release_level_names(skm):
    lv = skm.SignatureBuilder._release_level
    assert [lv(False), lv(True), lv(0), lv(1), lv(2), lv("keep_sequences")] == [0, 1, 0, 1, 2, 2]
    for bad in (3, -1, "keep", None):
        with pytest.raises(skm.SkmError, match="release_work"):
            lv(bad)


def test_struct_layouts_and_symbols(skm):
    assert C.sizeof(skm._RecallOpts) == 24 and C.sizeof(skm._RecallStats) == 72
    assert skm._RecallStats.view_ms.offset == 48 and skm._RecallStats.wall_s.offset == 64
    for name in ("skm_build_recall", "skm_build_resident_seqs", "skm_recall_plan"):
        assert hasattr(skm.lib(), name)
    # null handles are refused before anything else is touched
    assert skm.lib().skm_build_resident_seqs(None, None, None) == -1
    assert skm.lib().skm_build_recall(None, None, None, None, None, None, None, None) == -1
    assert b"null" in skm.lib().skm_last_error()


def test_shared_header_against_a_naive_loop_under_sanitizers(tmp_path):
    """tests/native/recallplan_check.cpp: the header alone over random length vectors, the lengths in a
    heap block of exactly n entries; built with the address and undefined-behaviour sanitizers (a
    stand-alone program: it needs no preloading) and run as it is."""
    src = os.path.join(ROOT, "tests", "native", "recallplan_check.cpp")
    exe = str(tmp_path / "recallplan_check_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "signature_kmers_amd", "csrc"), src, "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "cases 4000 " in p.stdout and p.stdout.rstrip().endswith("bad 0"), p.stdout + p.stderr
