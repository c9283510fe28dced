"""The integer edges of the LDS group-by (k_bucket_process / process_sub / seg_groups<S>), of
k_big_groups' size dispatch, of k_partition's split and of k_heavy's function table, on planted
buckets (planted.py, planted_scenarios.py; test_planted_cpu.py proves the inputs are what they
claim).  Every build is compared bit for bit with the CPU oracle, scenario by scenario -- one
scenario is one level-1 bucket, walked by its own workgroup -- then against the hand-written kept /
cut expectations and the scenarios' counter sums."""
import numpy as np
import pytest

import oracle_ref
import planted_scenarios as ps
from planted import HV_FT, assert_same, assert_scenarios, counter_sums
from test_gpu_multirank import run_group

pytestmark = pytest.mark.gpu

_ref = {}


def reference(name, make):
    """(scenarios, input arrays, oracle result), computed once per build."""
    if name not in _ref:
        scs, arrays = make()
        _ref[name] = (scs, arrays, oracle_ref.build(*arrays, scs[0].nf))
    return _ref[name]


def build(skm, scs, arrays, opts):
    b = skm.SignatureBuilder(scs[0].nf)
    for k, v in opts.items():
        b.set_option(k, v)
    b.add_batch(*arrays)
    got = b.finish()
    c = b.counters()
    b.close()
    return got, c


def check(got, counters, scs, ref):
    assert_scenarios(got.keys, got.data, ref, scs)
    assert_same(got, ref)
    want = counter_sums(scs)
    have = {f: sum(c[f] for c in counters) for f in want}
    assert have == want


@pytest.mark.parametrize("which", ["a", "b"])
def test_one_pass(skm, gpu, which):
    """Build A: every bucket is one batch straight from recs (the direct path).  Build B: bucket
    totals above CAP, so k_partition splits them and next_batch merges the sub-buckets."""
    scs, arrays, ref = reference(which, ps.build_a if which == "a" else ps.build_b)
    got, c = build(skm, scs, arrays, {"key_range_passes": 1})
    assert c["passes"] == 1
    check(got, [c], scs, ref)
    if which == "a":
        assert c["overflow_subbuckets"] == 0


@pytest.mark.parametrize("which", ["a", "b"])
def test_four_passes(skm, gpu, which):
    """The same scenarios planted for 2 pass bits + 12 bucket bits + a 29-bit rem, spread over all
    four passes."""
    make = ps.build_a if which == "a" else ps.build_b
    scs, arrays, ref = reference(which + "_passes4", lambda: make(2))
    assert sorted(set(sc.prefix >> 12 for sc in scs)) == [0, 1, 2, 3]
    got, c = build(skm, scs, arrays, {"key_range_passes": 4})
    assert c["passes"] == 4
    check(got, [c], scs, ref)


def test_world_2(skm, gpu):
    """Build A's input, even sequences on rank 0 and odd ones on rank 1: nsrc = 2, so every bucket
    is partitioned from two segments and k_bucket_process never takes the direct form.  The group's
    sequence order is (rank, sequence) -- rank 0's sequences, then rank 1's -- and the P^2 median and
    the variance of a group depend on the visit order, so the oracle gets the input in that order."""
    scs, arrays, _ = reference("a", ps.build_a)
    n = len(arrays[2])
    if "a_world2" not in _ref:
        r, o, l, f, i = arrays
        order = np.concatenate([np.arange(0, n, 2), np.arange(1, n, 2)])
        _ref["a_world2"] = oracle_ref.build(r, o[order], l[order], f[order], i[order], scs[0].nf)
    ref = _ref["a_world2"]
    ctrs = []
    outs = run_group(skm, arrays, scs[0].nf, 2, lambda rank: np.arange(n) % 2 == rank, counters=ctrs)
    check(outs[0], ctrs, scs, ref)


@pytest.mark.parametrize("nf", [HV_FT, HV_FT + 1])
def test_heavy_function_table(skm, gpu, nf):
    """k_heavy at the last n_functions that takes the LDS function table and the first that takes
    the Boyer-Moore path: a heavy key whose best function is nf - 1 at exactly 80 % (kept), and a
    50 : 50 tie (cut)."""
    scs, arrays, ref = reference(f"heavy_{nf}", lambda: ps.heavy_table(nf))
    got, c = build(skm, scs, arrays, {"key_range_passes": 1})
    check(got, [c], scs, ref)
    sc = scs[0]
    row = got.data[got.keys == np.uint64(int.from_bytes(sc.top80, "little"))]
    assert len(row) == 1 and row["function_index"][0] == nf - 1
