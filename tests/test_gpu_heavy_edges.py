"""The integer edges of the path the heaviest k-mers take -- k_ovf_plan, k_ovf_split, k_heavy (the
bucketed sample order and the Boyer-Moore + radix-sort path), k_overflow with group_block, and the
giant-chain hand-off -- on planted sub-buckets (planted_heavy.py; test_planted_heavy_cpu.py proves
the inputs and the model without a GPU and prints which scenario holds which edge).

Every build is compared bit for bit with the CPU oracle, scenario by scenario (one scenario is one
overflow sub-bucket), then against the hand-written kept / cut, best-function, avg_from_end and mean
expectations and against the counters the model of the kernels' decisions predicts for the option
set.  The oracle runs once per build; the option sets share it."""
import numpy as np
import pytest

import oracle_ref
import planted_heavy as ph
from planted import HV_FT, assert_scenarios

pytestmark = pytest.mark.gpu

_ref = {}


def reference(name, nf=None):
    """(scenarios, input arrays, sequences, n_functions, oracle result), computed once per build."""
    if (name, nf) not in _ref:
        scs, arrays, nt = ph.BUILDS[name][0]()
        nf_ = scs[0].nf if nf is None else nf
        _ref[(name, nf)] = (scs, arrays, nt, nf_, oracle_ref.build(*arrays, nf_))
    return _ref[(name, nf)]


def run_and_check(skm, name, opts, nf=None, short=0):
    """short: the work buffers are that many elements short of the plan's demand (the step is redone)."""
    scs, arrays, nt, nf, ref = reference(name, nf)
    want = ph.counters_of(scs, nt, nf, opts)
    want["redone"] = 1 if short else 0
    b = skm.SignatureBuilder(nf)
    # exactly what k_ovf_plan must ask for: one element less and the step is redone
    b.set_option("work_buffer_elements", want["demand_overflow_scratch"] - short)
    for k, v in opts.items():
        b.set_option(k, v)
    b.add_batch(*arrays)
    got = b.finish()
    c = b.counters()
    b.close()
    # the oracle, scenario by scenario, and the kept / cut expectations
    assert_scenarios(got.keys, got.data, ref, scs)
    np.testing.assert_array_equal(got.keys, ref["keys"])
    np.testing.assert_array_equal(got.distinct_functions, ref["distinct_functions"])
    np.testing.assert_array_equal(got.seqs_with_func, ref["seqs_with_func"])
    assert got.n_seqs_with_signature == ref["n_seqs_with_signature"]
    # the hand-written records
    rows = dict(zip((int(k) for k in got.keys), got.data))
    for sc in scs:
        for field, hand in (("function_index", sc.best), ("avg_from_end", sc.avg), ("mean", sc.mean)):
            for kmer, v in hand.items():
                assert rows[int.from_bytes(kmer, "little")][field] == v, (sc.name, field, kmer, v)
    # the counters: which kernel took what
    have = {f: c[f] for f in want}
    assert have == want, (name, opts)
    assert c["passes"] == opts.get("key_range_passes", 1)
    return c


@pytest.mark.parametrize("optset", list(ph.MAIN_OPTS))
def test_split_and_heavy(skm, gpu, optset):
    """The split's entry sizes, key table and SPLIT_MAXH; k_heavy's buckets, classes, median bins,
    length sum, best function and radix rounds; giant chains at 2^giant_class."""
    run_and_check(skm, "main", ph.MAIN_OPTS[optset])


def test_heavy_beyond_the_function_table(skm, gpu):
    """The same build with n_functions = HV_FT + 1: every heavy key takes Boyer-Moore and the sort."""
    run_and_check(skm, "main", {}, nf=HV_FT + 1)


@pytest.mark.parametrize("optset", list(ph.PASS4_OPTS))
def test_four_passes(skm, gpu, optset):
    run_and_check(skm, "main_passes4", ph.PASS4_OPTS[optset])


@pytest.mark.parametrize("optset", list(ph.OVF_OPTS))
def test_overflow_unsplit(skm, gpu, optset):
    """k_overflow's network sizes and padding chunks, group-size classes, group_block's run heads,
    chain lengths and inline chains; under the default options the 16,400-member keys of 4,200
    functions are k_heavy's Boyer-Moore path and giant chains."""
    run_and_check(skm, "overflow", ph.OVF_OPTS[optset])


@pytest.mark.parametrize("optset", list(ph.WIDE_OPTS))
def test_three_radix_rounds(skm, gpu, optset):
    run_and_check(skm, "wide", ph.WIDE_OPTS[optset])


@pytest.mark.parametrize("optset", list(ph.PLAN_OPTS))
def test_plan_of_many_entries(skm, gpu, optset):
    """More than 1024 entries on both sides of split_min, of a power of two and of
    overflow_heavy_min; the scratch demand is the model's to the element."""
    run_and_check(skm, "plan", ph.PLAN_OPTS[optset])


def test_plan_one_element_short(skm, gpu):
    run_and_check(skm, "plan", ph.PLAN_OPTS["split_min_mid"], short=1)
