"""The edges of the deferred statistics scheduler -- the class sort (k_job_count / k_job_scan /
k_job_scatter), the per-lane chains (k_chains), the run arena of key-range passes (k_long_plan /
k_long_stash / k_long_snap), the lane | wave-pair split of a batch (flush_long_chains) and the giant
chains (k_giant_order / k_chain_dyn) -- on planted chains (planted_chains.py;
test_planted_chains_cpu.py proves the inputs and the model without a GPU and prints which build
holds which edge).

Every run is compared bit for bit with the CPU oracle, then with pyref's recurrences over the
samples of every planted chain (each has a nonzero median and variance of its own within its pass,
so a chain that was skipped or ran on a neighbour's samples shows), then with the counters the
model predicts for the option set.  The oracle runs once per build; the option sets share it."""
import numpy as np
import pytest

import oracle_ref
import planted_chains as pc
from planted import assert_same
from test_gpu_multirank import run_group

pytestmark = pytest.mark.gpu

_ref = {}
COUNTERS = ("chain_jobs", "chain_samples", "long_samples", "demand_long_samples", "demand_long_jobs", "giant_chains",
            "giant_max", "redone", "passes")


def reference(name):
    """(build, recount, pyref expectations, oracle result), computed once per build."""
    if name not in _ref:
        b = pc.BUILDS[name][0]()
        F = pc.facts(b.arrays, b.pass_bits)
        _ref[name] = (b, F, pc.expected(F), oracle_ref.build(*b.arrays, pc.NF))
    return _ref[name]


def check_result(got, F, exp, ref):
    assert_same(got, ref)
    at = np.searchsorted(got.keys, F.keys)
    idx = np.fromiter(exp, np.int64, len(exp))
    want = np.array([exp[int(k)] for k in idx], np.int64).reshape(-1, 2)
    rows = got.data[at[idx]]
    bad = np.nonzero((rows["median"] != want[:, 0]) | (rows["var"] != want[:, 1]))[0]
    assert len(bad) == 0, (len(bad), [(int(F.cb[idx[j]]), int(F.pas[idx[j]]), F.source[idx[j]], rows[j], want[j])
                                      for j in bad[:5]])


def configure(b, opts, work):
    b.set_option("work_buffer_elements", work)
    for k, v in opts.items():
        b.set_option(k, v)


def run_and_check(skm, name, opts, short=0):
    """short: the work buffers are that many elements short of the arena's demand (the step is redone)."""
    b_, F, exp, ref = reference(name)
    m = pc.model(F, opts)
    want = dict(m["counters"], redone=1 if short else 0)
    b = skm.SignatureBuilder(pc.NF)
    configure(b, opts, pc.work_buffer(m) - short)
    b.add_batch(*b_.arrays)
    got = b.finish()
    c = b.counters()
    b.close()
    check_result(got, F, exp, ref)
    assert {f: c[f] for f in COUNTERS} == want, (name, opts)
    return c


@pytest.mark.parametrize("optset", list(pc.MAIN_OPTS))
def test_sixteen_passes(skm, gpu, optset):
    """Job counts 0 | 1 | 255 | 256 | 257 | 513 and long-job counts 0 | 1 | 1023 | 1024 | 1025 | 2049
    a pass, the four sample sources, both chain sets stashing in one pass, chains at the class and
    lane thresholds in an early and in the tail batch; the option sets move the thresholds, the
    batches, the streams and the grids."""
    run_and_check(skm, "main", pc.MAIN_OPTS[optset])


@pytest.mark.parametrize("optset", list(pc.BUILDS["arena"][1]))
def test_arena_filled_to_the_last_element(skm, gpu, optset):
    c = run_and_check(skm, "arena", pc.BUILDS["arena"][1][optset])
    assert c["cap_long_samples"] == c["long_samples"]


def test_arena_one_element_short(skm, gpu):
    """The reservation of the last pass does not fit: the library's grow-and-retry, with every slot
    of the long-job list poisoned (a batch that named an unwritten slot would fail the run)."""
    c = run_and_check(skm, "arena", pc.ARENA, short=1)
    assert c["cap_long_samples"] > c["long_samples"]


@pytest.mark.parametrize("name", ["passes_64", "passes_2", "giant", "giant_4097"])
def test_other_pass_counts_and_giant_chains(skm, gpu, name):
    for opts in pc.BUILDS[name][1].values():
        run_and_check(skm, name, opts)


def test_second_run_is_identical(skm, gpu):
    b_, F, exp, ref = reference("main")
    opts = pc.MAIN_OPTS["batches_3"]
    m = pc.model(F, opts)
    b = skm.SignatureBuilder(pc.NF)
    configure(b, opts, pc.work_buffer(m))
    b.add_batch(*b_.arrays)
    b.run()
    c1 = b.counters()
    b.run()
    c2 = b.counters()
    got = b.finish()
    b.close()
    assert {f: c1[f] for f in COUNTERS} == {f: c2[f] for f in COUNTERS} == m["counters"]
    check_result(got, F, exp, ref)


def test_world_2(skm, gpu):
    """Even sequences on rank 0 and odd ones on rank 1: a group's visit order is (rank, sequence),
    so the oracle and pyref get the input in that order."""
    b_, F, _, _ = reference("main")
    r, o, l, f, i = b_.arrays
    n = len(l)
    if "main_world2" not in _ref:
        order = np.concatenate([np.arange(0, n, 2), np.arange(1, n, 2)])
        F2 = pc.facts(b_.arrays, b_.pass_bits, order=order, classify=False)
        _ref["main_world2"] = (F2, pc.expected(F2), oracle_ref.build(r, o[order], l[order], f[order], i[order], pc.NF))
    F2, exp2, ref2 = _ref["main_world2"]
    opts = dict(pc.MAIN, work_buffer_elements=pc.work_buffer(pc.model(F, pc.MAIN)))
    ctrs = []
    outs = run_group(skm, b_.arrays, pc.NF, 2, lambda rank: np.arange(n) % 2 == rank, opts=opts, counters=ctrs)
    check_result(outs[0], F2, exp2, ref2)
    assert sum(c["chain_jobs"] for c in ctrs) == pc.model(F, pc.MAIN)["counters"]["chain_jobs"]
