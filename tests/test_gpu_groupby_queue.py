"""k_bucket_process as a persistent kernel over (bucket, part) tasks: part c of a bucket is the
sub-buckets [c nsub / 8, (c + 1) nsub / 8) of k_partition's table, a batch never crosses a part
boundary, and a bucket that fits LDS is its part 0 (read from k_partition's copy of it in tmp).

Planted buckets (planted.py, planted_queue.py; test_planted_queue_cpu.py proves the new ones land
where they claim):
Build B of planted_scenarios.py has nsub = 8 (one sub-bucket per part: the pairs of 1000 + 1048 =
CAP and 1000 + 1049 = CAP + 1 that the one-workgroup walk merged or not now sit across a part
boundary, an overflow sub-bucket is a whole part, empty parts) and nsub = 4 (below the part count:
parts 1, 3, 5 and 7 hold one sub-bucket each, the others none); Build A has the buckets grouped in
place, one of exactly CAP.  planted_queue.py adds nsub = 16, two sub-buckets per part, and a bucket
of 1200 elements that two ranks split with b2 = 1: nsub = 2, only parts 3 and 7 hold anything.  Every
build is compared bit for bit with the oracle, scenario by scenario, then with the hand-written
kept / cut expectations and the counter sums."""
import numpy as np
import pytest

import oracle_ref
from planted import assert_same, assert_scenarios, counter_sums
from planted_queue import batches_of, build_q, sizes_of, tasks_of
from signature_kmers_amd import synth
from test_gpu_multirank import run_group

pytestmark = pytest.mark.gpu

_ref = {}


def reference(pass_bits):
    if pass_bits not in _ref:
        scs, arrays = build_q(pass_bits)
        _ref[pass_bits] = (scs, arrays, oracle_ref.build(*arrays, scs[0].nf))
    return _ref[pass_bits]


def build(skm, scs, arrays, opts):
    b = skm.SignatureBuilder(scs[0].nf)
    for k, v in opts.items():
        b.set_option(k, v)
    b.add_batch(*arrays)
    got = b.finish()
    c = b.counters()
    b.close()
    return got, c


@pytest.mark.parametrize("pass_bits", [0, 2])
def test_parts(skm, gpu, pass_bits):
    """One pass and four key-range passes.  The batch counter equals the part-restricted walk's
    count worked out from the declared sub-bucket sizes, and the task counter the parts that hold a
    batch: merge_exact makes four batches of 1000, 1048, 2047 and 1, where the whole-bucket walk
    made two of 2048."""
    scs, arrays, ref = reference(pass_bits)
    got, c = build(skm, scs, arrays, {"key_range_passes": 1 << pass_bits})
    assert c["passes"] == 1 << pass_bits
    assert_scenarios(got.keys, got.data, ref, scs)
    assert_same(got, ref)
    want = counter_sums(scs)
    assert {f: c[f] for f in want} == want
    assert scs[0].name == "merge_exact" and batches_of(scs[0]) == 4 and batches_of(scs[0], 1) == 2
    assert c["groupby_batches"] == sum(batches_of(sc) for sc in scs)
    assert c["groupby_tasks"] == sum(tasks_of(sc) for sc in scs)


def test_world_2(skm, gpu):
    """The same input on two in-process ranks, even sequences on rank 0: nsrc = 2, so no bucket is
    grouped in place and the buckets of at most CAP elements are partitioned too: small_nsub2 with
    nsub = 2, the two buckets of exactly CAP with nsub = 4, all below the part count.  The ranks'
    counters add up to the scenarios' sums and to the tasks and batches of the part-restricted walk
    (small_nsub2: two batches in parts 3 and 7).  The oracle gets the sequences in (rank, sequence)
    order, as in test_gpu_groupby_edges.test_world_2."""
    scs, arrays, _ = reference(0)
    r, o, l, f, i = arrays
    n = len(l)
    order = np.concatenate([np.arange(0, n, 2), np.arange(1, n, 2)])
    ref = oracle_ref.build(r, o[order], l[order], f[order], i[order], scs[0].nf)
    ctrs = []
    outs = run_group(skm, arrays, scs[0].nf, 2, lambda rank: np.arange(n) % 2 == rank, counters=ctrs)
    assert_scenarios(outs[0].keys, outs[0].data, ref, scs)
    assert_same(outs[0], ref)
    want = counter_sums(scs)
    assert {f: sum(c[f] for c in ctrs) for f in want} == want
    small = next(sc for sc in scs if sc.name == "small_nsub2")
    assert sizes_of(small) is None and sizes_of(small, True) == (700, 500)
    assert (batches_of(small), batches_of(small, two_ranks=True), tasks_of(small, True)) == (1, 2, 2)
    assert sum(c["groupby_batches"] for c in ctrs) == sum(batches_of(sc, two_ranks=True) for sc in scs)
    assert sum(c["groupby_tasks"] for c in ctrs) == sum(tasks_of(sc, True) for sc in scs)


def test_workgroups_take_many_tasks(skm, gpu):
    """60 K proteins in 4 passes: every pass has 4096 buckets x 8 parts = 32768 tasks for a grid of
    two workgroups per CU.  The counter is the total of the 4 passes, so more than 4 x 2 x 1024
    means that some pass had more tasks with a batch than a device of 1024 CUs has workgroups in
    the grid (MI355X: 256 CUs, 512 workgroups): in that pass at least one workgroup grouped two
    tasks, reloading its slice of a sub table over the last one; most of the tasks it popped in
    between were empty parts."""
    p = synth.generate_arrays(60000, 60, per_file=2000, seed=6)
    r, o, l, f, i, funcs = synth.build_inputs(p)
    ref = oracle_ref.build(r, o, l, f, i, len(funcs))
    b = skm.SignatureBuilder(len(funcs))
    b.set_option("key_range_passes", 4)
    b.add_batch(r, o, l, f, i)
    got = b.finish()
    c = b.counters()
    b.close()
    assert c["groupby_tasks"] > 4 * 2 * 1024, c["groupby_tasks"]
    assert c["groupby_batches"] >= c["groupby_tasks"]
    np.testing.assert_array_equal(got.keys, ref["keys"])
    np.testing.assert_array_equal(got.data.view(np.uint8), ref["data"].view(np.uint8))
