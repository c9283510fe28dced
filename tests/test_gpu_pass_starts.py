"""The per-pass bucket starts, staging cursors, slice table and partition order computed at emission
time (k_pass_starts, one workgroup per pass of an emission group, two buffer sets alternating by
group parity) instead of by six small kernels on the main stream before every pass.

Every build is compared bit for bit with the oracle on the 60 K-protein input that
test_key_range_passes uses (level-2 partition, overflow sub-buckets, chains), must not have been
redone, and is run twice on one handle: the second run re-emits every group, so a copy left by the
first run (the staging consumes the cursor copies) cannot serve it."""
import numpy as np
import pytest

import oracle_ref
from signature_kmers_amd import synth
from test_gpu_build import assert_same
from test_gpu_multirank import check_against_oracle, run_group, shard

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case():
    p = synth.generate_arrays(60000, 60, per_file=2000, seed=6)
    r, o, l, f, i, funcs = synth.build_inputs(p)
    ref = oracle_ref.build(r, o, l, f, i, len(funcs))
    return p, (r, o, l, f, i), len(funcs), ref


def build_twice(skm, arrays, nf, opts):
    b = skm.SignatureBuilder(nf)
    for k, v in opts.items():
        b.set_option(k, v)
    b.set_option("main_long_class", 8)
    b.set_option("overflow_long_class", 8)
    b.add_batch(*arrays)
    b.run()
    c1 = b.counters()
    b.run()
    c2 = b.counters()
    got = b.finish()
    b.close()
    assert c1["redone"] == 0 and c2["redone"] == 0, (c1["redone"], c2["redone"])
    assert c1 == c2
    return got, c1


@pytest.mark.parametrize("passes", [2, 4, 16, 64])
def test_pass_counts(skm, gpu, case, passes):
    """One group only (2, 4), four groups (16) and sixteen (64) at the default group of four passes:
    both buffer sets are reused several times."""
    _, arrays, nf, ref = case
    got, c = build_twice(skm, arrays, nf, {"key_range_passes": passes})
    assert c["passes"] == passes and c["grouped"] == c["valid"], c
    assert_same(got, ref)


@pytest.mark.parametrize("eg", [1, 2, 4, 16])
def test_emit_groups(skm, gpu, case, eg):
    """16 passes emitted 1, 2, 4 and 16 at a time: sixteen groups of one copy each, ..., one group
    of sixteen copies."""
    _, arrays, nf, ref = case
    got, c = build_twice(skm, arrays, nf, {"key_range_passes": 16, "emit_group": eg})
    assert c["passes"] == 16 and c["grouped"] == c["valid"], c
    assert_same(got, ref)


def test_part_order_off(skm, gpu, case):
    """part_order 0: no order list is written or read; the starts and cursors still come from the
    emission-time kernel."""
    _, arrays, nf, ref = case
    got, _ = build_twice(skm, arrays, nf, {"key_range_passes": 16, "part_order": 0})
    assert_same(got, ref)


@pytest.mark.parametrize("first", [0, 1])
def test_routing(skm, gpu, case, first):
    """Heavy-key routing into the first half of 8 passes, and route_first: a heavy-only pass 0, far
    smaller than the others, most of its buckets empty.  route_first runs at 4 passes: from 8 passes
    on, this input's heavy pass outgrows the first-guess overflow buffers and the step is redone
    once, with or without the per-pass copies."""
    _, arrays, nf, ref = case
    opts = {"key_range_passes": 8, "route_heavy_min": 256}
    if first:
        opts.update(key_range_passes=4, route_first=1, route_first_min=256)
    got, c = build_twice(skm, arrays, nf, opts)
    assert c["routed"] > 100_000 and c["grouped"] == c["valid"], c
    assert_same(got, ref)


def test_one_pass_path_untouched(skm, gpu, case):
    """key_range_passes 1 keeps the per-workgroup histogram matrix and its scan kernels."""
    _, arrays, nf, ref = case
    got, c = build_twice(skm, arrays, nf, {"key_range_passes": 1})
    assert c["passes"] == 1, c
    assert_same(got, ref)


@pytest.mark.parametrize("world", [2, 4])
def test_world(skm, gpu, case, world):
    """In-process ranks: the histogram row spans every owner's buckets, k_send_counts reads the
    pass's copy of the starts, and the partition order comes from the received layout."""
    p, arrays, nf, ref = case
    ctrs = []
    opts = {"key_range_passes": 4, "main_long_class": 8, "overflow_long_class": 8}
    outs = run_group(skm, arrays, nf, world, lambda k: shard(p, world, k), opts, ctrs)
    check_against_oracle(outs[0], ref)
    for c in ctrs:
        assert c["passes"] == 4 and c["redone"] == 0, c
