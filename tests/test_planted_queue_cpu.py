"""The planted buckets of planted_queue.py are what they claim, without a GPU: every scenario's
windows hash into its bucket and into the declared level-2 sub-buckets, the declared split is the
kernel's choice, the overflow / big-group counts and the hand-written kept flags follow from the
members, and the part-restricted walk makes the batches the GPU test expects."""
import numpy as np
import pytest

import oracle_ref
from planted import CAP, b2_of, scenario_hashes
from planted_queue import PARTS, batches_of, build_q, part_batches, sizes_of, tasks_of


@pytest.mark.parametrize("pass_bits", [0, 2])
def test_scenarios_are_as_declared(pass_bits):
    scs, _ = build_q(pass_bits)
    for sc in scs:
        h, fn, kmers = scenario_hashes(sc)
        g = sc.geom
        assert np.all(g.prefix_of(h) == np.uint64(sc.prefix)), sc.name
        assert len(h) == sc.total == sc.n_elements(), (sc.name, len(h), sc.total)
        if sc.sub_sizes is None:
            assert sc.total <= CAP, sc.name
            over = np.zeros(len(h), bool)
        else:
            # small_nsub2 declares the split that two ranks' k_partition makes of a bucket <= CAP
            assert (sc.total > CAP or sc.name == "small_nsub2") and sc.b2 == b2_of(len(h)), sc.name
            sub = g.sub_of(h, sc.b2).astype(np.int64)
            got = np.bincount(sub, minlength=1 << sc.b2)
            assert tuple(int(x) for x in got) == tuple(sc.sub_sizes), (sc.name, got)
            over = got[sub] > CAP
        assert sc.overflow_subbuckets == (0 if sc.sub_sizes is None else sum(s > CAP for s in sc.sub_sizes)), sc.name
        assert sc.overflow_elements == int(np.count_nonzero(over)), sc.name
        km, cnt = np.unique(kmers[~over], return_counts=True)
        assert sc.big_groups == int(np.count_nonzero(cnt > 64)), (sc.name, sc.big_groups)
        assert sc.big_kept == sum(1 for k, c in zip(km, cnt) if c > 64 and sc.expect[int(k).to_bytes(8, "little")]), sc.name
        assert np.unique(kmers[over], return_counts=True)[1].max(initial=0) <= 64, sc.name  # light overflow only
        for kmer, funcs in sc.groups:
            best = max(np.bincount(funcs))
            assert sc.expect[kmer] == (5 * best >= 4 * len(funcs)), (sc.name, kmer)


def test_parts_and_batches():
    by = {sc.name: sc for sc in build_q(0)[0]}
    assert PARTS == 8
    # nsub = 8: one sub-bucket per part; nsub = 4: below the part count; nsub = 16: two per part
    assert [len(by[n].sub_sizes) for n in ("merge_exact", "just_over_a", "parts16_edges", "parts16_plus_one")] == [8, 4, 16, 16]
    want = {"merge_exact": (4, 2), "merge_plus_one": (4, 3), "cap_beside_overflow": (2, 2), "just_over_a": (2, 2),
            "just_over_b": (2, 2), "parts16_edges": (6, 3), "parts16_plus_one": (7, 4), "singletons_2048": (1, 1),
            "probe_wrap": (1, 1), "small_nsub2": (1, 1)}
    for name, (parts, whole) in want.items():
        assert (batches_of(by[name]), batches_of(by[name], 1)) == (parts, whole), name
    # from two ranks: nsub = 2 (b2 1) for the bucket of 1200, only parts 3 and 7 hold a sub-bucket;
    # nsub = 4 for the two buckets of exactly CAP (their sub-buckets are parts 1, 3, 5 and 7)
    small = by["small_nsub2"]
    assert small.b2 == 1 and sizes_of(small) is None and sizes_of(small, True) == (700, 500)
    assert part_batches(sizes_of(small, True)) == [0, 0, 0, 1, 0, 0, 0, 1] and part_batches((700, 500), 1) == [1]
    assert (batches_of(small, two_ranks=True), tasks_of(small, True)) == (2, 2)
    for name in ("singletons_2048", "probe_wrap"):
        z = sizes_of(by[name], True)
        assert len(z) == 4 and sum(z) == CAP and part_batches(z)[0::2] == [0] * 4 and sum(part_batches(z)) >= 1, (name, z)
    e = by["parts16_edges"].sub_sizes
    assert e[1] + e[2] == CAP and e[0] == e[3] == 0            # the pair across the parts 0 | 1 boundary
    assert e[4] == e[7] == CAP + 1                              # overflow first of part 2, last of part 3
    assert [bool(n) for n in part_batches(e)] == [True, True, True, True, False, False, True, True]
    q = by["parts16_plus_one"].sub_sizes
    assert q[1] + q[2] == CAP + 1
    # the last batch of the last part holds groups of > 64 members and chain jobs (groups of >= 3 of one function)
    last = by["parts16_edges"]
    h, fn, kmers = scenario_hashes(last)
    sub = last.geom.sub_of(h, 4)
    cnt = np.unique(kmers[sub == np.uint64(14)], return_counts=True)[1]
    assert cnt.max() > 64 and np.count_nonzero(cnt >= 3) > 10 and len(kmers[sub == np.uint64(15)]) == 0


def test_oracle_agrees_with_expectations():
    scs, arrays = build_q(0)
    ref = oracle_ref.build(*arrays, scs[0].nf)
    kept = set(int(k) for k in ref["keys"])
    for sc in scs:
        wrong = [k for k, is_kept in sc.expect.items() if (int.from_bytes(k, "little") in kept) != is_kept]
        assert not wrong, (sc.name, wrong[:5], len(wrong))
