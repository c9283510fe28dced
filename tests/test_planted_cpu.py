"""The planted scenarios are what test_gpu_groupby_edges.py claims (no GPU): every planted window,
re-hashed from the residues, lies in its scenario's bucket, sub-bucket and slot range; bucket and
sub-bucket sizes, the b2 they imply and the batches they form are the declared ones; and the
oracle's kept set agrees with every hand-written expectation."""
import numpy as np
import pytest

import oracle_ref
import planted_scenarios as ps
from planted import (CAP, HV_FT, KEY_MASK, NCODES, Geometry, b2_of, codes, mix43, scenario_hashes, unmix43)

BUILDS = {
    "a": lambda: ps.build_a(0),
    "b": lambda: ps.build_b(0),
    "a_passes4": lambda: ps.build_a(2),
    "b_passes4": lambda: ps.build_b(2),
    "heavy_4096": lambda: ps.heavy_table(HV_FT),
    "heavy_4097": lambda: ps.heavy_table(HV_FT + 1),
}
_facts = {}


def facts(name):
    """Per scenario of the build: hash, function and k-mer of every planted window."""
    if name not in _facts:
        scs, arrays = BUILDS[name]()
        _facts[name] = (scs, arrays, {sc.name: scenario_hashes(sc) for sc in scs})
    return _facts[name]


def by_name(name, scenario):
    scs, _, fx = facts(name)
    sc = next(s for s in scs if s.name == scenario)
    return sc, fx[scenario]


def group_sizes(kmers):
    return np.unique(kmers, return_counts=True)[1]


def batches(sizes):
    """k_bucket_process::next_batch restated: runs of consecutive sub-buckets of at most CAP
    elements in total; empty sub-buckets and those beyond CAP (k_overflow's) are skipped."""
    out, d = [], 0
    while d < len(sizes):
        if sizes[d] == 0 or sizes[d] > CAP:
            d += 1
            continue
        tot, d2 = sizes[d], d + 1
        while d2 < len(sizes) and tot + sizes[d2] <= CAP:
            tot += sizes[d2]
            d2 += 1
        out.append(tot)
        d = d2
    return out


def test_unmix43_inverts_mix43():
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.integers(0, 1 << 43, 100000, dtype=np.uint64),
                        np.array([0, 1, 2, NCODES - 1, NCODES, KEY_MASK - 1, KEY_MASK, 1 << 42, (1 << 22) - 1,
                                  1 << 22], np.uint64)])
    assert np.array_equal(unmix43(mix43(x)), x)
    assert np.array_equal(mix43(unmix43(x)), x)


def test_codes_have_their_prefix():
    rng = np.random.default_rng(4)
    g = Geometry(2)
    c = codes(g.prefix_bits, 0x2ABC, 3000, rng, where=lambda h: g.slot_of(h) == np.uint64(4095))
    assert len(np.unique(c)) == 3000 and np.all(c < np.uint64(NCODES))
    h = mix43(c)
    assert np.all(g.prefix_of(h) == np.uint64(0x2ABC)) and np.all(g.slot_of(h) == np.uint64(4095))
    c = codes(23, 0x5A5A5A, 5000, rng)  # 2^20 low values: the walk wraps
    assert len(np.unique(c)) == 5000 and np.all(mix43(c) >> np.uint64(20) == np.uint64(0x5A5A5A))


def test_geometry_and_b2():
    assert (Geometry().prefix_bits, Geometry().rem_bits) == (12, 31)
    assert (Geometry(2).prefix_bits, Geometry(2).rem_bits) == (14, 29)
    assert (Geometry(0, 1).b1_bits, Geometry(0, 1).rem_bits) == (11, 31)
    assert (Geometry(0, 2).b1_bits, Geometry(0, 2).rem_bits) == (11, 30)
    assert [b2_of(n) for n in (1, 768, 769, 1537, 1538, 2049, 4096, 4100, 768 << 11, 1 << 30)] == \
        [0, 0, 1, 1, 2, 2, 3, 3, 11, 11]


def test_fp32_cut_is_the_exact_rule():
    """(float)best < float(c) * 0.8f, for every group size a 16-bit rank can count and every best
    count near the cut: the same as 5 * best < 4 * c, in fp32 and in double alike."""
    c = np.arange(1, 65536, dtype=np.int64)
    for d in (-2, -1, 0, 1, 2):
        best = np.clip((4 * c + 4) // 5 + d, 0, c)
        cut32 = best.astype(np.float32) < c.astype(np.float32) * np.float32(0.8)
        cut64 = best.astype(np.float64) < c.astype(np.float64) * 0.8
        exact = 5 * best < 4 * c
        assert np.array_equal(cut32, exact) and np.array_equal(cut64, exact)


@pytest.mark.parametrize("name", list(BUILDS))
def test_scenarios_are_as_declared(name):
    scs, _, fx = facts(name)
    assert len(set(sc.prefix for sc in scs)) == len(scs)
    for sc in scs:
        h, fn, kmers = fx[sc.name]
        g = sc.geom
        assert np.all(g.prefix_of(h) == np.uint64(sc.prefix)), sc.name
        assert len(h) == sc.total == sc.n_elements(), (sc.name, len(h), sc.total)
        sizes = sorted(group_sizes(kmers))
        assert sizes == sorted(len(f) for _, f in sc.groups), sc.name
        if sc.sub_sizes is None:
            assert sc.total <= CAP, sc.name
            over = np.zeros(len(h), bool)
        else:
            assert sc.total > CAP and sc.b2 == b2_of(len(h)), sc.name
            sub = g.sub_of(h, sc.b2).astype(np.int64)
            got = np.bincount(sub, minlength=1 << sc.b2)
            assert tuple(int(x) for x in got) == tuple(sc.sub_sizes), (sc.name, got)
            over = got[sub] > CAP
        assert sc.overflow_subbuckets == (0 if sc.sub_sizes is None else sum(s > CAP for s in sc.sub_sizes)), sc.name
        assert sc.overflow_elements == int(np.count_nonzero(over)), sc.name
        # the groups of more than 64 members that k_bucket_process hands to k_big_groups
        km, cnt = np.unique(kmers[~over], return_counts=True)
        assert sc.big_groups == int(np.count_nonzero(cnt > 64)), (sc.name, sc.big_groups)
        keptbig = sum(1 for k, c in zip(km, cnt) if c > 64 and sc.expect[int(k).to_bytes(8, "little")])
        assert sc.big_kept == keptbig, sc.name
        if max(sizes) > 1:
            assert sc.has_long and sc.has_twice, sc.name
            assert max(len(s) for s in sc.seqs) > 65535
        # every hand-written expectation is the exact rule's
        for kmer, funcs in sc.groups:
            best = max(np.bincount(funcs))
            assert sc.expect[kmer] == (5 * best >= 4 * len(funcs)), (sc.name, kmer)


def test_build_a_edges():
    sc, (h, fn, kmers) = by_name("a", "singletons_2048")
    assert len(np.unique(kmers)) == CAP
    sc, (h, fn, kmers) = by_name("a", "probe_wrap")
    km, first, cnt = np.unique(kmers, return_index=True, return_counts=True)
    wrapped = sc.geom.slot_of(h[first]) >= np.uint64(4088)
    assert np.count_nonzero(wrapped) >= 600 and len(kmers) == CAP and len(km) < 4096
    assert {70, 40, 2} <= set(cnt[wrapped].tolist())
    sc, (h, fn, kmers) = by_name("a", "pairs_1024")
    assert group_sizes(kmers).tolist() == [2] * 1024                      # G = 1024 = len(big)
    assert sum(sc.expect.values()) == 512
    sc, (h, fn, kmers) = by_name("a", "triples")
    assert sorted(group_sizes(kmers).tolist()) == [2] + [3] * 682 and all(sc.expect.values())
    sc, (h, fn, kmers) = by_name("a", "classes")
    cnt = group_sizes(kmers)
    assert {2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64} <= set(cnt.tolist()) and cnt.max() == 64
    for seg, per in ((2, 32), (4, 16), (8, 8), (16, 4), (32, 2), (64, 1)):
        n = int(np.count_nonzero((cnt > seg // 2) & (cnt <= seg)))
        assert n == ps.CLASS_COUNTS[seg] and (per == 1 or n % per != 0), (seg, n)
    assert np.count_nonzero(cnt == 1) > 0
    # exactly 80 % and one short at 5, 10, 15, 20, 40, 60; functions 0 and nf - 1
    seen = {(len(f), int(max(np.bincount(f)))) for _, f in sc.groups}
    for c in (5, 10, 15, 20, 40, 60):
        assert (c, 4 * c // 5) in seen and (c, 4 * c // 5 - 1) in seen
    scs = [s for s in facts("a")[0] if s.name.startswith("big_E")]
    assert all(s.total <= CAP for s in scs) and any(s.total == CAP for s in scs)
    seen = sorted((len(f), int(max(np.bincount(f)))) for s in scs for _, f in s.groups if len(f) > 1)
    assert seen == sorted((c, b) for c in ps.BIG_SIZES for b in (c, ps.ceil80(c), ps.ceil80(c) - 1))
    assert sum(s.big_groups for s in scs) == 33 and sum(s.big_kept for s in scs) == 22


def test_build_b_batches():
    want = {"merge_exact": [2048, 2048], "merge_plus_one": [1000, 1049, 2047], "cap_beside_overflow": [2048, 3],
            "just_over_a": [2048, 1], "just_over_b": [1, 2048]}
    for sc in facts("b")[0]:
        assert batches(sc.sub_sizes) == want[sc.name], sc.name
    sc, (h, fn, kmers) = by_name("b", "cap_beside_overflow")
    sub = sc.geom.sub_of(h, 3)
    assert group_sizes(kmers[sub == np.uint64(1)]).tolist() == [2048]
    assert group_sizes(kmers[sub == np.uint64(2)]).max() <= 64        # light groups only


@pytest.mark.parametrize("nf", [HV_FT, HV_FT + 1])
def test_heavy_table_scenario(nf):
    sc = facts(f"heavy_{nf}")[0][0]
    h, fn, kmers = facts(f"heavy_{nf}")[2][sc.name]
    assert len(np.unique(sc.geom.sub_of(h, 11))) == 1 and len(h) >= 4096
    f80 = dict(sc.groups)[sc.top80]
    assert np.bincount(f80).argmax() == nf - 1 and 5 * f80.count(nf - 1) == 4 * len(f80) >= 5 * 1024
    ft = dict(sc.groups)[sc.tie]
    assert ft.count(3) == ft.count(nf - 1) == len(ft) // 2 >= 512
    assert sc.expect[sc.top80] and not sc.expect[sc.tie] and fn.max() == nf - 1


@pytest.mark.parametrize("name", list(BUILDS))
def test_oracle_agrees_with_expectations(name):
    scs, arrays, _ = facts(name)
    ref = oracle_ref.build(*arrays, scs[0].nf)
    kept = set(int(k) for k in ref["keys"])
    for sc in scs:
        wrong = [k for k, is_kept in sc.expect.items() if (int.from_bytes(k, "little") in kept) != is_kept]
        assert not wrong, (sc.name, wrong[:5], len(wrong))
    assert len(kept) == sum(sum(sc.expect.values()) for sc in scs)
