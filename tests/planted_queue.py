"""Planted buckets for the (bucket, part) task queue of k_bucket_process (test_gpu_groupby_queue.py
builds them, test_planted_queue_cpu.py proves they are what they claim): Build B's and two of Build
A's scenarios (planted_scenarios.py) beside two buckets of 16 sub-buckets, two per part, and one of 1200 elements that is grouped in place
on one rank and split into two sub-buckets (b2 = 1) when it arrives from two."""
import numpy as np

import planted_scenarios as ps
from planted import CAP, Geometry, Scenario, assemble, b2_of, scenario_hashes

PARTS = 8  # BPK_PARTS of skm_build.hip


def parts16_edges(geom, prefix):
    """16 sub-buckets, parts of two.  Part 0: an empty sub-bucket first; its last (1000) and part
    1's first (1048) sum to exactly CAP (one batch for a walk of the whole bucket, two here), and
    part 1 ends with an empty one.  Part 2 starts and part 3 ends with an overflow sub-bucket
    (CAP + 1, skipped: k_overflow's).  Part 4 is empty, part 5 all overflow.  Part 7's last batch
    holds groups of more than 64 members and chain jobs (their length slots and big-group
    descriptors next to the bucket's end), then an empty sub-bucket."""
    sizes = (0, 1000, 1048, 0, CAP + 1, 300, 200, CAP + 1, 0, 0, CAP + 1, CAP + 1, 100, 200, 900, 0)
    sc = Scenario("parts16_edges", geom, prefix, 41, ps.NF, total=sum(sizes), sub_sizes=sizes, b2=4)
    for d, n in enumerate(sizes):
        if n > CAP:
            ps.fill_mix(sc, d, n, big=False)
            sc.overflow_subbuckets += 1
            sc.overflow_elements += n
        elif n:
            ps.fill_mix(sc, d, n, big=n >= 900, extras=d == 14)
    return sc


def parts16_plus_one(geom, prefix):
    """Part 0's last sub-bucket (1000) and part 1's first (1049) sum to CAP + 1: two batches either
    way.  Part 6 is one element in its second sub-bucket, part 7 one element in its first."""
    sizes = (500, 1000, 1049, 400, 700, 700, 600, 601, 0, 0, 300, 300, 0, 1, 1, 0)
    sc = Scenario("parts16_plus_one", geom, prefix, 42, ps.NF, total=sum(sizes), sub_sizes=sizes, b2=4)
    for d, n in enumerate(sizes):
        if n > 1:
            ps.fill_mix(sc, d, n, big=n >= 1000, extras=d == 2)
        elif n:
            sc.singletons(1, sub=d)
    return sc


def small_nsub2(geom, prefix):
    """1200 elements, 700 with the top bit of rem clear and 500 with it set.  One rank groups the
    bucket in place (<= CAP).  From two ranks (nsrc = 2) k_partition splits it with b2 = 1: nsub = 2
    is below the part count, parts 3 and 7 hold one sub-bucket each and the other six none, so the
    two halves are two batches where a walk of the whole bucket made one."""
    sc = Scenario("small_nsub2", geom, prefix, 43, ps.NF, total=1200, sub_sizes=(700, 500), b2=1)
    ps.fill_mix(sc, 0, 700, extras=True)
    ps.fill_mix(sc, 1, 500, big=False)
    return sc


_built = {}


def build_q(pass_bits=0):
    """Build B's scenarios, the three above, and Build A's buckets of exactly CAP beside them."""
    if pass_bits not in _built:
        geom = Geometry(pass_bits)
        makers = (ps.merge_exact, ps.merge_plus_one, ps.cap_beside_overflow, ps.just_over_a, ps.just_over_b,
                  parts16_edges, parts16_plus_one, ps.singletons_2048, ps.probe_wrap, small_nsub2)
        scs = [m(geom, ps.prefix_for(geom, 3 + k)) for k, m in enumerate(makers)]
        assert len(set(s.prefix for s in scs)) == len(scs)
        _built[pass_bits] = (scs, assemble(scs, 11))
    return _built[pass_bits]


def sizes_of(sc, two_ranks=False):
    """The sub-bucket sizes of k_partition's table, or None where the bucket is grouped in place: on
    one rank a bucket of at most CAP elements; from two ranks every bucket is partitioned, with b2
    from its total (the undeclared sizes come from the hashes)."""
    if sc.total > CAP:
        return tuple(sc.sub_sizes)
    if not two_ranks:
        return None
    if sc.sub_sizes is not None:
        return tuple(sc.sub_sizes)
    b2 = b2_of(sc.total)
    h = scenario_hashes(sc)[0]
    return tuple(int(x) for x in np.bincount(sc.geom.sub_of(h, b2).astype(np.int64), minlength=1 << b2))


def part_batches(sizes, parts=PARTS):
    """Batches per part of the part-restricted walk over a sub table (parts = 1: the whole bucket)."""
    nsub, out = len(sizes), []
    for c in range(parts):
        d, d1, n = c * nsub // parts, (c + 1) * nsub // parts, 0
        while d < d1:
            if sizes[d] == 0 or sizes[d] > CAP:
                d += 1
                continue
            tot = sizes[d]
            d += 1
            while d < d1 and tot + sizes[d] <= CAP:
                tot += sizes[d]
                d += 1
            n += 1
        out.append(n)
    return out


def batches_of(sc, parts=PARTS, two_ranks=False):
    """The process_sub batches k_bucket_process makes of the scenario."""
    sizes = sizes_of(sc, two_ranks)
    return 1 if sizes is None else sum(part_batches(sizes, parts))


def tasks_of(sc, two_ranks=False):
    """Its (bucket, part) tasks that hold a batch."""
    sizes = sizes_of(sc, two_ranks)
    return 1 if sizes is None else sum(1 for n in part_batches(sizes) if n)
