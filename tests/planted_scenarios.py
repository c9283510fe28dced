"""The planted-bucket scenarios of test_planted_cpu.py (which proves they are what they claim) and
test_gpu_groupby_edges.py (which builds them): the integer edges of process_sub, seg_groups<S>,
k_big_groups, k_bucket_process::next_batch, k_partition and k_heavy (skm_build.hip).

Every `kept` flag below is written by hand from the reference rule (signature_build.tcc:219-293):
a k-mer is kept unless (float)best < float(count) * 0.8f, best the largest occurrence count of one
function.  For count < 2^24 that is exactly 5 * best >= 4 * count (test_planted_cpu.py checks it),
so exactly 80 % is kept, one member short is cut, and a tie for the best count (at most half of
the members) is always cut."""
import numpy as np

from planted import CAP, Geometry, Scenario, assemble, b2_of, best_mix

NF = 50
HI = NF - 1


def ceil80(c):
    return (4 * c + 4) // 5


def first_double(funcs, skip):
    """The first j, j and j + 1 not `skip`, with funcs[j] == funcs[j + 1]."""
    for j in range(len(funcs) - 1):
        if funcs[j] == funcs[j + 1] and j != skip and j + 1 != skip:
            return j
    raise AssertionError("no two adjacent members of one function")


def with_extras(sc, funcs, kept, **kw):
    """The group with one protein of more than 65535 residues and one that holds the k-mer twice."""
    return sc.group(funcs, kept, long_at=0, twice_at=first_double(funcs, 0), **kw)


def class_groups():
    """(member functions, kept) of groups at every size-class edge of seg_groups<S> (2, 3|4, 5|8,
    9|16, 17|32, 33|64).  Per class the count is no multiple of the groups a wave packs (32, 16, 8,
    4, 2, 1; the last class has one per wave), so each class ends in a partly filled wave task."""
    g = []
    for k in range(33):  # 33 pairs
        g.append(([k % NF] * 2, True) if k % 2 == 0 else ([k % NF, (k + 7) % NF], False))
    # 17 groups of 3-4
    g += [([0] * 3, True), ([HI] * 3, True), ([5] * 3, True), ([6] * 3, True), ([7] * 3, True)]
    g += [([8, 9, 8], False), ([HI, 0, HI], False), ([1, 2, 3], False), ([HI, 0, 4], False)]
    g += [([0] * 4, True), ([HI] * 4, True), ([11] * 4, True)]
    g += [([12, 12, 13, 12], False), ([0, HI, HI, HI], False)]           # 75 %
    g += [([0, HI, HI, 0], False), ([HI, 20, HI, 20], False), ([1, 2, 3, 4], False)]  # ties
    # 10 groups of 5-8
    g += [([3, 3, 9, 3, 3], True)]                       # 4 of 5: exactly 80 %
    g += [([3, 9, 3, 9, 3], False)]                      # 3 of 5: one short
    g += [([0] * 5, True), ([HI] * 8, True)]
    g += [([0, HI] * 4, False)]                          # tie 4 : 4, lowest and highest function
    g += [([0, 0, HI, HI, 7], False)]                    # tie 2 : 2 beside a third function
    g += [(best_mix(6, 5, 14, [2]), True), (best_mix(7, 6, HI, [0]), True), (best_mix(8, 7, 0, [HI]), True)]
    g += [(best_mix(8, 6, 15, [1, 2]), False)]           # 75 %
    # 7 groups of 9-16
    g += [([16] * 9, True), ([HI] * 16, True)]
    g += [(best_mix(10, 8, 17, [0, HI]), True), (best_mix(10, 7, 17, [0, HI]), False)]
    g += [(best_mix(15, 12, 0, [HI]), True), (best_mix(15, 11, 0, [HI]), False)]
    g += [([HI, 0] * 8, False)]                          # tie 8 : 8
    # 5 groups of 17-32
    g += [([18] * 17, True), ([0] * 32, True)]
    g += [(best_mix(20, 16, HI, [3, 4]), True), (best_mix(20, 15, HI, [3, 4]), False)]
    g += [([0, HI] * 16, False)]                         # tie 16 : 16
    # 7 groups of 33-64
    g += [([19] * 33, True), ([HI] * 64, True)]
    g += [(best_mix(40, 32, 21, [0]), True), (best_mix(40, 31, 21, [0]), False)]
    g += [(best_mix(60, 48, 0, [HI, 22]), True), (best_mix(60, 47, 0, [HI, 22]), False)]
    g += [([HI, 0] * 32, False)]                         # tie 32 : 32
    return g


CLASS_COUNTS = {2: 33, 4: 17, 8: 10, 16: 7, 32: 5, 64: 7}  # groups per segment size


# ---------------------------------------------------------------------------------------------
# Build A: the direct path (every bucket total <= CAP)
# ---------------------------------------------------------------------------------------------
def singletons_2048(geom, prefix):
    sc = Scenario("singletons_2048", geom, prefix, 11, NF, total=CAP)
    sc.singletons(CAP - 1)
    sc.group([7], True, long_at=0)
    return sc


def probe_wrap(geom, prefix):
    """640 keys whose home slot is one of the table's last 8: their probe chains wrap past slot
    4095; pairs, a group of 40 and a group of 70 are among them."""
    sc = Scenario("probe_wrap", geom, prefix, 12, NF, total=CAP)
    w = sc.take(640, where=lambda h: geom.slot_of(h) >= np.uint64(4088))
    f70 = best_mix(70, 56, 3, [4, 9])                                 # exactly 80 %; k_big_groups' hand-off
    sc.group(f70, True, code=w[0], long_at=0, twice_at=first_double(f70, 0))
    sc.group(best_mix(40, 31, 0, [HI]), False, code=w[1])             # one short of 32
    for k in range(100):
        if k % 2 == 0:
            sc.group([k % NF] * 2, True, code=w[2 + k])
        else:
            sc.group([k % NF, (k + 3) % NF], False, code=w[2 + k])
    for c in w[102:]:
        sc.group([int(sc.rng.integers(0, NF))], True, code=c)
    sc.singletons(CAP - sc.n_elements())
    sc.big_groups, sc.big_kept = 1, 1
    return sc


def pairs_1024(geom, prefix):
    """G = 1024 groups: all of big[CAP / 2]."""
    sc = Scenario("pairs_1024", geom, prefix, 13, NF, total=CAP)
    for k in range(1024):
        f = k % NF
        if k % 2 == 0:
            sc.group([f, f], True, twice_at=0 if k == 0 else None, long_at=1 if k == 2 else None)
        else:
            sc.group([f, (f + 1 + (k // 2) % (NF - 1)) % NF], False)
    return sc


def triples(geom, prefix):
    """682 chain jobs in one emit."""
    sc = Scenario("triples", geom, prefix, 14, NF, total=CAP)
    for k in range(682):
        sc.group([k % NF] * 3, True, long_at=1 if k == 5 else None, twice_at=0 if k == 9 else None)
    sc.group([4, 4], True)
    return sc


def classes(geom, prefix):
    sc = Scenario("classes", geom, prefix, 15, NF, total=1999)
    for funcs, kept in class_groups():
        if len(funcs) == 33:
            with_extras(sc, funcs, kept)
        else:
            sc.group(funcs, kept)
    sc.singletons(1999 - sc.n_elements())
    return sc


BIG_SIZES = (65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2047, 2048)


def big_e(geom, prefixes):
    """k_big_groups' E dispatch at 65, 128|129, 256|257, 512|513, 1024|1025 (the LARGE launch) and
    2048, each size pure, with best = ceil(0.8 c) and with one less; first-fit into buckets of at
    most CAP elements, a group of 2047 beside one singleton."""
    groups = []
    for c in sorted(BIG_SIZES, reverse=True):
        f = c % NF
        groups.append(([f] * c, True))
        groups.append((best_mix(c, ceil80(c), f, [(f + 1) % NF, (f + 9) % NF]), True))
        groups.append((best_mix(c, ceil80(c) - 1, f, [(f + 1) % NF, (f + 9) % NF]), False))
    bins = []
    for funcs, kept in groups:
        size = len(funcs) + (1 if len(funcs) == 2047 else 0)
        for b in bins:
            if b[0] + size <= CAP:
                b[0] += size
                b[1].append((funcs, kept))
                break
        else:
            bins.append([size, [(funcs, kept)]])
    out = []
    for k, (size, gs) in enumerate(bins):
        sc = Scenario(f"big_E_{k}", geom, prefixes[k], 100 + k, NF, total=size)
        for j, (funcs, kept) in enumerate(gs):
            if j == 0:
                with_extras(sc, funcs, kept)
            else:
                sc.group(funcs, kept)
            if len(funcs) == 2047:
                sc.singletons(1)
            sc.big_groups += 1
            sc.big_kept += 1 if kept else 0
        out.append(sc)
    return out


# ---------------------------------------------------------------------------------------------
# Build B: the partition path (bucket totals above CAP)
# ---------------------------------------------------------------------------------------------
def fill_mix(sc, sub, size, big=True, extras=False):
    """Exactly `size` elements in sub-bucket `sub`: a few big groups (not in an overflow
    sub-bucket, where k_bucket_process hands nothing over), the size-class groups as far as they
    fit, then singletons."""
    left = size
    todo = []
    if big:
        todo += [(best_mix(300, 240, 2, [5, 6]), True), ([9] * 129, True), (best_mix(65, 51, 1, [8]), False)]
    todo += sorted(class_groups(), key=lambda g: -len(g[0]))
    first = extras
    for funcs, kept in todo:
        if left < len(funcs) + 1:
            continue
        if first and len(funcs) >= 9:
            with_extras(sc, funcs, kept, sub=sub)
            first = False
        else:
            sc.group(funcs, kept, sub=sub)
        if len(funcs) > 64:
            sc.big_groups += 1
            sc.big_kept += 1 if kept else 0
        left -= len(funcs)
    assert not first or size < 10
    sc.singletons(left, sub=sub)


def merge_exact(geom, prefix):
    """Two batches of exactly CAP: sub-buckets 0 + 1, and 2 + 3."""
    sc = Scenario("merge_exact", geom, prefix, 21, NF, total=4096, sub_sizes=(1000, 1048, 2047, 1, 0, 0, 0, 0), b2=3)
    fill_mix(sc, 0, 1000, extras=True)
    fill_mix(sc, 1, 1048)
    fill_mix(sc, 2, 2047)
    sc.singletons(1, sub=3)
    return sc


def merge_plus_one(geom, prefix):
    """Sub-buckets 0 + 1 sum to CAP + 1: three batches."""
    sc = Scenario("merge_plus_one", geom, prefix, 22, NF, total=4096, sub_sizes=(1000, 1049, 2046, 1, 0, 0, 0, 0),
                  b2=3)
    fill_mix(sc, 0, 1000)
    fill_mix(sc, 1, 1049, extras=True)
    fill_mix(sc, 2, 2046)
    sc.singletons(1, sub=3)
    return sc


def cap_beside_overflow(geom, prefix):
    """A sub-bucket of exactly CAP (one group: the LARGE launch, lengths from tmp) is
    k_bucket_process's; the next, of CAP + 1 (light groups only), is k_overflow's."""
    sc = Scenario("cap_beside_overflow", geom, prefix, 23, NF, total=4100, sub_sizes=(0, 2048, 2049, 0, 3, 0, 0, 0),
                  b2=3)
    with_extras(sc, best_mix(2048, ceil80(2048), 30, [0, HI]), True, sub=1)
    sc.big_groups, sc.big_kept = 1, 1
    fill_mix(sc, 2, 2049, big=False)
    sc.group([HI] * 3, True, sub=4)
    sc.overflow_subbuckets, sc.overflow_elements = 1, 2049
    return sc


def just_over_a(geom, prefix):
    sc = Scenario("just_over_a", geom, prefix, 24, NF, total=2049, sub_sizes=(2048, 1, 0, 0), b2=2)
    fill_mix(sc, 0, 2048, extras=True)
    sc.singletons(1, sub=1)
    return sc


def just_over_b(geom, prefix):
    sc = Scenario("just_over_b", geom, prefix, 25, NF, total=2049, sub_sizes=(1, 0, 0, 2048), b2=2)
    sc.singletons(1, sub=0)
    fill_mix(sc, 3, 2048, extras=True)
    return sc


# ---------------------------------------------------------------------------------------------
# the builds
# ---------------------------------------------------------------------------------------------
def prefix_for(geom, k):
    """Scenario k's bucket: distinct level-1 buckets, spread over the passes (and both owners)."""
    bucket = (37 + 211 * k) % (1 << (geom.owner_bits + geom.b1_bits))
    return ((k % (1 << geom.pass_bits)) << (geom.owner_bits + geom.b1_bits)) | bucket


_built = {}


def build_a(pass_bits=0):
    """(scenarios, input arrays) of Build A at 2^pass_bits key-range passes."""
    if ("a", pass_bits) not in _built:
        geom = Geometry(pass_bits)
        sc = [singletons_2048(geom, prefix_for(geom, 0)), probe_wrap(geom, prefix_for(geom, 1)),
              pairs_1024(geom, prefix_for(geom, 2)), triples(geom, prefix_for(geom, 3)),
              classes(geom, prefix_for(geom, 4))]
        sc += big_e(geom, [prefix_for(geom, 5 + k) for k in range(16)])
        assert len(set(s.prefix for s in sc)) == len(sc)
        _built[("a", pass_bits)] = (sc, assemble(sc, 7))
    return _built[("a", pass_bits)]


def build_b(pass_bits=0):
    if ("b", pass_bits) not in _built:
        geom = Geometry(pass_bits)
        makers = (merge_exact, merge_plus_one, cap_beside_overflow, just_over_a, just_over_b)
        sc = [m(geom, prefix_for(geom, 3 + k)) for k, m in enumerate(makers)]
        _built[("b", pass_bits)] = (sc, assemble(sc, 8))
    return _built[("b", pass_bits)]


def heavy_table(nf):
    """One overflow sub-bucket (its keys share the top 11 bits of rem, so every level-2 split keeps
    them together) with two heavy keys for k_heavy: the best function of one is nf - 1 at exactly
    80 %, the other is a 50 : 50 tie; the remainder is singletons."""
    if ("h", nf) not in _built:
        geom = Geometry()
        total = 1500 + 1200 + 1500
        sub11 = 0x5A3
        sizes = [0] * 8
        sizes[sub11 >> 8] = total
        sc = Scenario(f"heavy_table_{nf}", geom, 777, 31, nf, total=total, sub_sizes=tuple(sizes), b2=b2_of(total))
        deep = (11, sub11)
        sc.top80 = with_extras(sc, best_mix(1500, 1200, nf - 1, [0, 17]), True, sub=deep)
        sc.tie = sc.group([3, nf - 1] * 600, False, sub=deep)
        sc.singletons(1500, sub=deep)
        sc.overflow_subbuckets, sc.overflow_elements = 1, total
        _built[("h", nf)] = ([sc], assemble([sc], 9))
    return _built[("h", nf)]
