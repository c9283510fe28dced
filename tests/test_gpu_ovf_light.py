"""Light remainders of overflow sub-buckets: k_ovf_split compacts them in place (to the front of the
sub-bucket's range) and k_ovf_light groups those of at most CAP = 2048 elements with the LDS hash
path (process_sub); with option ovf_light = 0 they go through k_overflow's sort instead.

Every input is built so that all its k-mers land in one level-2 sub-bucket: their 43-bit hashes
(mix43 of the base-40 code, skm_common.h, restated in planted.py) share the top 23 bits, i.e. the level-1
bucket (12 bits) and every level-2 split of up to 11 bits.  Each occurrence has a protein of its
own, X*a + 8-mer + X*b (exactly one valid window; length and offset vary), so the sub-bucket's size
and every group's size are exact.  Results are compared bit for bit with the CPU oracle, with
ovf_light 1 and 0; the counters tell which path took the remainder."""
import numpy as np
import pytest

import oracle_ref
from planted import CAP, HEAVY_MIN, Planter, assert_same

pytestmark = pytest.mark.gpu

NF = 6


def contents(p):
    """Every kind of group a remainder can hold (1,445 elements); returns {name: (kmer, kept)}."""
    want = {}
    p.singletons(40)
    want["pair_same"] = (p.group([2, 2]), True)
    want["pair_diff"] = (p.group([2, 3]), False)
    want["run3"] = (p.group([4] * 5), True)                        # best run >= 3: a chain job, lengths in tmp
    want["g64"] = (p.group([1] * 60 + [0] * 4), True)              # the largest packed-wave group
    want["g65"] = (p.group([1] * 62 + [5] * 3), True)              # the smallest k_big_groups hand-off
    want["g1023"] = (p.group([3] * 1000 + [2] * 23, long_at=7), True)  # stays light; one > 65535-residue protein
    want["g80"] = (p.group([0] * 80 + [4] * 20), True)             # exactly 80 %
    want["g79"] = (p.group([0] * 79 + [4] * 21), False)            # one member short
    want["s80"] = (p.group([5] * 8 + [1] * 2), True)
    want["s79"] = (p.group([5] * 7 + [1] * 3), False)
    want["long1"] = (p.group([2] * 4, long_at=1), True)
    want["tie"] = (p.group([1] * 10 + [3] * 10), False)
    return want


def remainder(p, n):
    """n light elements: groups of mixed sizes, then singletons."""
    left = n
    for c in (300, 65, 64, 17, 9, 5, 3, 2):
        if left >= c + 1:
            p.group([int(p.rng.integers(0, 2)) if c > 16 and k % 11 == 0 else 1 for k in range(c)])
            left -= c
    p.singletons(left)


def case_contents():
    p = Planter(1)
    p.heavy(1100)
    return p, contents(p), 1


def case_size(n):
    p = Planter(2 + n)
    p.heavy(2100, funcs=[1] * 1800 + [2] * 300)  # the sub-bucket is beyond CAP whatever the remainder
    remainder(p, n)
    return p, {}, 1 if 0 < n <= CAP else 0


def case_all_heavy():
    p = Planter(3)
    p.heavy(3000)
    return p, {}, 0


def case_boundary(size):
    p = Planter(100 + size)
    remainder(p, 700)
    p.heavy(size - 700)
    return p, {}, 1


def case_two_heavy():
    p = Planter(5)
    want = {"heavy_a": (p.heavy(1500), True)}
    want["heavy_1024"] = (p.plant(p.code(), [2] * HEAVY_MIN, False), True)      # exactly heavy_min: heavy
    want["light_1023"] = (p.plant(p.code(), [4] * (HEAVY_MIN - 1), True), True)  # one less: stays light
    p.singletons(30)
    return p, want, 1


CASES = {
    "contents": (case_contents, "shuffled", {}),
    "size_1": (lambda: case_size(1), "shuffled", {}),
    "size_cap": (lambda: case_size(CAP), "shuffled", {}),
    "size_cap_plus_1": (lambda: case_size(CAP + 1), "shuffled", {}),
    "all_heavy": (case_all_heavy, "shuffled", {}),
    "two_heavy": (case_two_heavy, "shuffled", {}),
    "passes_4": (case_contents, "shuffled", {"key_range_passes": 4}),
}
for _size in (4095, 4096, 4097, 8193):
    for _order in ("first", "last", "shuffled"):
        CASES[f"boundary_{_size}_{_order}"] = (lambda s=_size: case_boundary(s), _order, {})

_built = {}


def built(name):
    """The case's input and oracle result, computed once for both ovf_light settings."""
    if name not in _built:
        make, order, opts = CASES[name]
        p, want, nlight = make()
        arrays = p.arrays(order)
        ref = oracle_ref.build(*arrays, NF)
        _built[name] = (arrays, ref, want, nlight, int(np.count_nonzero(p.light)), len(p.seqs), opts)
    return _built[name]


@pytest.mark.parametrize("ovf_light", [1, 0])
@pytest.mark.parametrize("name", list(CASES))
def test_light_remainder(skm, gpu, name, ovf_light):
    arrays, ref, want, nlight, light_elems, total, opts = built(name)
    b = skm.SignatureBuilder(NF)
    for k, v in opts.items():
        b.set_option(k, v)
    b.set_option("ovf_light", ovf_light)
    b.add_batch(*arrays)
    got = b.finish()
    c = b.counters()
    b.close()
    assert_same(got, ref)
    # the planted k-mers are one overflow sub-bucket of exactly `total` elements
    assert c["overflow_subbuckets"] == 1 and c["overflow_elements"] == total
    if ovf_light:
        # a remainder of 1..CAP elements is k_ovf_light's; an empty or larger one is not
        assert c["overflow_light_subbuckets"] == nlight
        assert c["overflow_light_elements"] == (light_elems if nlight else 0)
    else:
        assert c["overflow_light_subbuckets"] == 0 and c["overflow_light_elements"] == 0
    kept = set(int(k) for k in got.keys)
    for what, (kmer, is_kept) in want.items():
        assert (int.from_bytes(kmer, "little") in kept) == is_kept, what
