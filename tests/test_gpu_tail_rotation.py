"""The pass tail beside the next pass's partition: with tail_async (one GPU, key-range passes) the
element buffers tmp and stg swap roles by pass parity, so the partition of a pass no longer waits
for the previous pass's tail -- only the staging of the pass after next does.

Every case compares the sorted hand-off (keys, records, the four statistics) with the CPU oracle
(oracle_build_mt) bit for bit, and asserts through counters() that every consumer of a pass's
element buffer ran: group-by chains, groups of > 64 members (k_big_groups), split overflow entries
with heavy keys, light remainders (k_ovf_light) and unsplit overflow entries (k_overflow).

The input: 20 000 proteins of ONE family (synth, 2 names: the family and the hypothetical proteins).
An ancestral 8-mer survives a member's substitutions with probability ~0.185, so the ~360
ancestral k-mers of the 13 000 members occur 2049..2477 times each -- more than CAP = 2048, one
overflow sub-bucket each, 15..32 of them in every one of 16 passes -- and ~450 more k-mers occur
65..2048 times (big groups in every pass).  An overflow entry is such a k-mer plus the 25..110
other elements of its sub-bucket (sub_target stays at its default: a larger one would put the
whole level-1 bucket, 840 elements at two passes, into every entry): split_min 2350 leaves about
half of the entries unsplit at every pass count, and heavy_min 64 makes the ancestral k-mer of a
split entry heavy, the rest of the entry its light remainder."""
import os

import numpy as np
import pytest

import oracle_ref
import planted
from planted import assert_same
from signature_kmers_amd import synth

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

OPTS = {"heavy_min": 64, "split_min": 2350, "main_long_class": 6, "overflow_long_class": 6}
_cache = {}


def _threads():
    return max(1, min(16, len(os.sched_getaffinity(0))))


def family():
    """The one-family input and its oracle result, computed once."""
    if "family" not in _cache:
        p = synth.generate_arrays(20000, 2, per_file=1000, seed=2)
        r, o, l, f, i, funcs = synth.build_inputs(p)
        ref = oracle_ref.build_mt(r, o, l, f, i, len(funcs), _threads(), sort=True)
        for a in (r, o, l, f, i, ref["keys"], ref["data"]):
            a.setflags(write=False)
        _cache["family"] = ((r, o, l, f, i), len(funcs), ref)
    return _cache["family"]


def one_range():
    """Planted k-mers whose hashes all lie in key range 2 of 4 (passes 0, 1 and 3 are empty): 300
    groups of 3..12 members, three of 65, 300 and 1500, and one of 2100 (an overflow sub-bucket)."""
    if "one" not in _cache:
        rng = np.random.default_rng(77)
        # (one code per call: each from a random place of the range, not 304 neighbours of one bucket)
        codes = [planted.codes(2, 2, 1, rng)[0] for _ in range(304)]
        sizes = [int(x) for x in rng.integers(3, 13, size=300)] + [65, 300, 1500, 2100]
        seqs, funcs = [], []
        for c, n in zip(codes, sizes):
            kmer = planted.kmer_of(c)
            major = int(rng.integers(1, 5))
            for _ in range(n):
                seqs.append(b"X" * int(rng.integers(0, 60)) + kmer + b"X" * int(rng.integers(0, 60)))
                funcs.append(major if rng.random() < 0.9 else int(rng.integers(1, 5)))
        perm = rng.permutation(len(seqs))
        r, o, l = planted.pack([seqs[k] for k in perm])
        arrays = (r, o, l, np.array(funcs, np.uint16)[perm], np.arange(len(seqs), dtype=np.uint32))
        assert len(seqs) <= 20000
        _cache["one"] = (arrays, 6, oracle_ref.build_mt(*arrays, 6, _threads(), sort=True))
    return _cache["one"]


def builder(skm, arrays, nf, passes, extra=None):
    b = skm.SignatureBuilder(nf)
    b.set_option("key_range_passes", passes)
    for k, v in {**OPTS, **(extra or {})}.items():
        b.set_option(k, v)
    b.add_batch(*arrays)
    return b


def assert_paths_ran(c, passes):
    """Every consumer of the pass's element buffer: no case passes by missing one."""
    assert c["passes"] == passes, c
    assert c["chain_jobs"] > 0 and c["big_groups"] > 0 and c["big_kept"] > 0, c
    assert c["overflow_subbuckets"] > 0 and c["overflow_kept"] > 0, c
    assert c["demand_split"] > 0, c                                   # entries of >= split_min went through k_ovf_split
    assert c["overflow_light_subbuckets"] > 0 and c["overflow_light_elements"] > 0, c
    assert c["overflow_light_subbuckets"] < c["overflow_subbuckets"], c   # and some entries stayed unsplit


@pytest.mark.parametrize("passes", [2, 4, 8, 16])
def test_pass_counts_match_the_oracle(skm, gpu, passes):
    """Both parities, with first and last passes of either parity."""
    arrays, nf, ref = family()
    b = builder(skm, arrays, nf, passes)
    b.run()
    c = b.counters()
    got = b.finish()
    flags = b.signature_flags()
    b.close()
    assert_paths_ran(c, passes)
    assert c["redone"] == 0, c
    assert_same(got, ref)
    assert int(np.count_nonzero(flags)) == ref["n_seqs_with_signature"]


def test_handle_reuse(skm, gpu):
    """Three runs on one handle: the parity and the pending tails start afresh each time."""
    arrays, nf, ref = family()
    b = builder(skm, arrays, nf, 16)
    outs = []
    for _ in range(3):
        b.run()
        c = b.counters()
        k = b.finish()
        outs.append((c, k.keys.tobytes(), k.data.tobytes(), b.signature_flags().tobytes(), k))
    b.close()
    assert_paths_ran(outs[0][0], 16)
    assert_same(outs[0][4], ref)
    def steady(c):  # without the host and device clocks and the hand-off's own figures
        return {k: v for k, v in c.items() if not k.endswith("_us") and not k.startswith("finish_")}

    for c, keys, data, flags, _ in outs[1:]:
        assert steady(c) == steady(outs[0][0])
        assert keys == outs[0][1] and data == outs[0][2] and flags == outs[0][3]


@pytest.mark.parametrize("passes", [4, 16])
def test_empty_passes(skm, gpu, passes):
    """Every key in one key range: the other passes stage, partition and tail nothing, and their
    joins and events still pair up (no hang: the file's per-test timeout)."""
    arrays, nf, ref = one_range()
    b = builder(skm, arrays, nf, passes, {"split_min": 2049})
    b.run()
    c = b.counters()
    got = b.finish()
    b.close()
    assert c["passes"] == passes and c["big_groups"] >= 3 and c["overflow_subbuckets"] >= 1 and c["chain_jobs"] > 0, c
    assert_same(got, ref)


def test_redo_path(skm, gpu):
    """Work buffers far too small: the first attempt records its demands with every pass skipped or
    run, the redo (grown buffers, the same handle state) matches, and so does the next run."""
    arrays, nf, ref = family()
    b = builder(skm, arrays, nf, 16, {"work_buffer_elements": 64, "poison_jobs": 1})
    b.run()
    c = b.counters()
    assert c["redone"] >= 1, c
    assert_paths_ran(c, 16)
    b.run()
    assert b.counters()["redone"] == c["redone"]
    got = b.finish()
    b.close()
    assert_same(got, ref)


@pytest.mark.parametrize("passes", [4, 16])
def test_tail_async_off(skm, gpu, passes):
    """tail_async 0: the tail on the main stream, the unrotated buffers."""
    arrays, nf, ref = family()
    b = builder(skm, arrays, nf, passes, {"tail_async": 0})
    b.run()
    c = b.counters()
    got = b.finish()
    b.close()
    assert_paths_ran(c, passes)
    assert_same(got, ref)
