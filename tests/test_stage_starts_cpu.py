"""The staging's exact starts, without a GPU: the planted layouts of planted_stage.py hold the pass
and span counts they claim, and the table restated from planted_front.Windows (stage_table, what
test_gpu_stage_starts.py compares SignatureBuilder.debug_stage_starts with) has the invariants every
such table has: columns non-decreasing in w, the last row the next slice's start, the total the
pass's entry count."""
import numpy as np
import pytest

import planted_front as pf
import planted_stage as ps

P = ps.PASSES


def geometry(W, stage_round=1, world=1):
    counts = [int(x) for x in W.pass_counts(P)]
    g = pf.front_geometry(W.rp, P, max(counts), 0, stage_round, world)
    return counts, g["pf_span"], g["pf_nwg"]


@pytest.mark.parametrize("name", list(ps.LAYOUTS_S))
def test_layout_s_counts(name):
    lay = ps.LAYOUTS_S[name]()
    W = lay.windows
    counts, span, nwg = geometry(W)
    assert counts == lay.counts and W.n == sum(lay.counts) == lay.distinct
    assert len(np.unique(W.keys)) == W.n                       # every window is a singleton
    want_span, want_nwg, want_last = ps.S_CLAIMS[name]
    assert (span, nwg) == (want_span, want_nwg)
    assert 0 < counts[0] < ps.PH_TILE and counts[1] == 0       # a pass below one hist tile, an empty pass
    assert any(c % ps.PH_TILE for c in counts)                 # a k_pass_hist tail tile
    big = ps.span_counts(counts[3], span, nwg)
    assert big[:-1] == [span] * (nwg - 1) and big[-1] == want_last
    mid = ps.span_counts(counts[2], span, nwg)                 # ends inside its second span, then zero rows
    assert mid[0] == span and 0 < mid[1] < span and not any(mid[2:])
    assert not any(ps.span_counts(counts[1], span, nwg))
    # the same spans at stage_round 0
    assert geometry(W, stage_round=0)[1:] == (span, nwg)


def test_layout_h_counts():
    lay = ps.layout_h()
    W = lay.windows
    counts, span, nwg = geometry(W)
    q = lay.heavy_pass
    assert q >= P // 2                                          # the vacated half: routing moves the key
    assert counts[q] == ps.H_COPIES + ps.H_OTHERS // P and counts[q] == max(counts)
    assert (span, nwg) == (ps.MIN_SPAN, 3)
    passes, d = ps.destinations(W, P)
    dq = d[passes == q]
    assert len(np.unique(dq[:2 * span])) == 1                  # two whole spans of one destination
    assert len(np.unique(W.keys)) == lay.distinct
    t = ps.stage_table(W, P, q, span, nwg).astype(np.int64)
    flat = np.delete(np.arange(ps.N0), dq[0])
    assert np.array_equal(t[0, flat], t[1, flat]) and np.array_equal(t[1, flat], t[2, flat])
    assert t[2, dq[0]] - t[0, dq[0]] == 2 * span


@pytest.mark.parametrize("name", ["s1", "s2", "s3", "h"])
@pytest.mark.parametrize("world", [1, 2])
def test_table_invariants(name, world):
    lay = dict(ps.LAYOUTS_S, h=ps.layout_h)[name]()
    n = len(lay.arrays[2])
    for rank in range(world):
        W = lay.windows if world == 1 else pf.Windows(lay.arrays, np.arange(n) % 2 == rank)
        counts, span, nwg = geometry(W, world=world)
        passes, d = ps.destinations(W, P, world)
        assert np.array_equal(np.bincount(passes, minlength=P), counts)
        for q in range(P):
            t = ps.stage_table(W, P, q, span, nwg, world)
            assert t.shape == (nwg + 1, ps.N0)
            ps.check_invariants(t, counts[q])
            # a row's increments are the span's entries
            assert int(t[1:].astype(np.int64).sum() - t[:-1].astype(np.int64).sum()) == counts[q]
            rows = np.diff(t.astype(np.int64), axis=0).sum(1)
            assert [int(x) for x in rows] == ps.span_counts(counts[q], span, nwg)


def test_invariants_refuse_a_wrong_table():
    lay = ps.layout_s1()
    counts, span, nwg = geometry(lay.windows)
    t = ps.stage_table(lay.windows, P, 3, span, nwg)
    for r, c in ((0, 5), (nwg, 0), (nwg, ps.N0 - 1)):
        bad = t.copy()
        bad[r, c] += np.uint64(1)
        with pytest.raises(AssertionError):
            ps.check_invariants(bad, counts[3])
