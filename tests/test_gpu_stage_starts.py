"""The staging's exact starts on the GPU (planted_stage.py; test_stage_starts_cpu.py proves the
layouts and the restated table without one): with key-range passes k_pass_hist counts every staging
span's entries per level-0 destination, k_pass_starts scans the columns into the pass's copy, and
k_extract_stage_pos appends from that table without a global atomic.  Every build is compared bit
for bit with the oracle (a window stored outside its slice is a lost or foreign element of some
bucket), runs twice on one handle with equal counters and redone == 0 (a workgroup whose cursors do
not end on the next row fails the run), and SignatureBuilder.debug_stage_starts() of every pass of
the last emission group must equal the restatement exactly -- after a routed run, whose spans follow
the routed pass sizes, its invariants."""
import numpy as np
import pytest

import oracle_ref
import planted_front as pf
import planted_stage as ps
from planted import assert_same

pytestmark = pytest.mark.gpu

P = ps.PASSES
_ref = {}


def reference(name):
    """(layout, oracle result), computed once per layout."""
    if name not in _ref:
        lay = dict(ps.LAYOUTS_S, h=ps.layout_h)[name]()
        _ref[name] = (lay, oracle_ref.build(*lay.arrays, lay.nf))
    return _ref[name]


def check_tables(b, W, opts, world=1, routed=False):
    """debug_front() and debug_stage_starts() of one handle against the windows W of its shard."""
    counts = [int(x) for x in W.pass_counts(P)]
    front = b.debug_front()
    eg = front["emit_g"]
    assert eg == max(1, min(P, opts.get("emit_group", 0) or 4))
    if not routed:
        want = pf.front_geometry(W.rp, P, max(counts), opts.get("emit_group", 0), opts.get("stage_round", 1), world)
        assert front == want
        assert b.debug_pass_windows() == counts
    span, nwg = front["pf_span"], front["pf_nwg"]
    sizes = b.debug_pass_windows()
    assert sum(sizes) == W.n and max(sizes) <= span * nwg
    last = (P - 1) // eg * eg
    for q in range(last, P):   # the read-out covers the last emission group
        t = b.debug_stage_starts(q)
        assert t.shape == (nwg + 1, ps.N0)
        ps.check_invariants(t, sizes[q])
        if not routed:
            np.testing.assert_array_equal(t, ps.stage_table(W, P, q, span, nwg, world))
    return last


def build(skm, name, opts, routed=False):
    lay, ref = reference(name)
    opts = dict(opts, key_range_passes=P)
    W = lay.windows
    b = skm.SignatureBuilder(lay.nf)
    for k, v in opts.items():
        b.set_option(k, v)
    b.add_batch(*lay.arrays)
    b.run()
    c1 = b.counters()
    last = check_tables(b, W, opts, routed=routed)
    if last > 0:
        with pytest.raises(skm.SkmError):   # a pass of an earlier group: its copy is overwritten
            b.debug_stage_starts(0)
    b.run()
    c2 = b.counters()
    check_tables(b, W, opts, routed=routed)
    got = b.finish()
    b.close()
    assert c1 == c2
    assert c1["passes"] == P and c1["redone"] == 0, c1
    assert (c1["windows"], c1["valid"], c1["grouped"]) == (W.positions, W.n, W.n), c1
    assert_same(got, ref)
    assert len(got.keys) == lay.distinct
    return c1


@pytest.mark.parametrize("name", list(ps.LAYOUTS_S))
def test_layout_s(skm, gpu, name):
    """Four passes in one emission group: the largest in four spans of 16,384 with exactly one entry
    in the last (s1), in three spans of 12,288 (s2), in exactly three full spans (s3); a pass of fewer
    than 2048 entries, an empty pass, a pass that ends inside its second span."""
    c = build(skm, name, {})
    assert c["routed"] == 0


def test_layout_s_round0(skm, gpu):
    """The whole-round staging kernel (4096 elements a round, two workgroups per CU)."""
    build(skm, "s1", {"stage_round": 0})


@pytest.mark.parametrize("eg", [1, 16])
def test_layout_s_emit_group(skm, gpu, eg):
    """One pass per emission group (the copies alternate between the two sets, the read-out is the
    last pass's alone), and the largest group."""
    build(skm, "s1", {"emit_group": eg})


def test_layout_h(skm, gpu):
    """40,000 copies of one 8-residue protein: two whole spans of the key's pass go to a single
    destination (the other 63 columns are flat over them), nothing routed."""
    c = build(skm, "h", {"route_heavy_min": 1 << 30, "route_first": 0})
    assert c["routed"] == 0


def test_layout_h_routed(skm, gpu):
    """The same with routing on: the key moves into an earlier pass and the spans follow the routed
    pass sizes, so the table is held to its invariants."""
    c = build(skm, "h", {"route_heavy_min": 1024, "route_first": 0}, routed=True)
    assert c["routed"] >= ps.H_COPIES, c


def test_layout_s_two_ranks(skm, gpu):
    """Even sequences on rank 0, odd ones on rank 1, both on one GPU: every rank stages its own
    windows from its own table (owner bit above the level-1 bucket bits).  The group's sequence
    order is (rank, sequence), so the oracle gets the input in that order."""
    lay, _ = reference("s3")
    r, o, l, f, i = lay.arrays
    n = len(l)
    if "s3_world2" not in _ref:
        order = np.concatenate([np.arange(0, n, 2), np.arange(1, n, 2)])
        _ref["s3_world2"] = oracle_ref.build(r, o[order], l[order], f[order], i[order], lay.nf)
    ref = _ref["s3_world2"]
    opts = {"key_range_passes": P}
    bs, Ws = [], []
    for rank in range(2):
        sel = np.arange(n) % 2 == rank
        b = skm.SignatureBuilder(lay.nf, device=0, rank=rank, world_size=2)
        for k, v in opts.items():
            b.set_option(k, v)
        idx = np.nonzero(sel)[0]
        b.add_batch(r, o[idx], l[idx], f[idx], i[idx])
        bs.append(b)
        Ws.append(pf.Windows(lay.arrays, sel))
    assert Ws[0].n + Ws[1].n == lay.windows.n and min(W.n for W in Ws) > 30000
    skm.group_run(bs)
    c1 = [b.counters() for b in bs]
    for b, W in zip(bs, Ws):
        check_tables(b, W, opts, world=2)
    skm.group_run(bs)
    c2 = [b.counters() for b in bs]
    for b, W in zip(bs, Ws):
        check_tables(b, W, opts, world=2)
    outs = [b.finish() for b in bs]
    for b in bs:
        b.close()
    assert c1 == c2
    for c, W in zip(c1, Ws):
        assert c["passes"] == P and c["redone"] == 0 and c["routed"] == 0, c
        assert (c["windows"], c["valid"]) == (W.positions, W.n), c
    assert sum(c["grouped"] for c in c1) == lay.windows.n
    assert_same(outs[0], ref)
