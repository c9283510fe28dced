"""The build's extraction front end on planted window layouts (planted_front.py;
test_planted_front_cpu.py proves the layouts without a GPU): k_pass_ids, k_sel_scan, k_pass_emit<G>,
k_pass_hist and k_extract_stage_pos<R> with key-range passes, k_extract, k_extract_stage,
k_split_stage and k_blk2seq with one pass.

Layout G has emission rows of 2064 windows (two full tiles and a short one), most of them empty,
with windows on chosen row, tile, chunk and lane-byte offsets, full tiles of one pass, sequences of
0..8 residues, dropped sequences and the longest accepted protein.  Layout E has passes without a
window; the tails end on the last residue at every rp mod 16 that matters.  Every window is its own
kept key (the homopolymers aside), so the bit-for-bit compare with the oracle sees every lost,
extra or misplaced window.  Every build also checks debug_front() against the restated geometry
-- a mismatch fails, the test does not adapt --, debug_pass_windows() and the counters against the
layout's counts, and runs twice on one handle."""
import numpy as np
import pytest

import oracle_ref
import planted_front as pf
from planted import assert_same

pytestmark = pytest.mark.gpu

_ref = {}


def reference(name, make):
    """(layout, oracle result), computed once per layout."""
    if name not in _ref:
        lay = make()
        _ref[name] = (lay, oracle_ref.build(*lay.arrays, lay.nf))
    return _ref[name]


def check_front(b, W, opts, world=1, routed=False):
    """debug_front() and debug_pass_windows() of one handle against the windows W of its shard."""
    P = opts["key_range_passes"]
    counts = [int(x) for x in W.pass_counts(P)]
    want = pf.front_geometry(W.rp, P, max(counts), opts.get("emit_group", 0), opts.get("stage_round", 1), world)
    front = b.debug_front()
    if routed:  # the staged scatter's grid follows the routed pass sizes
        for f in ("pf_span", "pf_nwg"):
            want.pop(f), front.pop(f)
    assert front == want
    if not routed:
        assert b.debug_pass_windows() == counts


def build(skm, lay, ref, opts, routed=False):
    W = lay.windows
    b = skm.SignatureBuilder(lay.nf)
    for k, v in opts.items():
        b.set_option(k, v)
    b.add_batch(*lay.arrays)
    b.run()
    c1 = b.counters()
    check_front(b, W, opts, routed=routed)
    b.run()
    c2 = b.counters()
    got = b.finish()
    b.close()
    assert c1 == c2
    assert c1["passes"] == opts["key_range_passes"] and c1["redone"] == 0, c1
    assert (c1["windows"], c1["valid"], c1["grouped"]) == (W.positions, W.n, W.n), c1
    assert_same(got, ref)
    assert len(got.keys) == lay.distinct
    return c1


# ---------------------------------------------------------------------------------------------
# Layout G
# ---------------------------------------------------------------------------------------------
G_RUNS = {
    "passes1": {"key_range_passes": 1},
    "passes4": {"key_range_passes": 4},
    "passes16": {"key_range_passes": 16},
    "passes64": {"key_range_passes": 64},
    "passes16_emit1": {"key_range_passes": 16, "emit_group": 1},
    "passes16_emit2": {"key_range_passes": 16, "emit_group": 2},
    "passes16_emit16": {"key_range_passes": 16, "emit_group": 16},     # the non-packed form at full tiles
    "passes16_round0": {"key_range_passes": 16, "stage_round": 0},
}


@pytest.mark.parametrize("run", list(G_RUNS))
def test_layout_g(skm, gpu, run):
    lay, ref = reference("g", pf.layout_g)
    c = build(skm, lay, ref, G_RUNS[run])
    assert c["routed"] == 0


@pytest.mark.parametrize("first", [0, 1])
def test_layout_g_routed(skm, gpu, first):
    """The upper-half homopolymer (two full rows of one key) is routed into the first half of 16
    passes, or into the heavy-only pass 0 of 4: full tiles of a pass that is not the hash's own."""
    lay, ref = reference("g", pf.layout_g)
    opts = {"key_range_passes": 16, "route_heavy_min": 1024, "route_first": 0}
    if first:
        opts = {"key_range_passes": 4, "route_first": 1, "route_first_min": 1024}
    c = build(skm, lay, ref, opts, routed=True)
    upper = lay.homo[1]
    assert upper[0] == bytes([lay.claims["upper"]]) * 8 and upper[2] == pf.G_UPPER_LEN - 7
    assert c["routed"] >= upper[2], c


def test_layout_g_two_ranks(skm, gpu):
    """Even sequences on rank 0, odd ones on rank 1: each rank has rows of its own span (rank 0 a
    full tile and a part of one, rank 1 less than a tile), so every island sits at another row and
    lane offset than on one rank, and its own sequence numbering base.  The group's sequence order is (rank, sequence), so the
    oracle gets the input in that order."""
    lay, _ = reference("g", pf.layout_g)
    r, o, l, f, i = lay.arrays
    n = len(l)
    if "g_world2" not in _ref:
        order = np.concatenate([np.arange(0, n, 2), np.arange(1, n, 2)])
        _ref["g_world2"] = oracle_ref.build(r, o[order], l[order], f[order], i[order], lay.nf)
    ref = _ref["g_world2"]
    opts = {"key_range_passes": 4}
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
    assert Ws[0].n + Ws[1].n == lay.windows.n and min(W.n for W in Ws) > 300
    spans = [pf.sel_geometry(W.rp)[1] for W in Ws]
    assert pf.TILE < spans[0] < pf.G_SPAN and spans[1] < pf.TILE   # more than a tile, less than a tile
    skm.group_run(bs)
    c1 = [b.counters() for b in bs]
    for b, W in zip(bs, Ws):
        check_front(b, W, opts, world=2)
    skm.group_run(bs)
    c2 = [b.counters() for b in bs]
    outs = [b.finish() for b in bs]
    for b in bs:
        b.close()
    assert c1 == c2
    for c, W in zip(c1, Ws):
        assert c["passes"] == 4 and c["redone"] == 0 and c["routed"] == 0, c
        assert (c["windows"], c["valid"]) == (W.positions, W.n), c
    assert sum(c["grouped"] for c in c1) == lay.windows.n
    assert_same(outs[0], ref)


# ---------------------------------------------------------------------------------------------
# Layout E: passes without a window
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eg", [0, 16, 1])
@pytest.mark.parametrize("name", ["e64", "e4"])
def test_empty_passes(skm, gpu, name, eg):
    """Windows in passes 0, 37 and 63 of 64 (pass 63 only in the last occupied row; the smallest and
    the largest hash with a valid code), and in pass 2 of 4: every other pass has nothing to stage,
    partition or group."""
    lay, ref = reference(name, pf.layout_e64 if name == "e64" else pf.layout_e4)
    P = lay.claims["passes"]
    assert [int(p) for p in np.nonzero(lay.pass_counts[P])[0]] == lay.claims["natural"]
    opts = {"key_range_passes": P}
    if eg:
        opts["emit_group"] = eg
    build(skm, lay, ref, opts)


@pytest.mark.parametrize("passes", [1, 64])
def test_single_window(skm, gpu, passes):
    lay, ref = reference("one", pf.layout_one)
    c = build(skm, lay, ref, {"key_range_passes": passes})
    assert c["kept"] == 1


def test_no_window_with_passes(skm, gpu):
    """Zero windows in every one of 16 passes: an empty kept set, no fault."""
    lay, ref = reference("none", pf.layout_none)
    c = build(skm, lay, ref, {"key_range_passes": 16})
    assert c["kept"] == 0 and c["valid"] == 0 and len(ref["keys"]) == 0


# ---------------------------------------------------------------------------------------------
# the end of the buffer, and the longest protein
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("passes", [1, 4])
@pytest.mark.parametrize("mod", pf.TAIL_MODS)
def test_tails(skm, gpu, mod, passes):
    """The last window ends on the last residue, rp mod 16 = mod."""
    lay, ref = reference(f"tail{mod}", lambda: pf.layout_tail(mod))
    c = build(skm, lay, ref, {"key_range_passes": passes})
    assert c["kept"] == 4


def test_too_long_protein_is_refused(skm, gpu):
    """1,048,576 residues do not fit the element's 20-bit offset: add_batch refuses the batch (the
    longest accepted protein, one residue shorter, is in layout G), takes nothing of it, and the
    builder still builds a following valid batch."""
    lay, ref = reference("tail7", lambda: pf.layout_tail(7))
    good = b"ACDEFGHIKLMN"
    long_ = b"WYVTSRQP" + b"X" * (pf.MAX_LEN + 1 - 16) + b"PQRSTVWY"
    assert len(long_) == pf.MAX_LEN + 1 == 1 << 20
    res = np.frombuffer(good + long_, np.uint8)
    off = np.array([0, len(good)], np.uint64)
    lens = np.array([len(good), len(long_)], np.uint32)
    b = skm.SignatureBuilder(lay.nf)
    with pytest.raises(skm.SkmError):
        b.add_batch(res, off, lens, np.array([1, 2], np.uint16), np.arange(2, dtype=np.uint32))
    b.add_batch(*lay.arrays)
    got = b.finish()
    c = b.counters()
    b.close()
    assert c["sequences"] == 2 and c["windows"] == lay.windows.positions
    assert_same(got, ref)
