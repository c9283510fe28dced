"""CPU proof of the planted-hit catalogue (tests/planted_hits.py): the inputs are what they claim to
be, the reference answers what each scenario's hand-written expectation says, and the Python
restatement of HitSet (pyref.hitset_calls) equals the C++ oracle bit for bit on all of it.  The GPU
side is tests/test_gpu_hitset_edges.py."""
import numpy as np
import pytest

import oracle_ref
import planted_hits as ph
import pyref

MG = sorted({(o[0], o[1]) for o in ph.OPTION_SETS})
MAD0 = [o for o in ph.OPTION_SETS if o[4] == 0]


def _ids(opts):
    return [ph.opt_id(o) for o in opts]


def _calls_array(calls):
    a = np.zeros(len(calls), oracle_ref.CALL_DTYPE)
    for k, (start, end, count, func, median, mad) in enumerate(calls):
        a[k] = (start, end, count, func, 0, median, mad)
    return a


def _seq_calls(opt, s):
    off, calls = ph.oracle_calls(opt)
    return calls[int(off[s]):int(off[s + 1])]


@pytest.mark.parametrize("m,g", MG, ids=["m%d-g%d" % x for x in MG])
def test_catalogue_is_what_it_claims(m, g):
    b = ph.batch_for(m, g)
    sc = b.scens
    assert b.distinct()
    assert len(sc) >= ph.MIN_SEQS and b.n_windows < 100000
    assert sum(s.kind == "fill" for s in sc) > len(sc) // 2
    # every nwin at every pstart & 3, pstart the running sum of len + 1
    pstart = np.concatenate([[0], np.cumsum(b.seq_len.astype(np.int64) + 1)[:-1]])
    np.testing.assert_array_equal(pstart, b.pstart.astype(np.int64))
    seen = {(s.nwin, int(pstart[i]) & 3) for i, s in enumerate(sc) if s.name.startswith("tile_n")}
    assert seen == {(n, mis) for n in ph.TILE_NWIN for mis in range(4)}
    assert {s.length for s in sc if s.kind == "fill"} == {0, 1, 7, 8}
    # call makers on both sides of every block and tile boundary
    for bd in ph.STRADDLES:
        assert sc[bd - 1].name == "straddle_%d_lo" % bd and sc[bd].name == "straddle_%d_hi" % bd
        assert sc[bd - 1].dense and sc[bd].dense and sc[bd].nwin == 20
    # the slot sequences: in the middle between call makers, and that of min_hits as the very last
    assert sc[-1].name == "slots_m%d" % m
    mid = [i for i, s in enumerate(sc) if s.kind == "slots"][:len(ph.SLOT_M)]
    assert [sc[i].claims["runs"] for i in mid] == list(ph.SLOT_M)
    for i in mid:
        assert sc[i - 1].kind == "tile" and sc[i + 1].kind == "tile" and sc[i - 1].nwin == sc[i + 1].nwin == 20
        assert sc[i].dense and sc[i].nwin == ph.SLOT_NWIN
    # the segment scenarios: n, span and R recomputed from the hits
    for s in sc:
        if s.kind != "seg":
            continue
        own = [h for h in s.hits if h[1] == "A"]
        c = s.claims
        if "n" in c:
            assert len(own) == c["n"], s.name
        if "span" in c:
            assert s.hits[-1][0] - s.hits[0][0] + 1 == c["span"], s.name
        if "R" in c:
            assert max(h[2] for h in own) - min(h[2] for h in own) + 1 == c["R"], s.name
        if "c2" in c:
            v = sorted(h[2] for h in own)
            assert v[len(v) // 2 - 1] + v[len(v) // 2] == c["c2"], s.name
        if "ns" in c:
            assert tuple(sum(h[1] == f for h in s.hits) for f in ("A", ("S", 3), ("S", 4))) == c["ns"]
    names = {s.name: s for s in sc}
    assert {names["seg_n%d" % n].claims["n"] for n in ph.LDS_N} == set(ph.LDS_N)
    assert names["seg_R65536_n6"].claims["R"] == 65536
    assert {0, 65535} <= {h[2] for h in names["seg_R65536_n6"].hits}
    assert names["seg_strangers_lds"].claims["n"] <= ph.SEG_CAP < names["seg_strangers_seq"].claims["n"]
    assert all(names["seg_span%d" % x].claims["n"] < ph.SEG_CAP for x in (1024, 1025, 1088, 1089))
    assert names["seg_third_n1024"].claims["n"] == ph.SEG_CAP and names["seg_third_n1024"].claims["span"] > ph.SEG_CAP


@pytest.mark.parametrize("opt", MAD0, ids=_ids(MAD0))
def test_pyref_hitset_equals_oracle(opt):
    """pyref.hitset_calls == oracle_annotate_exact on the whole catalogue, field for field, the
    MAD's float bits included."""
    b = ph.batch_for(opt[0], opt[1])
    off, calls = ph.oracle_calls(opt)
    total = 0
    for s, sc in enumerate(b.scens):
        want = calls[int(off[s]):int(off[s + 1])]
        if not sc.hits:
            assert len(want) == 0, sc.name
            continue
        got = _calls_array(pyref.hitset_calls(sc.length, b.hits_of(s), opt[0], opt[1], opt[2], ph.HYPO, opt[3]))
        assert got.tobytes() == want.tobytes(), (s, sc.name, got[:4], want[:4])
        total += len(got)
    assert total == len(calls) and (total > 300 or opt[1] == 0)


@pytest.mark.parametrize("opt", ph.OPTION_SETS, ids=_ids(ph.OPTION_SETS))
def test_reference_answers_the_expectations(opt):
    """The oracle's calls against what each scenario states by hand: the state machine's exact
    (start, end, count, function), the 600 // m calls of the slot sequences, and (with the default
    statistics) the call every statistics scenario must make so that its median and MAD are seen."""
    m, g, ignore, mean_mode, mad_mode = opt
    b = ph.batch_for(m, g)
    n_sm = 0
    for s, sc in enumerate(b.scens):
        got = _seq_calls(opt, s)
        if sc.kind == "slots":
            if g >= 1 and sc.claims["runs"] == m:
                assert len(got) == ph.SLOT_NWIN // m, sc.name
                assert (got["count"] == m).all()
            continue
        if sc.expect is None or (sc.kind == "seg" and (mean_mode or mad_mode)):
            continue
        want = sc.expect(m, g, ignore)
        if want is None:
            continue
        if isinstance(want, int):
            assert len(got) == want, (sc.name, got)
            own = sc.claims.get("n")
            if want == 1 and own is not None:
                assert got["count"][0] == own, sc.name
                if "mad" in sc.claims:
                    assert got["protein_length_med_avg_dev"][0] == np.float32(sc.claims["mad"]), sc.name
                if "end" in sc.claims:
                    assert got["end"][0] == sc.claims["end"], sc.name
            continue
        have = [(int(c["start"]), int(c["end"]), int(c["count"]), int(c["function_index"])) for c in got]
        assert have == [(a, e, c, ph.resolve(f, s)) for a, e, c, f in want], (sc.name, have, want)
        n_sm += sc.kind == "sm"
    assert n_sm == 15


def test_whole_sequence_ends_on_the_last_residue():
    b = ph.batch_for(5, 200)
    s = next(i for i, x in enumerate(b.scens) if x.name == "sm_whole_sequence")
    c = _seq_calls((5, 200, 0, 0, 0), s)
    assert len(c) == 1 and c["start"][0] == 0 and c["end"][0] == b.scens[s].length - 1


def test_every_third_window_chains_at_gap_3_only():
    b = ph.batch_for(4, 3)
    for name, n in (("seg_third_n1034", 1034), ("seg_third_n1024", 1024)):
        s = next(i for i, x in enumerate(b.scens) if x.name == name)
        c3 = pyref.hitset_calls(b.scens[s].length, b.hits_of(s), 4, 3, 0, ph.HYPO, 0)
        assert [c[2] for c in c3] == [n]
        assert pyref.hitset_calls(b.scens[s].length, b.hits_of(s), 4, 2, 0, ph.HYPO, 0) == []
        assert len(_seq_calls((4, 3, 0, 0, 0), s)) == 1


@pytest.mark.parametrize("opt", [o for o in ph.OPTION_SETS if o[1] >= 1],
                         ids=_ids([o for o in ph.OPTION_SETS if o[1] >= 1]))
def test_calls_on_both_sides_of_the_boundaries(opt):
    off, _ = ph.oracle_calls(opt)
    cnt = np.diff(off.astype(np.int64))
    for bd in ph.STRADDLES:
        assert cnt[bd - 1] == 1 and cnt[bd] == 1
    assert cnt[-1] >= 1  # the last sequence makes calls: its slots end the allocation


@pytest.mark.parametrize("m,nwin", [(2, 9), (3, 9), (4, 8)])
def test_runs_of_min_hits_are_the_densest(m, nwin):
    """Every pattern of {no hit, A, B} over nwin windows: no sequence makes more calls than runs of
    exactly min_hits of alternating functions do (nwin // m, what the slot sequences plant), and
    that stays within the slot range k_caps gives a sequence."""
    import itertools
    cap = nwin // (m - 2) + 2 if m > 2 else 2 * nwin + 2
    best = 0
    for pat in itertools.product((0, 1, 2), repeat=nwin):
        hits = [(i, f, nwin + 7) for i, f in enumerate(pat) if f]
        if len(hits) >= m:
            best = max(best, len(pyref.hitset_calls(nwin + 7, hits, m, 200, 0, ph.HYPO, 0)))
    assert best == nwin // m and best <= cap


def test_hitset_small_hand_cases():
    """pyref.hitset_calls on cases small enough to follow by eye."""
    hits = [(0, 1, 100), (1, 1, 100), (2, 2, 100), (3, 1, 100), (4, 3, 100), (5, 1, 100)]  # A A B A C A
    assert pyref.hitset_calls(100, hits, 5, 200, 0, 9, 0) == []
    got = pyref.hitset_calls(100, hits, 4, 200, 0, 9, 0)
    assert got == [(0, 12, 4, 1, 100, np.float32(30))]
    # means 1, 2, 3, 10: median 2.5, |x - 2.5| = 1.5 .5 .5 7.5 -> MAD 1.0, mean 4 inside 4 -/+ 2
    got = pyref.hitset_calls(4, [(k, 1, v) for k, v in enumerate((1, 2, 3, 10))], 2, 200, 0, 9, 0)
    assert got == [(0, 10, 4, 1, 2, np.float32(1.0))]


# ---- the matrix distance's length filter -------------------------------------------------------

def test_matrix_length_filter_boundaries():
    """pyref.matrix_distance == the oracle over the exact DB on the planted length boundaries, and
    both give the hand-written pairs where var != 0."""
    mb = ph.MatrixBatch()
    assert mb.distinct()
    recs = {int(k): tuple(int(x) for x in d) for k, d in zip(mb.keys, mb.data)}
    idx = list(range(len(mb.seqs)))
    exp = pyref.matrix_distance(mb.seqs, idx, recs.get, ph.HYPO)
    got = oracle_ref.matrix_distance_exact(mb.keys, mb.data, mb.residues, mb.seq_off, mb.seq_len, idx, ph.HYPO)
    assert {(int(a), int(c)): int(n) for a, c, n in got} == exp
    hand = mb.expected_by_hand()
    by_hand = {i for i in idx if mb.kept[i] is not None}
    assert {p: n for p, n in exp.items() if p[0] in by_hand} == hand and len(hand) == 21
    # var == 0: every case keeps some sequences and drops some
    for c, case in enumerate(mb.cases):
        if case[2]:
            continue
        ids = [i for i in idx if mb.case_of[i] == c]
        kept = {i for p in exp for i in p if i in ids}
        assert 2 <= len(kept) < len(ids), case[0]
