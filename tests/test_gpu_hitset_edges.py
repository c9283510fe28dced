"""GPU parity on planted hits: every integer edge of the HitSet call path (k_lookup at sequence
boundaries, k_caps, k_calls_scan, the scans, k_seg_process) hit on purpose.

tests/planted_hits.py holds the catalogue and how a scenario becomes residues and an exact-key DB;
tests/test_planted_hits_cpu.py proves on the CPU that every input is what it claims to be and that
the oracle answers the hand-written expectations.  Here the device must equal the oracle on the
whole catalogue, for every option set: call_off equal and the calls byte for byte, no tolerance.

min_hits = 1 is out of scope: with a single hit the reference's HitSet::process reads end[1]
before the beginning of its vector (call_functions.tcc:88-91), so it defines no answer.

Every handle is closed by a `with`, queries before their DB, also when a comparison fails:
skm_query_destroy reads its DB's device, so a query left to the garbage collector may be destroyed
after its DB, and the HIP error of that call fails whichever test opens a DB next."""
from contextlib import closing

import numpy as np
import pytest

import oracle_ref
import planted_hits as ph
import pyref

pytestmark = pytest.mark.gpu

FI = ph.function_index()
MG = sorted({(o[0], o[1]) for o in ph.OPTION_SETS})


def _caller(skm, db, opt):
    c = skm.FunctionCaller(db, FI, min_hits=opt[0], max_gap=opt[1], mean_mode=opt[3], mad_mode=opt[4])
    c.ignore_hypothetical(bool(opt[2]))
    assert c.hypo_index == ph.HYPO
    return c


def _same(scens, got, want, what):
    goff, gcalls = got
    ooff, ocalls = want
    if not np.array_equal(goff, ooff) or gcalls.tobytes() != ocalls.tobytes():
        assert len(goff) == len(ooff), what
        pytest.fail("%s: %s" % (what, ph.first_difference(scens, goff, gcalls, ooff, ocalls)))


@pytest.mark.parametrize("opt", ph.OPTION_SETS, ids=[ph.opt_id(o) for o in ph.OPTION_SETS])
def test_calls_match_oracle(skm, gpu, opt):
    """FunctionCaller.process_seqs over the KeptKmerDb == oracle_annotate_exact on the whole
    catalogue; then the same batch in the packed layout (seq_off[s] = sum of len + 1, uploaded as
    it is), where every gap byte would complete a DB key of its sequence if it were a residue."""
    b = ph.batch_for(opt[0], opt[1])
    want = ph.oracle_calls(opt)
    with closing(skm.KeptKmerDb(b.keys, b.data)) as db:
        caller = _caller(skm, db, opt)
        _same(b.scens, caller.process_seqs(b.residues, b.seq_off, b.seq_len), want, "sequences back to back")
        _same(b.scens, caller.process_seqs(b.p_residues, b.p_seq_off, b.seq_len), want, "packed layout")


@pytest.mark.parametrize("m,g", MG, ids=["m%d-g%d" % x for x in MG])
def test_window_hits_are_the_planted_hits(skm, gpu, m, g):
    """k_lookup at every sequence boundary: QueryBatch.window_hits() is exactly the planted
    (position, function_index << 16 | mean) lists, in both layouts (the trap keys of the gap bytes
    never hit); QueryBatch.run's own min_hits / max_gap give the oracle's calls."""
    b = ph.batch_for(m, g)
    with closing(skm.KeptKmerDb(b.keys, b.data)) as db:
        for res, off in ((b.residues, b.seq_off), (b.p_residues, b.p_seq_off)):
            with closing(skm.QueryBatch(db, res, off, b.seq_len)) as qb:
                qb.run(hypo_index=ph.HYPO, min_hits=m, max_gap=g)
                hoff, pos, fm = qb.window_hits()
                np.testing.assert_array_equal(hoff, b.hit_off)
                np.testing.assert_array_equal(pos, b.hit_pos)
                np.testing.assert_array_equal(fm, b.hit_fm)
                _same(b.scens, qb.calls(), ph.oracle_calls((m, g, 0, 0, 0)), "QueryBatch")


def test_reused_query_object(skm, gpu):
    """The DB's own query object, reused by skm_annotate: the whole catalogue, then only the tiny
    load-tiling sequences, then the catalogue again.  Nothing of one batch may reach the next."""
    opt = (5, 200, 0, 0, 0)
    b = ph.batch_for(5, 200)
    want = ph.oracle_calls(opt)
    idx = [i for i, s in enumerate(b.scens) if s.kind in ("fill", "tile", "straddle")]
    res, off, lens = b.subset(idx)
    twant = oracle_ref.annotate_exact(b.keys, b.data, res, off, lens, **ph.oracle_opts(opt))
    assert len(twant[1]) > 40
    with closing(skm.KeptKmerDb(b.keys, b.data)) as db:
        caller = _caller(skm, db, opt)
        first = caller.process_seqs(b.residues, b.seq_off, b.seq_len)
        _same(b.scens, first, want, "first run")
        tiny = caller.process_seqs(res, off, lens)
        _same([b.scens[i] for i in idx], tiny, twant, "tiny batch after the catalogue")
        third = caller.process_seqs(b.residues, b.seq_off, b.seq_len)
        _same(b.scens, third, first, "catalogue after the tiny batch")


@pytest.mark.parametrize("opt", [(5, 200, 0, 0, 0), (2, 200, 0, 0, 1), (6, 200, 0, 1, 0), (3, 7, 0, 0, 0)],
                         ids=lambda o: ph.opt_id(o))
def test_dense_subset_over_bdz(skm, gpu, tmp_path, opt):
    """The scenarios in which every window is planted (load tiling, segment slots, the dense
    statistics ones), over a BDZ DB built from their keys (k_lookup<LK_BDZ7>) against the oracle's
    BDZ restatement."""
    b = ph.batch_for(opt[0], opt[1])
    idx = [i for i, s in enumerate(b.scens) if s.dense]
    assert {"tile", "slots", "seg", "fill", "straddle"} <= {b.scens[i].kind for i in idx}
    sel = np.concatenate([np.arange(int(b.hit_off[i]), int(b.hit_off[i + 1])) for i in idx])
    sel = sel[np.argsort(b.planted_keys[sel])]
    keys = b.planted_keys[sel]
    data = np.zeros(len(keys), skm.STORED_DTYPE)
    data["function_index"] = b.hit_fm[sel] >> 16
    data["mean"] = b.hit_fm[sel] & 0xFFFF
    base = str(tmp_path / "kmer_data")
    skm.mph_build(keys, data, base + ".mph", base + ".dat", seed=7)
    res, off, lens = b.subset(idx)
    with closing(skm.CmphKmerDb(base)) as db:
        got = _caller(skm, db, opt).process_seqs(res, off, lens)
    ob = oracle_ref.Bdz(open(base + ".mph", "rb").read())
    want = oracle_ref.annotate(ob, open(base + ".dat", "rb").read(), res, off, lens, **ph.oracle_opts(opt))
    assert len(want[1]) > 100
    _same([b.scens[i] for i in idx], got, want, "dense subset over BDZ")
    # every window is a member: the BDZ answer is the exact DB's
    o2, c2 = ph.oracle_calls(opt)
    exact = np.concatenate([c2[int(o2[i]):int(o2[i + 1])] for i in idx])
    assert exact.tobytes() == want[1].tobytes()


def test_matrix_length_filter_boundaries(skm, gpu):
    """k_md_hits' length filter ((len - mean)^2 <= 4 var in integers, the reference's doubles when
    var == 0) on the planted boundaries: MatrixDistance over the exact DB == pyref == the oracle."""
    mb = ph.MatrixBatch()
    with closing(skm.KeptKmerDb(mb.keys, mb.data)) as db:
        with closing(skm.MatrixDistance(db, FI, mb.residues, mb.seq_off, mb.seq_len)) as md:
            got = {(int(a), int(c)): int(n) for a, c, n in md.compute()}
    idx = list(range(len(mb.seqs)))
    recs = {int(k): tuple(int(x) for x in d) for k, d in zip(mb.keys, mb.data)}
    assert got == pyref.matrix_distance(mb.seqs, idx, recs.get, ph.HYPO)
    ora = oracle_ref.matrix_distance_exact(mb.keys, mb.data, mb.residues, mb.seq_off, mb.seq_len, idx, ph.HYPO)
    assert got == {(int(a), int(c)): int(n) for a, c, n in ora}
    hand = mb.expected_by_hand()
    assert {p: n for p, n in got.items() if mb.kept[p[0]] is not None} == hand
