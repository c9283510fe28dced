"""GPU parity on planted groups: every integer edge of the matrix distance's pair-count kernels
(k_md_slot, the radix sort, k_md_rowstat / k_md_rowfill, k_md_rows in its u16, wide and multi-pass
forms, k_md_rows_seg, the gathers) hit on purpose.

tests/planted_matrix.py holds the catalogue and how a plan becomes residues and an exact-key DB;
tests/test_planted_matrix_cpu.py proves on the CPU that every input is what it claims to be, that
the oracle answers the hand-written expectations and which scenario holds which edge.  Here the
device must equal both, as sorted (id1, id2, count): exact integer equality, no tolerance.

Every handle is closed by a `with`, queries before their DB, also when a comparison fails (see
tests/test_gpu_hitset_edges.py: a query destroyed after its DB fails whichever test opens a DB
next)."""
from contextlib import closing

import numpy as np
import pytest

import planted_matrix as pm

pytestmark = pytest.mark.gpu

FI = pm.function_index()
EMPTY_BAND = (3000, 4000)  # no scenario run as row tiles has a sequence with an index in it


def _band(want, a, b):
    return want[(want[:, 0] >= a) & (want[:, 0] < b)]


def _check_counters(c, want, hits, groups):
    assert c["hits"] == hits and c["kmers"] == groups
    assert c["pairs"] == len(want) and c["increments"] == int(want[:, 2].astype(np.int64).sum())


@pytest.mark.parametrize("name", pm.NAMES)
def test_single_problem(skm, gpu, name):
    """MatrixDistance over the scenario's KeptKmerDb == the oracle == the expectation written from
    the plan; the counters are the plan's; a second run() on the same handle gives the same."""
    plan, mat = pm.single(name)
    want = pm.expect_array(name)
    np.testing.assert_array_equal(pm.oracle_array(name), want)
    hits, groups = pm.hits_groups(plan)
    res, off, lens, idx, n_idx = mat.problem(0)
    with closing(skm.KeptKmerDb(mat.keys, mat.data)) as db:
        with closing(skm.MatrixDistance(db, FI, res, off, lens, seq_idx=idx, n_idx=n_idx)) as md:
            got = md.compute()
            assert got.dtype == np.uint32 and got.shape == want.shape, (got.shape, want.shape)
            np.testing.assert_array_equal(got, want)
            _check_counters(md.counters(), want, hits, groups)
            np.testing.assert_array_equal(md.compute(), want)
            _check_counters(md.counters(), want, hits, groups)


@pytest.mark.parametrize("name", pm.BAND_NAMES)
def test_row_tiles(skm, gpu, name):
    """compute(rows=(a, b)): row 0 alone, row 5 alone, a band holding no sequence, the last row
    alone (in most scenarios it has hits and no entry), and three matrix_tile_rows bands whose
    concatenation is the full matrix."""
    plan, mat = pm.single(name)
    want = pm.expect_array(name)
    hits, groups = pm.hits_groups(plan)
    res, off, lens, idx, n_idx = mat.problem(0)
    used = {s.idx for s in plan.seqs}
    assert not any(EMPTY_BAND[0] <= i < EMPTY_BAND[1] for i in used) and 0 in used
    assert len(_band(want, 0, 1)) > 0 and len(_band(want, n_idx - 1, n_idx)) == 0
    with closing(skm.KeptKmerDb(mat.keys, mat.data)) as db:
        with closing(skm.MatrixDistance(db, FI, res, off, lens, seq_idx=idx, n_idx=n_idx)) as md:
            for a, b in ((0, 1), (5, 6), EMPTY_BAND, (n_idx - 1, n_idx)):
                got = md.compute(rows=(a, b))
                np.testing.assert_array_equal(got, _band(want, a, b), err_msg="rows [%d, %d)" % (a, b))
                _check_counters(md.counters(), _band(want, a, b), hits, groups)
            parts = []
            for r in range(3):
                a, b = skm.matrix_tile_rows(n_idx, r, 3)
                parts.append(md.compute(rows=(a, b)) if b > a else np.zeros((0, 3), np.uint32))
                np.testing.assert_array_equal(parts[-1], _band(want, a, b), err_msg="tile %d" % r)
            np.testing.assert_array_equal(np.concatenate(parts), want)
            np.testing.assert_array_equal(md.compute(), want)  # and the whole matrix after the tiles


@pytest.mark.parametrize("small_cols", [0, 1], ids=["seg_path", "rows_path"])
def test_batch_of_all_scenarios(skm, gpu, small_cols):
    """MatrixDistanceBatch with the scenarios as adjacent problems (local seq_idx, explicit
    prob_nidx), every far-column k-mer also planted at the next problem's index 0.  With the
    default small_cols the problems of at most 1,024 indices go through k_md_rows_seg, the
    65,536-entry rows included; with small_cols = 1 every problem of two or more indices goes
    through k_md_rows with rowsel / idx_prob / pbase, multi-pass rows ending at their problem's
    end."""
    mat = pm.batch()
    names = [p.name for p in mat.plans]
    want = [pm.expect_array(n) for n in names]
    hg = [pm.hits_groups(p) for p in mat.plans]
    nidx = [p.n_idx for p in mat.plans]
    limit = small_cols or pm.SEG_COLS
    with closing(skm.KeptKmerDb(mat.keys, mat.data)) as db:
        with closing(skm.MatrixDistanceBatch(db, FI, mat.flat, mat.seq_off, mat.seq_len, mat.prob_seq,
                                             seq_idx=mat.seq_idx, prob_nidx=mat.prob_nidx)) as mb:
            for _ in range(2):  # the handle is reusable
                got = mb.compute(small_cols=small_cols)
                assert len(got) == len(want)
                for n, g, w in zip(names, got, want):
                    assert g.dtype == np.uint32 and g.shape == w.shape, (n, g.shape, w.shape)
                    np.testing.assert_array_equal(g, w, err_msg=n)
                c = mb.counters()
                assert c["hits"] == sum(h for h, _ in hg) and c["groups"] == sum(g for _, g in hg)
                assert c["pairs"] == sum(len(w) for w in want)
                assert c["increments"] == sum(int(w[:, 2].astype(np.int64).sum()) for w in want)
                assert c["rows_small"] == sum(n for n in nidx if n <= limit)
                assert c["rows_large"] == sum(n for n in nidx if n > limit)
                np.testing.assert_array_equal(mb.group_counts(), np.array([g for _, g in hg], np.uint64))
                flat, poff = mb.pairs_flat()
                np.testing.assert_array_equal(poff, np.concatenate([[0], np.cumsum([len(w) for w in want])]))
                assert len(flat) == int(poff[-1])
    if small_cols == 1:
        assert sum(n <= limit for n in nidx) == 1  # only the one-index problem stays on the small path
