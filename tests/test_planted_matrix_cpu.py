"""CPU proof of the planted-group catalogue (tests/planted_matrix.py): the inputs are what they claim
to be, the oracle (and, for the smaller ones, pyref.matrix_distance) answers the hand-written
expectations exactly, and the model of the kernels' path decisions confirms every claim.  The last
test prints each edge with the scenario that holds it.  The GPU side is
tests/test_gpu_matrix_edges.py."""
import numpy as np
import pytest

import planted_matrix as pm
import pyref

ROW_KEYS = ("entries", "ncol", "wide", "passes", "multi", "sweeps", "sweep_total", "steps", "nnz", "pass_kinds")
PROBLEM_KEYS = ("hits", "groups", "lg", "rounds", "total_entries")


def _dict(a):
    return {(int(x), int(y)): int(c) for x, y, c in a}


def test_mirrored_constants_equal_the_source():
    src = pm.source_constants()
    for name in pm.MIRRORED:
        assert src[name] == getattr(pm, name), name
    assert src["MR_BM"] == pm.MR_THREADS  # one bitmap word of 32 histogram words per compaction thread


@pytest.mark.parametrize("name", pm.NAMES)
def test_scenario_is_what_it_claims(name):
    plan, mat = pm.single(name)
    assert mat.planted_distinct() and mat.no_accidental_hits()
    assert np.array_equal(mat.keys, np.sort(mat.keys))
    # the expectation: derived from the member lists, written by hand, the oracle, pyref
    want = pm.pairs(plan)
    if plan.hand is not None:
        assert want == plan.hand
    ora = pm.oracle_array(name)
    assert _dict(ora) == want and len(ora) == len(want)
    np.testing.assert_array_equal(ora, pm.expect_array(name))
    # pyref scans a sequence in quadratic time: the smaller scenarios without very long sequences
    if mat.n_windows < 100000 and float((mat.seq_len.astype(np.float64) ** 2).sum()) < 5e7:
        recs = {int(k): tuple(int(x) for x in d) for k, d in zip(mat.keys, mat.data)}
        assert pyref.matrix_distance(mat.seqs_of(0), mat.seq_idx, recs.get, pm.HYPO) == want
    # hits and groups: counted from the residues against the DB, not from the plan
    m = pm.Model(plan)
    res, off, lens, idx, _ = mat.problem(0)
    hit_keys = []
    for o, n in zip(off, lens):
        w = pm.window_keys(res[int(o):int(o) + int(n)])
        hit_keys.append(w[np.isin(w, mat.keys)])
    hk = np.concatenate(hit_keys) if hit_keys else np.zeros(0, np.uint64)
    hypo = mat.keys[mat.data["function_index"] == pm.HYPO]
    hk = hk[~np.isin(hk, hypo)]
    assert len(hk) == m.hits and len(np.unique(hk)) == m.groups
    # the claims
    c = dict(plan.claims)
    row = c.pop("row", None)
    count = c.pop("count", None)
    for k, v in c.items():
        if k in PROBLEM_KEYS:
            assert getattr(m, k) == v, (name, k, getattr(m, k), v)
        else:
            assert k in ROW_KEYS and getattr(m.rows[row], k) == v, (name, row, k, getattr(m.rows[row], k), v)
    if count is not None:
        assert set(want.values()) == {count}
    # a row's nonzero columns in the model are the expectation's
    cols = {}
    for a, b in want:
        cols.setdefault(a, set()).add(b - a - 1)
    for r, R in m.rows.items():
        assert cols.get(r, set()) == R.columns, (name, r)
    assert set(cols) <= set(m.rows)


def test_batch_is_the_catalogue_with_strangers():
    """The batch's problems pair exactly as the single scenarios do, although every far-column
    k-mer also sits at the next problem's index 0; the oracle on each problem of the batch's own
    residues agrees."""
    mat = pm.batch()
    assert mat.planted_distinct() and mat.no_accidental_hits()
    n_far = 0
    for p, plan in enumerate(mat.plans):
        assert pm.pairs(plan) == pm.pairs(pm.single(plan.name)[0]), plan.name
        np.testing.assert_array_equal(mat.oracle(p), pm.expect_array(plan.name), err_msg=plan.name)
        if p and mat.plans[p - 1].far:
            prev = mat.plans[p - 1]
            for k, kid in enumerate(prev.far):
                s = plan.seqs[k]
                assert s.idx == 0 and s.kmers == [prev.key(kid)]
                n_far += 1
            # the stranger k-mers are hits and groups of this problem, and entries of no row
            assert pm.Model(plan).hits == pm.Model(pm.single(plan.name)[0]).hits + len(prev.far)
            assert pm.Model(plan).total_entries == pm.Model(pm.single(plan.name)[0]).total_entries
    assert n_far == sum(len(p.far) for p in mat.plans) == 12
    # both paths: with the default small_cols the wide rows go through k_md_rows_seg
    by = {p.name: p for p in mat.plans}
    assert by["dense3_65536"].n_idx <= pm.SEG_COLS and by["prob_1024"].n_idx == pm.SEG_COLS
    assert by["colpass"].n_idx > pm.SEG_COLS and by["wide_2pass"].n_idx > pm.SEG_COLS


def test_every_edge_has_an_input(capsys):
    """Each edge the GPU tests are meant to hit, with the scenarios that hold it."""
    rows = []  # (scenario, row, Row, Model)
    for name in pm.NAMES:
        plan, _ = pm.single(name)
        m = pm.Model(plan)
        rows += [(name, r, R, m) for r, R in m.rows.items()]
    models = {name: pm.Model(pm.single(name)[0]) for name in pm.NAMES}
    counts = {name: set(pm.pairs(pm.single(name)[0]).values()) for name in pm.NAMES}

    def holders(pred):
        return sorted({n for n, r, R, m in rows if pred(R)})

    edges = [("wide", lambda R: R.wide),
             ("2+ passes, non-wide", lambda R: R.passes >= 2 and not R.wide),
             ("2 passes, wide", lambda R: R.passes == 2 and R.wide),
             ("a last pass of one column", lambda R: R.multi and R.ncol % R.cpp == 1),
             ("entries with no column (ncol 0)", lambda R: R.ncol == 0),
             ("an entry and nnz 0", lambda R: R.nnz == 0),
             ("partners in pass 0 only, pass 1 only and both, in one row",
              lambda R: {(0,), (1,)} <= R.pass_kinds and any(len(k) > 1 for k in R.pass_kinds))]
    edges += [("ncol %d" % v, lambda R, v=v: R.ncol == v) for v in (65536, 65537)]
    edges += [("%d entries" % v, lambda R, v=v: R.entries == v) for v in (63, 64, 65, 129, 1023, 1024, 1025, 2049,
                                                                        65535, 65536)]
    edges += [("sweep total %d" % v, lambda R, v=v: R.sweep_total == v) for v in (4095, 4096, 4097)]
    edges += [("one sweep, %d partners" % v, lambda R, v=v: R.sweep_total == v) for v in (1, 2, 63, 64, 1023, 1024)]
    lines = []
    for what, pred in edges:
        h = holders(pred)
        lines.append("%-60s %s" % (what, ", ".join(h)))
        assert h, what
    for v in (65535, 65536):
        h = sorted(n for n in pm.NAMES if v in counts[n])
        lines.append("%-60s %s" % ("count %d" % v, ", ".join(h)))
        assert h
    for v in (1, 2, 3, 4, 5):
        h = sorted(n for n in pm.NAMES if models[n].rounds == v)
        lines.append("%-60s %s" % ("radix rounds %d" % v, ", ".join(h)))
        assert h
    for v in (2, 255, 256, 257, 4095, 4096, 4097, 8193):
        h = sorted(n for n in pm.NAMES if models[n].hits == v)
        lines.append("%-60s %s" % ("%d surviving hits" % v, ", ".join(h)))
        assert h
    # compaction words: row 0 of the u16 groups has columns 63 | 64 and 65471 | 65472 (threads 0 | 1 and
    # 1022 | 1023), row 0 of the wide row columns 31 | 32
    g = models["group_1025"].rows[0]
    assert {63, 64, 65471, 65472, 65535} <= g.columns and not g.wide
    w = models["wide_2pass"].rows[0]
    assert {31, 32, 32767, 32768} <= w.columns and w.wide and w.cpp == 32768
    with capsys.disabled():
        print("\n" + "\n".join(lines))
