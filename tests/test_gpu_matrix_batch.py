"""GPU parity of the batched matrix distance (skm_matrix_batch_* / MatrixDistanceBatch): every
problem of a batch against the CPU oracle (oracle_matrix_distance) run on that problem alone,
bit-exact as sorted (id1, id2, count) with problem-local indices."""
import numpy as np
import pytest

import oracle_ref
from test_gpu_matrix import make_db, queries

pytestmark = pytest.mark.gpu

SEG_COLS = 1024  # built-in limit of the small-row kernel (k_md_rows_seg)
AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)


class Env:
    pass


@pytest.fixture(scope="module")
def env(skm, gpu, tmp_path_factory):
    """One small DB, its oracle handle and the ~300-problem batch of tests 1, 7 and 8."""
    e = Env()
    e.ref, e.funcs, e.base = make_db(skm, tmp_path_factory.mktemp("mdb"))
    e.bdz = oracle_ref.Bdz(open(e.base + ".mph", "rb").read())
    e.dat = open(e.base + ".dat", "rb").read()
    e.hypo = e.funcs.index("hypothetical protein")
    e.db = skm.CmphKmerDb(e.base)
    # queries grouped by family, so a problem (a contiguous cut) holds related sequences
    q = queries(6000)
    order = np.argsort(q.labels, kind="stable")
    e.seqs = [q.residues[int(q.seq_off[s]):int(q.seq_off[s]) + int(q.seq_len[s])].tobytes() for s in order]
    rng = np.random.default_rng(5)
    sizes = rng.integers(0, 41, size=300)
    sizes[:3] = [0, 40, 1]
    bounds = np.zeros(len(sizes) + 1, np.int64)
    bounds[1:] = np.cumsum(sizes)
    assert bounds[-1] <= len(e.seqs)
    e.problems = [e.seqs[bounds[p]:bounds[p + 1]] for p in range(len(sizes))]
    e.exp = [oracle(e, pr) for pr in e.problems]
    yield e
    e.db.close()


def pack(problems, idx=None):
    """problems: list of lists of bytes -> (residues, seq_off, seq_len, prob_seq)."""
    seqs = [s for pr in problems for s in pr]
    lens = np.array([len(s) for s in seqs], np.uint32)
    off = np.zeros(len(seqs), np.uint64)
    if len(seqs):
        off[1:] = np.cumsum(lens[:-1].astype(np.uint64))
    res = np.frombuffer(b"".join(seqs), np.uint8)
    prob_seq = np.zeros(len(problems) + 1, np.uint64)
    if problems:
        prob_seq[1:] = np.cumsum([len(pr) for pr in problems])
    return res, off, lens, prob_seq


def oracle(e, seqs, idx=None):
    if not seqs:
        return np.zeros((0, 3), np.uint32)
    res, off, lens, _ = pack([seqs])
    if idx is None:
        idx = np.arange(len(seqs), dtype=np.uint32)
    return oracle_ref.matrix_distance(e.bdz, e.dat, res, off, lens, idx, e.hypo)


def batch(skm, e, problems, db=None, **kw):
    res, off, lens, prob_seq = pack(problems)
    return skm.MatrixDistanceBatch(db or e.db, e.funcs, res, off, lens, prob_seq, **kw)


def check(got, exp):
    assert len(got) == len(exp)
    for p, (g, x) in enumerate(zip(got, exp)):
        assert g.dtype == np.uint32 and g.shape == x.shape, (p, g.shape, x.shape)
        np.testing.assert_array_equal(g, x, err_msg=f"problem {p}")


def noisy_copies(rng, sources, n, rate, core=None):
    """n copies of the sources in turn, each residue replaced at `rate`; with core=(a, b) only
    [a, b) is copied and the rest of the length is random residues (few DB hits, and the length
    still passes the matrix distance's length filter)."""
    out = []
    for i in range(n):
        src = sources[i % len(sources)]
        s = src.copy()
        m = rng.random(len(s)) < rate
        if core is not None:
            m[:core[0]] = True
            m[core[1]:] = True
        s[m] = AA[rng.integers(0, len(AA), int(m.sum()))]
        out.append(s.tobytes())
    return out


def test_batch_matches_per_problem_oracle(skm, env):
    mb = batch(skm, env, env.problems)
    got = mb.compute()
    check(got, env.exp)
    npairs = sum(len(x) for x in env.exp)
    assert npairs > 10000
    c = mb.counters()
    assert c["pairs"] == npairs
    assert c["increments"] == sum(int(x[:, 2].astype(np.int64).sum()) for x in env.exp)
    assert c["rows_small"] == sum(len(pr) for pr in env.problems) and c["rows_large"] == 0
    g = mb.group_counts()
    assert len(g) == len(env.problems) and int(g.sum()) == c["groups"] and g[0] == 0 and g[1] > 0
    check(mb.compute(), env.exp)  # the handle is reusable
    mb.close()


def test_shared_kmers_do_not_pair_across_problems(skm, env):
    fam = env.problems[1][:12]
    assert len(fam) == 12
    single = oracle(env, fam)
    assert len(single) > 0
    other = env.problems[200][:1] or env.problems[201][:1]
    with_extra = oracle(env, fam + other)
    mb = batch(skm, env, [fam, fam + other, fam])
    got = mb.compute()
    check(got, [single, with_extra, single])
    # the extra sequence is unrelated: problem 1 has the 12 sequences' pairs and nothing else
    np.testing.assert_array_equal(with_extra, single)
    assert mb.counters()["pairs"] == 3 * len(single)
    flat, off = mb.pairs_flat()
    assert list(off) == [0, len(single), 2 * len(single), 3 * len(single)] and len(flat) == 3 * len(single)
    mb.close()


def test_empty_and_degenerate_problems(skm, env):
    a, b = env.problems[1][:10], env.problems[3][:9]
    problems = [[], a, [], [], a[:1], [b"ACDEFGH", b"AC", b""], [b"XXXXXXXXXXXX", b"XXXXXXXXXXXXXXXX"], b, []]
    exp = [oracle(env, pr) for pr in problems]
    assert len(exp[1]) > 0 and all(len(exp[p]) == 0 for p in (0, 2, 3, 4, 5, 6, 8))
    mb = batch(skm, env, problems)
    check(mb.compute(), exp)
    _, off = mb.pairs_flat()
    n1 = len(exp[1])
    assert list(off[:8]) == [0, 0, n1, n1, n1, n1, n1, n1] and off[8] == off[9] == n1 + len(exp[7])
    mb.close()
    # P = 0
    z8, z64, z32 = np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32)
    mb = skm.MatrixDistanceBatch(env.db, env.funcs, z8, z64, z32, np.zeros(1, np.uint64))
    assert mb.compute() == []
    assert list(mb.pairs_flat()[1]) == [0]
    mb.close()
    # problems, but no sequences at all
    mb = skm.MatrixDistanceBatch(env.db, env.funcs, z8, z64, z32, np.zeros(4, np.uint64))
    got = mb.compute()
    assert len(got) == 3 and all(g.shape == (0, 3) for g in got)
    assert list(mb.pairs_flat()[1]) == [0, 0, 0, 0]
    mb.close()


def test_duplicate_ids_inside_a_problem(skm, env):
    base = env.problems[1][:30]
    src = base[0]
    seqs = base + [src, src, src.lower(), src * 5, b"*" + src + b"*"]
    # SeqIdMap: every 7th sequence repeats the id of the sequence 3 before it
    ids = skm.SeqIdMap()
    names = [f"fig|1.1.peg.{s}" for s in range(len(seqs))]
    for s in range(7, len(seqs), 7):
        names[s] = names[s - 3]
    idx = np.array([ids.lookup_id(nm) for nm in names], np.uint32)
    assert len(ids) < len(seqs)
    plain = env.problems[3][:11]
    problems = [plain, seqs, plain]
    res, off, lens, prob_seq = pack(problems)
    seq_idx = np.concatenate([np.arange(len(plain)), idx, np.arange(len(plain))]).astype(np.uint32)
    mb = skm.MatrixDistanceBatch(env.db, env.funcs, res, off, lens, prob_seq, seq_idx=seq_idx,
                                 prob_nidx=[len(plain), len(ids), len(plain)])
    exp = [oracle(env, plain), oracle(env, seqs, idx), oracle(env, plain)]
    assert len(exp[1]) > 0
    check(mb.compute(), exp)
    mb.close()


def test_path_boundary(skm, env):
    # small_cols = 8: problems of exactly 7, 8, 9 and 30 indices
    fam = env.problems[1]
    problems = [fam[:7], fam[:8], fam[:9], fam[:30]]
    exp = [oracle(env, pr) for pr in problems]
    assert all(len(x) > 0 for x in exp)
    mb = batch(skm, env, problems)
    check(mb.compute(small_cols=8), exp)
    c = mb.counters()
    assert c["rows_small"] == 15 and c["rows_large"] == 39
    check(mb.compute(), exp)  # and all four on the small path
    assert mb.counters()["rows_large"] == 0
    mb.close()
    # the built-in limit: SEG_COLS and SEG_COLS + 1 indices; noisy copies of a 40-residue stretch of
    # a few sources inside random residues of the source's length (shorter sequences would all
    # fail the length filter)
    rng = np.random.default_rng(11)
    sources = [np.frombuffer(s, np.uint8) for s in env.problems[1][:6]]
    big = [noisy_copies(rng, sources, SEG_COLS, 0.08, core=(40, 80)),
           noisy_copies(rng, sources, SEG_COLS + 1, 0.08, core=(40, 80))]
    exp = [oracle(env, pr) for pr in big]
    assert all(len(x) > 1000 for x in exp)
    mb = batch(skm, env, big)
    check(mb.compute(), exp)
    c = mb.counters()
    assert c["rows_small"] == SEG_COLS and c["rows_large"] == SEG_COLS + 1
    mb.close()


def test_row_longer_than_one_wave_sweep(skm, env):
    rng = np.random.default_rng(3)
    src = max(env.seqs, key=len)  # ~500 residues, ~200 windows that hit the DB
    seqs = [src] + noisy_copies(rng, [np.frombuffer(src, np.uint8)], 99, 0.05)
    exp = oracle(env, seqs)
    row0 = exp[exp[:, 0] == 0]
    assert len(row0) > 64           # more than 64 nonzero columns: several compaction steps
    assert int(row0[:, 2].max()) > 64  # one partner shares > 64 distinct k-mers: row 0 has > 64 entries
    mb = batch(skm, env, [env.problems[3][:5], seqs, env.problems[3][:5]])
    got = mb.compute()
    np.testing.assert_array_equal(got[1], exp)
    np.testing.assert_array_equal(got[0], got[2])
    mb.close()


def test_batch_exact_db(skm, env):
    """KeptKmerDB semantics (only real signature k-mers hit), against pyref per problem."""
    import pyref
    db = skm.KeptKmerDb(env.ref["keys"], env.ref["data"])
    keys = {int(k): tuple(int(x) for x in d) for k, d in zip(env.ref["keys"], env.ref["data"])}
    problems = [pr[:12] for pr in env.problems[:50]]
    mb = batch(skm, env, problems, db=db)
    got = mb.compute()
    total = 0
    for p, pr in enumerate(problems):
        exp = pyref.matrix_distance(pr, list(range(len(pr))), keys.get, env.hypo)
        assert {(int(a), int(b)): int(c) for a, b, c in got[p]} == exp, p
        total += len(exp)
    assert total > 500
    mb.close()
    db.close()


def test_batch_equals_loop(skm, env):
    mb = batch(skm, env, env.problems)
    got = mb.compute()
    mb.close()
    for p, pr in enumerate(env.problems):
        res, off, lens, _ = pack([pr])
        md = skm.MatrixDistance(env.db, env.funcs, res, off, lens)
        np.testing.assert_array_equal(md.compute(), got[p], err_msg=f"problem {p}")
        md.close()


def test_batch_argument_errors(skm, env):
    res, off, lens, prob_seq = pack([env.problems[1][:4]])
    with pytest.raises(skm.SkmError, match="Cannot find hypothetical protein index"):
        skm.MatrixDistanceBatch(env.db, ["a", "b"], res, off, lens, prob_seq)
    with pytest.raises(skm.SkmError, match="seq_idx out of range"):
        skm.MatrixDistanceBatch(env.db, env.funcs, res, off, lens, prob_seq, seq_idx=[0, 1, 2, 3], prob_nidx=[3])
    with pytest.raises(skm.SkmError):
        skm.MatrixDistanceBatch(env.db, env.funcs, res, off, lens, np.array([0, 3], np.uint64))
