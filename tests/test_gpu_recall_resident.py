"""GPU tests of the recall pass over a build's resident sequences (skm_build_recall,
SignatureBuilder.recall): parity with the uploaded path for every kind of DB, the batch
boundaries, every alignment of a batch's view, skipped sequences, the release levels, the
refusals and the empty build."""
import numpy as np
import pytest

import oracle_ref
from signature_kmers_amd import synth

pytestmark = pytest.mark.gpu

UNDEF = 0xFFFF


def pack(seqs):
    lens = np.array([len(s) for s in seqs], np.uint32)
    off = np.zeros(len(seqs), np.uint64)
    off[1:] = np.cumsum(lens[:-1])
    return np.frombuffer(b"".join(seqs), np.uint8), off, lens


def builder_of(skm, inputs, n_functions):
    b = skm.SignatureBuilder(n_functions, device=0)
    b.add_batch(*inputs)
    return b


def same_best(got, want, msg=""):
    assert got.dtype == want.dtype and len(got) == len(want), msg
    np.testing.assert_array_equal(got.view(np.uint8), want.view(np.uint8), err_msg=msg)


def same_calls(got, want, msg=""):
    np.testing.assert_array_equal(got[-2], want[0], err_msg=msg)
    np.testing.assert_array_equal(got[-1].view(np.uint8), want[1].view(np.uint8), err_msg=msg)


@pytest.fixture(scope="module")
def base(skm, gpu):
    """The 2000-sequence build of test_gpu_kept_db.py, its three DBs, and for each of them the
    uploaded path's best calls over the build's own proteins (computed once, never changed)."""
    p = synth.generate_arrays(2000, 50, per_file=500, seed=5)
    r, o, l, f, i, funcs = synth.build_inputs(p)
    inputs = (r, o, l, f, i)
    b = builder_of(skm, inputs, len(funcs))
    kept = b.finish()
    dbs = {"kept_db": b.kept_db(), "host_exact": skm.KeptKmerDb(kept.keys, kept.data), "mph_db": b.mph_db()}
    hypo = funcs.index("hypothetical protein")
    tables = skm.FunctionIndexTables(funcs, device=0)
    own = (p.residues, p.seq_off, p.seq_len)
    want_best = {k: skm.FunctionCaller(d, funcs).best_seqs(*own).best.copy() for k, d in dbs.items()}
    d = dict(p=p, inputs=inputs, funcs=funcs, builder=b, kept=kept, dbs=dbs, hypo=hypo, tables=tables, own=own,
             want_best=want_best)
    yield d
    for x in dbs.values():
        x.close()
    tables.close()
    b.close()


# ---- 1. parity ----
@pytest.mark.parametrize("kind", ["kept_db", "host_exact", "mph_db"])
def test_parity_best_and_calls(skm, base, kind):
    b, db = base["builder"], base["dbs"][kind]
    assert b.resident_seqs() == (2000, int(base["p"].seq_len.astype(np.int64).sum()) + 2000)
    got = b.recall(db, base["tables"])
    same_best(got.best, base["want_best"][kind], kind)
    assert (got.best["fi"] != UNDEF).sum() > 1000  # the pass finds its own training proteins
    st = got.stats
    assert st["n_seqs"] == 2000 and st["n_batches"] == 1 and st["resident_bytes"] == b.resident_seqs()[1]
    assert st["n_windows"] == int(np.maximum(base["p"].seq_len.astype(np.int64) - 7, 0).sum())
    if kind == "mph_db":
        want = skm.FunctionCaller(db, base["funcs"]).process_seqs(*base["own"])
    else:
        want = oracle_ref.annotate_exact(base["kept"].keys, base["kept"].data, *base["own"], hypo_index=base["hypo"])
    calls = b.recall(db, want_calls=True, hypo_index=base["hypo"])
    same_calls(calls, want, kind)
    assert calls.stats["n_calls"] == len(want[1]) > 0
    both = b.recall(db, base["tables"], want_calls=True)
    same_best(both[0].best, base["want_best"][kind], kind)
    same_calls(both, want, kind)


# ---- 2. batch boundaries ----
@pytest.mark.parametrize("batch", [1, 17, 4096, 0])
def test_batch_boundaries(skm, base, batch):
    b, db = base["builder"], base["dbs"]["kept_db"]
    plan = skm.recall_plan(base["p"].seq_len, batch)
    got = b.recall(db, base["tables"], want_calls=True, batch_residues=batch)
    assert got.stats["n_batches"] == len(plan)
    assert len(plan) == {1: 2000, 17: 2000, 0: 1}.get(batch, len(plan)) and len(plan) >= 1
    same_best(got[0].best, base["want_best"]["kept_db"], str(batch))
    want = oracle_ref.annotate_exact(base["kept"].keys, base["kept"].data, *base["own"], hypo_index=base["hypo"])
    same_calls(got, want, str(batch))


# ---- 3. alignment and edges: a planted build recalled against the base DB ----
def planted_seqs(p):
    """A few dozen sequences cut from the base proteins (the base DB hits them): lengths 0, 7, 8, 9,
    the 16-window tile edges 23, 24, 25, 'X' / '*' at a window's start, end and inside, and lengths
    that walk the packed start through all 16 residues mod 16."""
    def src(k, n, at=0):
        s = p.residues[p.seq_off[k]:p.seq_off[k] + p.seq_len[k]].tobytes()
        assert len(s) >= at + n
        return s[at:at + n]

    seqs = [src(0, 60), b"", src(1, 7), src(2, 8), src(3, 9), src(4, 23), src(5, 24), src(6, 25), b"", b"",
            b"X" + src(7, 40), src(8, 40) + b"*", src(9, 20) + b"X" + src(9, 30, 21), src(10, 7) + b"*" + src(10, 50, 8),
            src(11, 8) + b"X" + src(11, 40, 9), b"*" * 20]
    # whole proteins less a few residues at either end (these carry calls): each tail is trimmed so
    # that the next sequence starts at a residue mod 16 that no sequence has started at yet
    def starts(ss):
        at, out = 0, set()
        for x in ss:
            out.add(at % 16)
            at += len(x) + 1
        return out, at

    for j in range(20):
        k = 20 + j
        whole = src(k, int(p.seq_len[k]) - j, j)
        seen, at = starts(seqs)
        trim = next((t for t in range(16) if (at + len(whole) - t + 1) % 16 not in seen | {at % 16}), 0)
        seqs.append(whole[:len(whole) - trim])
    seqs.append(src(50, 72))  # the last resident sequence: its view ends at the buffer's padding
    return seqs


@pytest.fixture(scope="module")
def planted(skm, base):
    seqs = planted_seqs(base["p"])
    r, o, l = pack(seqs)
    func = (np.arange(len(seqs)) % len(base["funcs"])).astype(np.uint16)
    b = skm.SignatureBuilder(len(base["funcs"]), device=0)
    b.add_batch(r, o, l, func, np.arange(len(seqs), dtype=np.uint32))
    b.prepare()
    db = base["dbs"]["kept_db"]
    caller = skm.FunctionCaller(db, base["funcs"])
    want = caller.best_seqs(r, o, l).best.copy()
    yield dict(builder=b, seqs=seqs, lens=l, want=want, db=db, call_off=caller.process_seqs(r, o, l)[0])
    b.close()


def test_planted_layout_covers_every_alignment(skm, planted):
    l = planted["lens"]
    pstart = np.concatenate([[0], np.cumsum(l.astype(np.int64) + 1)])[:-1]
    assert set((pstart % 16).tolist()) == set(range(16))
    assert {0, 7, 8, 9, 23, 24, 25} <= set(l.tolist())
    plan = skm.recall_plan(l, 1)
    assert len(plan) == len(l) and {b["pstart"] - b["base"] for b in plan} == set(range(16))
    # the base DB does hit them: the oracle finds calls in 19 of the 20 whole proteins untrimmed
    assert (np.diff(planted["call_off"].astype(np.int64)) > 0).sum() >= 15
    assert (planted["want"]["fi"] != UNDEF).sum() >= 1


def test_planted_one_sequence_per_batch(skm, base, planted):
    b = planted["builder"]
    for batch in (1, 0):
        got = b.recall(planted["db"], base["tables"], batch_residues=batch)
        same_best(got.best, planted["want"], str(batch))
    assert b.recall(planted["db"], base["tables"], batch_residues=1).stats["n_batches"] == len(planted["seqs"])


@pytest.mark.parametrize("count", [1, 3])
def test_planted_every_first_seq(skm, base, planted, count):
    b, n = planted["builder"], len(planted["seqs"])
    for first in range(n - count + 1):
        got = b.recall(planted["db"], base["tables"], first_seq=first, n_seqs=count)
        assert got.stats["n_seqs"] == count
        same_best(got.best, planted["want"][first:first + count], f"first_seq {first}")
    # the last sequence alone, and "to the end"
    same_best(b.recall(planted["db"], base["tables"], first_seq=n - 1).best, planted["want"][n - 1:])
    assert len(b.recall(planted["db"], base["tables"], first_seq=n).best) == 0
    with pytest.raises(skm.SkmError, match="error -1"):
        b.recall(planted["db"], base["tables"], first_seq=n + 1)
    with pytest.raises(skm.SkmError, match="error -1"):
        b.recall(planted["db"], base["tables"], first_seq=n - 1, n_seqs=2)


# ---- 4. skipped sequences, several add_batch calls ----
def test_skipped_sequences_and_several_batches(skm, base):
    r, o, l, f, i = base["inputs"]
    f2 = f.copy()
    f2[::3] = UNDEF
    f2[700:760] = UNDEF
    b = skm.SignatureBuilder(len(base["funcs"]), device=0)
    for a, e in ((0, 650), (650, 651), (651, 1400), (1400, 2000)):
        b.add_batch(r, o[a:e], l[a:e], f2[a:e], i[a:e])
    keep = np.nonzero(f2 != UNDEF)[0]
    assert b.resident_seqs() == (len(keep), int(l[keep].astype(np.int64).sum()) + len(keep))
    b.prepare()
    db = base["dbs"]["kept_db"]
    want = skm.FunctionCaller(db, base["funcs"]).best_seqs(r, o[keep], l[keep]).best
    for batch in (0, 3000):
        same_best(b.recall(db, base["tables"], batch_residues=batch).best, want, str(batch))
    b.close()


# ---- 5. release levels ----
def test_release_levels(skm, base):
    inputs, funcs = base["inputs"], base["funcs"]
    b = builder_of(skm, inputs, len(funcs))
    kept = b.finish()
    flags = b.signature_flags()
    db = b.kept_db(release_work=2)
    same_best(b.recall(db, base["tables"]).best, base["want_best"]["kept_db"])
    again = b.finish()
    np.testing.assert_array_equal(again.keys, kept.keys)
    np.testing.assert_array_equal(again.data.view(np.uint8), kept.data.view(np.uint8))
    np.testing.assert_array_equal(b.signature_flags(), flags)
    for call in (b.run, b.prepare, lambda: b.add_batch(*inputs), lambda: b.reserve(1000, 10)):
        with pytest.raises(skm.SkmError, match="error -6"):
            call()
    mph = b.mph_db(release_work="keep_sequences")  # the sequences are still there
    same_best(b.recall(mph, base["tables"], batch_residues=50_000).best, base["want_best"]["mph_db"])
    assert b.resident_seqs()[0] == 2000
    mph.close()
    # release_work = 1 frees them: the recall is refused and says why
    second = b.kept_db(release_work=True)
    with pytest.raises(skm.SkmError, match=r"error -6.*release_work"):
        b.recall(db, base["tables"])
    assert b.resident_seqs() == (0, 0)
    np.testing.assert_array_equal(b.finish().keys, kept.keys)
    second.close()
    db.close()
    b.close()
    b = builder_of(skm, inputs, len(funcs))
    db = b.kept_db(release_work=True)
    with pytest.raises(skm.SkmError, match=r"error -6.*release_work"):
        b.recall(db, base["tables"])
    with pytest.raises(skm.SkmError, match="release_work"):
        b.kept_db(release_work=3)
    db.close()
    b.close()


# ---- 6. refusals and empties ----
def test_refusals(skm, base):
    db = base["dbs"]["kept_db"]
    b = builder_of(skm, base["inputs"], len(base["funcs"]))
    with pytest.raises(skm.SkmError, match="error -6.*prepare"):  # added, not prepared
        b.recall(db, base["tables"])
    b.prepare()
    with pytest.raises(skm.SkmError, match="nothing asked for"):
        b.recall(db)
    opts = skm._AnnotOpts(5, 200, 0, base["hypo"], 0, 0)
    import ctypes as C
    assert skm.lib().skm_build_recall(b._h, db._h, C.byref(opts), None, None, None, None, None) == -1
    host_tables = skm.FunctionIndexTables(base["funcs"], device=-1)
    with pytest.raises(skm.SkmError, match="error -1.*without a device"):
        b.recall(db, host_tables)
    host_tables.close()
    same_best(b.recall(db, base["tables"]).best, base["want_best"]["kept_db"])  # prepared, not run: enough
    b.close()


def test_no_resident_sequences(skm, base):
    r, o, l, f, i = base["inputs"]
    b = skm.SignatureBuilder(len(base["funcs"]), device=0)
    b.add_batch(r, o[:50], l[:50], np.full(50, UNDEF, np.uint16), i[:50])
    b.prepare()
    assert b.resident_seqs() == (0, 0)
    got = b.recall(base["dbs"]["kept_db"], base["tables"], want_calls=True)
    assert len(got[0].best) == 0 and got[1].tolist() == [0] and len(got[2]) == 0
    assert got.stats["n_batches"] == 0 and got.stats["n_seqs"] == 0
    b.close()


# ---- 7. repeatability; the DB's uploaded path is unaffected in between ----
def test_repeatable_and_interleaved_with_uploads(skm, base):
    b, db = base["builder"], base["dbs"]["kept_db"]
    first = b.recall(db, base["tables"], batch_residues=100_000)
    up = skm.FunctionCaller(db, base["funcs"]).best_seqs(*base["own"]).best
    second = b.recall(db, base["tables"], batch_residues=100_000)
    same_best(first.best, second.best)
    same_best(up, base["want_best"]["kept_db"])
    same_best(first.best, up)
