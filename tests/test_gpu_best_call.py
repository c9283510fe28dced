"""The best-call kernel (skm_bestcall.hip k_best_calls, the core of csrc/skm_bestcall.h one lane per
sequence): bit-equal to the host batch function on the batches of bestcall_cases.py, at the wave and
workgroup edges, exact about what it defers, and -- on resident queries -- equal to a per-sequence
find_best_call over the downloaded calls."""
import ctypes as C

import numpy as np
import pytest

import bestcall_cases as bc
import fasta_device_util as fu

pytestmark = pytest.mark.gpu


def _host(skm, name):
    funcs, off, calls = bc.batch(name)
    return skm.best_calls_host(off, calls, skm.FunctionIndexTables(funcs, device=-1), n_threads=16)


@pytest.mark.parametrize("name", bc.SMALL + bc.FUZZ)
def test_kernel_is_bit_equal_to_the_host_batch(skm, gpu, name):
    funcs, off, calls = bc.batch(name)
    tb = skm.FunctionIndexTables(funcs, device=0)
    best, deferred, ms = skm.debug_best_calls(off, calls, tb)
    assert not deferred.any()
    want = _host(skm, name)
    assert want.n_deferred == 0
    bad = np.flatnonzero(best.view(np.uint64).reshape(-1, 2) != want.best.view(np.uint64).reshape(-1, 2))
    assert best.tobytes() == want.best.tobytes(), (len(bad), best[bad[0] // 2], want.best[bad[0] // 2])
    assert ms > 0


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 4097])
def test_batch_edges(skm, gpu, n):
    """The multi-call sequences last and first, single calls and empty sequences between."""
    tb, th = skm.FunctionIndexTables(bc.FUNCS, device=0), skm.FunctionIndexTables(bc.FUNCS, device=-1)
    multi = [s for s in bc.kat_seqs() if len(s) >= 3][:6]
    for where in ("last", "first"):
        seqs = [[(k % len(bc.FUNCS), 3 + k % 5, 300)] if k % 3 else [] for k in range(n)]
        m = multi[:n]
        if m:
            if where == "last":
                seqs[-len(m):] = m
            else:
                seqs[:len(m)] = m
        off, calls = bc.to_batch(seqs)
        best, deferred, _ = skm.debug_best_calls(off, calls, tb)
        want = skm.best_calls_host(off, calls, th)
        assert len(best) == n and not deferred.any() and best.tobytes() == want.best.tobytes()
        if n:
            bc.assert_equal_to_reference(best, tb.names(best), bc._reference(skm.lib().skm_find_best_call, bc.FUNCS,
                                                                             off, calls), (n, where))


def test_kernel_defers_exactly_by_the_rule(skm, gpu):
    funcs, seqs, expect = bc.defer_seqs()
    _, off, calls = bc.batch("defer")
    tb = skm.FunctionIndexTables(funcs, device=0)
    best, deferred, _ = skm.debug_best_calls(off, calls, tb)
    np.testing.assert_array_equal(deferred, expect)
    want = _host(skm, "defer")
    keep = expect == 0
    assert best[keep].tobytes() == want.best[keep].tobytes()


def test_tables_without_a_device_are_refused(skm, gpu):
    funcs, off, calls = bc.batch("split")
    th = skm.FunctionIndexTables(funcs, device=-1)
    n = len(off) - 1
    best, deferred = np.zeros(n, skm.BEST_DTYPE), np.zeros(n, np.uint8)
    rc = skm.lib().skm_debug_best_calls(calls.ctypes.data, off.ctypes.data, n, th._h, 0, best.ctypes.data,
                                        deferred.ctypes.data, None)
    assert rc == -1   # SKM_E_ARG


# ------------------------------------------------------------------ resident queries
@pytest.fixture(scope="module")
def small_db(skm, gpu, tmp_path_factory):
    from signature_kmers_amd import synth
    p = synth.generate_arrays(3000, 40, per_file=500, seed=17)
    r, o, l, f, i, funcs = synth.build_inputs(p)
    b = skm.SignatureBuilder(len(funcs), device=0)
    b.add_batch(r, o, l, f, i)
    kept = b.finish()
    b.close()
    base = str(tmp_path_factory.mktemp("best_db") / "kmer_data")
    skm.mph_build(kept.keys, kept.data, base + ".mph", base + ".dat", seed=1)
    assert len(kept.keys) > 1000
    return base, funcs


def _host_arrays(blobs):
    seqs = [s for b in blobs for _, s in fu.expected(b)]
    lens = np.array([len(s) for s in seqs], np.uint32)
    off = np.zeros(len(seqs), np.uint64)
    if len(seqs):
        off[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    return np.frombuffer(b"".join(seqs), dtype=np.uint8), off, lens


def _query_files(n_seqs, seed):
    from signature_kmers_amd import synth
    q = synth.generate_arrays(3000 + n_seqs, 40, per_file=250, first_file=12, n_files=(n_seqs + 249) // 250, seed=seed,
                              extras=True)
    blobs = []
    for f in np.unique(q.file_of):
        idx = np.nonzero(q.file_of == f)[0]
        a, e = int(q.seq_off[idx[0]]), int(q.seq_off[idx[-1]] + q.seq_len[idx[-1]])
        ids = [b"fig|%d.1.peg.%d" % (f, k + 1) for k in range(len(idx))]
        blobs.append(synth.fasta_bytes(ids, q.residues[a:e], q.seq_len[idx]))
    return blobs, _host_arrays(blobs)


def _per_sequence(skm, funcs, off, calls):
    return bc._reference(skm.lib().skm_find_best_call, funcs, off, np.ascontiguousarray(calls))


def _check(skm, r, funcs, off, calls):
    assert r.n_seqs == len(off) - 1 and r.n_calls == len(calls)
    bc.assert_equal_to_reference(r.best, r.names(), _per_sequence(skm, funcs, off, calls), "query")


@pytest.mark.parametrize("ignore_hypo", [False, True])
def test_query_best_calls_equal_find_best_call_over_its_calls(skm, gpu, small_db, ignore_hypo):
    base, funcs = small_db
    db = skm.CmphKmerDb(base, device=0)
    tb = skm.FunctionIndexTables(funcs, device=0)
    _, (res, qoff, lens) = _query_files(1500, seed=17)
    q = skm.QueryBatch(db, res, qoff, lens)
    out = skm._BestCalls()
    assert skm.lib().skm_query_best_calls(q._h, tb._h, C.byref(out)) == -6   # SKM_E_STATE: not run yet
    q.run(funcs.index("hypothetical protein"), ignore_hypo=ignore_hypo)
    r = q.best_calls(tb)
    off, calls = q.calls()
    assert len(calls) > 100 and r.n_deferred == 0 and r.kernel_ms > 0
    assert r.n_windows == int(np.maximum(lens.astype(np.int64) - 7, 0).sum())
    _check(skm, r, funcs, off, calls)
    assert (r.best["fi"] != 0xFFFF).sum() > 100
    th = skm.FunctionIndexTables(funcs, device=-1)
    assert skm.lib().skm_query_best_calls(q._h, th._h, C.byref(out)) == -1     # SKM_E_ARG: no device tables
    assert skm.lib().skm_query_best_calls(q._h, None, C.byref(out)) == -1
    assert r.best.tobytes() == skm.best_calls_host(off, calls, th).best.tobytes()
    q.close()
    db.close()


def test_function_caller_best_seqs_and_best_fasta(skm, gpu, small_db):
    """best_seqs and best_fasta through the DB's kept query: a large batch, a smaller one after it,
    the large one again; equal to each other and to the host path on a second DB handle."""
    base, funcs = small_db
    db, db_host = skm.CmphKmerDb(base, device=0), skm.CmphKmerDb(base, device=0)
    caller, host = skm.FunctionCaller(db, funcs), skm.FunctionCaller(db_host, funcs)
    large, small = _query_files(1500, seed=17), _query_files(250, seed=17)
    for hypo in (False, True):
        caller.ignore_hypothetical(hypo)
        host.ignore_hypothetical(hypo)
        for blobs, arrays in (large, small, large):
            off, calls = host.process_seqs(*arrays)
            a = caller.best_seqs(*arrays)
            b = caller.best_fasta(blobs)
            assert caller.last_fasta.n_recs == len(arrays[2])
            assert a.best.tobytes() == b.best.tobytes() and a.names() == b.names()
            assert a.n_deferred == b.n_deferred == 0 and a.n_calls == b.n_calls == len(calls) > 0
            _check(skm, a, funcs, off, calls)
    db.close()
    db_host.close()


def test_a_batch_without_calls(skm, gpu, small_db):
    base, funcs = small_db
    db = skm.CmphKmerDb(base, device=0)
    caller = skm.FunctionCaller(db, funcs)
    res = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWYACD" * 3, dtype=np.uint8)
    r = caller.best_seqs(res, np.array([0, 23, 46], np.uint64), np.array([23, 23, 5], np.uint32))
    assert r.n_seqs == 3 and r.n_calls == 0 and r.names() == ["", "", ""]
    assert (r.best["fi"] == 0xFFFF).all() and (r.best["score"] == 0).all() and (r.best["flags"] == 0).all()
    r = caller.best_fasta([b"junk only\n", b""])
    assert r.n_seqs == 0 and len(r.best) == 0
    r = caller.best_seqs(np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
    assert r.n_seqs == 0
    db.close()
