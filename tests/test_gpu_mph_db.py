"""GPU tests of the BDZ signature DB built and opened on the device from a finished build
(skm_build_mph_db, SignatureBuilder.mph_db): the image and the .dat byte for byte those of
mph_build over the sorted kept set, the DB against the one opened from those files and against the
oracle (lookups, calls, window hits, matrix distance), the host fallback below 1024 keys and the
first device sizes, independence from the build handle with release_work, and the refusals."""
import numpy as np
import pytest

import oracle_ref
from test_gpu_kept_db import AA, builder_of, edge_queries, fm_of, pack, strangers_of, synthetic

pytestmark = pytest.mark.gpu

RANK_TILE = 64  # rank blocks (of 128 vertices) per tile of the device rank scan: one wave


def read(path):
    with open(path, "rb") as fh:
        return fh.read()


def calls_of(skm, db, funcs, q):
    return skm.FunctionCaller(db, funcs).process_seqs(*q)


def assert_same_calls(a, b, msg=""):
    np.testing.assert_array_equal(a[0], b[0], err_msg=msg)
    np.testing.assert_array_equal(a[1].view(np.uint8), b[1].view(np.uint8), err_msg=msg)


@pytest.fixture(scope="module")
def base(skm, gpu, tmp_path_factory):
    """The 2000-sequence build of tests/test_gpu_kept_db.py: its kept set on the host, the files
    mph_build writes over it (the yardstick), the DB mph_db makes with the files it writes, the DB
    opened from those files, and the oracle's handle and calls."""
    p, inputs, funcs = synthetic(2000, 50, 5)
    b = builder_of(skm, inputs, len(funcs))
    kept = b.finish()
    d = tmp_path_factory.mktemp("mph_db")
    ref_stem, stem = str(d / "ref"), str(d / "kmer_data")
    skm.mph_build(kept.keys, kept.data, ref_stem + ".mph", ref_stem + ".dat", seed=7, device=0)
    db = b.mph_db(seed=7, verify=True, mph_path=stem + ".mph", dat_path=stem + ".dat")
    file_db = skm.CmphKmerDb(stem)
    image, dat = read(stem + ".mph"), read(stem + ".dat")
    bdz = oracle_ref.Bdz(image)
    hypo = funcs.index("hypothetical protein")
    queries = {"own": (p.residues, p.seq_off, p.seq_len), "edge": edge_queries(p)}
    want = {k: oracle_ref.annotate(bdz, dat, *q, hypo_index=hypo) for k, q in queries.items()}
    e = dict(p=p, inputs=inputs, funcs=funcs, builder=b, kept=kept, ref_stem=ref_stem, stem=stem, db=db,
             file_db=file_db, image=image, dat=dat, bdz=bdz, hypo=hypo, queries=queries, want=want,
             strangers=strangers_of(kept.keys, 100_000, 11))
    yield e
    db.close()
    file_db.close()
    b.close()


# ---- 1. the image and the .dat are mph_build's ----
def test_image_identity(skm, base):
    kept, n = base["kept"], len(base["kept"].keys)
    # the rank table spans many tiles of the device scan (411,363 keys: 3,953 rank blocks, 62 tiles)
    assert n > 10_000 and -(-skm.mph_db_plan(n)[1] // 128) > 4 * RANK_TILE
    assert base["image"] == read(base["ref_stem"] + ".mph")
    assert base["dat"] == read(base["ref_stem"] + ".dat")
    assert len(base["dat"]) == 10 * n
    again = base["builder"].mph_db(seed=7)       # no files: the same DB
    np.testing.assert_array_equal(again.lookup_keys(kept.keys), base["db"].lookup_keys(kept.keys))
    np.testing.assert_array_equal(again.lookup_keys(base["strangers"]), base["db"].lookup_keys(base["strangers"]))
    st = again.stats
    assert st["n_keys"] == n and st["n_vertices"] == skm.mph_db_plan(n)[1] and st["attempts"] == 1
    assert st["upload_s"] == 0 and st["verified"] == 0 and st["peel_rounds"] > 1
    again.close()
    other = base["builder"].mph_db(seed=8)       # another seed: another hash over the same keys
    assert not np.array_equal(other.lookup_keys(kept.keys), base["db"].lookup_keys(kept.keys))
    np.testing.assert_array_equal(other.lookup_fm(kept.keys), fm_of(kept.data))
    other.close()


# ---- 2. the DB against the one opened from its files and against the oracle ----
def test_db_equivalence(skm, base):
    kept, db, file_db, bdz = base["kept"], base["db"], base["file_db"], base["bdz"]
    n = len(kept.keys)
    assert isinstance(db, skm.CmphKmerDb) and db.stats["verified"] == 1
    assert db.hash_size() == file_db.hash_size() == bdz.size() == n
    assert db.table_info() == (0, 0, 0, 0, 0)
    slots = bdz.search(kept.keys)
    np.testing.assert_array_equal(np.sort(slots), np.arange(n, dtype=np.uint32))
    for keys, want in ((kept.keys, slots), (base["strangers"], bdz.search(base["strangers"]))):
        for d in (db, file_db):
            np.testing.assert_array_equal(d.lookup_keys(keys), want)
            np.testing.assert_array_equal(d.lookup_keys_generic(keys), want)
    np.testing.assert_array_equal(db.lookup_fm(kept.keys), fm_of(kept.data))
    np.testing.assert_array_equal(db.lookup_fm(base["strangers"]), file_db.lookup_fm(base["strangers"]))
    for name, q in base["queries"].items():
        got = calls_of(skm, db, base["funcs"], q)
        assert_same_calls(got, calls_of(skm, file_db, base["funcs"], q), name)
        assert_same_calls(got, base["want"][name], name)
        hits = []
        for d in (db, file_db):
            qb = skm.QueryBatch(d, *q)
            qb.run(hypo_index=base["hypo"])
            hits.append(qb.window_hits())
            qb.close()
        for a, c in zip(*hits):
            np.testing.assert_array_equal(a, c, err_msg=name)
        assert name == "edge" or len(hits[0][1]) > 10_000
    assert len(base["want"]["own"][1]) > 100


# ---- 3. matrix distance over it ----
def test_matrix_distance_over_the_device_built_db(skm, base):
    p, funcs = base["p"], base["funcs"]
    q = (p.residues, p.seq_off[:50], p.seq_len[:50])
    exp = oracle_ref.matrix_distance(base["bdz"], base["dat"], *q, np.arange(50, dtype=np.uint32), base["hypo"])
    assert len(exp) > 0
    for d in (base["db"], base["file_db"]):
        md = skm.MatrixDistance(d, funcs, *q)
        np.testing.assert_array_equal(md.compute(), exp)
        md.close()
    cuts = [0, 20, 50]
    exp_b = [oracle_ref.matrix_distance(base["bdz"], base["dat"], p.residues, p.seq_off[a:z], p.seq_len[a:z],
                                        np.arange(z - a, dtype=np.uint32), base["hypo"])
             for a, z in zip(cuts[:-1], cuts[1:])]
    assert sum(len(x) for x in exp_b) > 0
    for d in (base["db"], base["file_db"]):
        mb = skm.MatrixDistanceBatch(d, funcs, *q, np.array(cuts, np.uint64))
        got = mb.compute()
        mb.close()
        assert len(got) == 2
        for g, x in zip(got, exp_b):
            np.testing.assert_array_equal(g, x)


# ---- 4. the host fallback and the first device sizes ----
def singletons(n, seed):
    """n distinct 8-residue sequences: each is one window, kept as a singleton of its function."""
    rng = np.random.default_rng(seed)
    mers = np.unique(np.ascontiguousarray(AA[rng.integers(0, 20, size=(2 * n + 16, 8))]).view(np.uint64).ravel())
    assert len(mers) >= n
    mers = mers[:n].copy()
    rng.shuffle(mers)
    return [int(k).to_bytes(8, "little") for k in mers]


# 3r is odd at every one of these sizes (r is made odd), so the last g word and the last rank block
# are partly filled: 3r = 3, 3, 3, 1263, 1263, 1263, 1599, 5043
@pytest.mark.parametrize("n", [0, 1, 2, 1023, 1024, 1025, 1300, 4099])
def test_small_and_edge_sizes(skm, gpu, tmp_path, n):
    funcs = ["hypothetical protein", "alpha", "beta"]
    seqs = singletons(n, 100 + n) if n else [b"ACDEFGH"]     # n = 0: seven residues, no window
    func = (1 + np.arange(len(seqs)) % 2).astype(np.uint16)
    b = builder_of(skm, (*pack(seqs), func, np.arange(len(seqs), dtype=np.uint32)), len(funcs))
    kept = b.finish()
    assert len(kept.keys) == n and skm.mph_db_plan(n)[1] % 2 == 1
    stem, ref = str(tmp_path / "kmer_data"), str(tmp_path / "ref")
    db = b.mph_db(seed=3, verify=True, mph_path=stem + ".mph", dat_path=stem + ".dat")
    b.close()
    # below 1024 keys the host builder ran (no peel on the device), from 1024 on the device's
    assert (db.stats["attempts"] > 0) == (n >= 1024) and db.stats["verified"] == 1
    assert db.stats["n_keys"] == n
    skm.mph_build(kept.keys, kept.data, ref + ".mph", ref + ".dat", seed=3, device=0)
    image, dat = read(stem + ".mph"), read(stem + ".dat")
    assert image == read(ref + ".mph")
    assert dat == read(ref + ".dat") and len(dat) == 10 * n
    assert db.hash_size() == n
    bdz = oracle_ref.Bdz(image)
    if n:
        idx = db.lookup_keys(kept.keys)
        np.testing.assert_array_equal(np.sort(idx), np.arange(n, dtype=np.uint32))
        np.testing.assert_array_equal(idx, bdz.search(kept.keys))
        np.testing.assert_array_equal(db.lookup_keys_generic(kept.keys), idx)
        np.testing.assert_array_equal(db.lookup_fm(kept.keys), fm_of(kept.data))
    # three short queries: a run of kept k-mers of one function, an empty sequence, and a stranger
    one = b"".join([s for s, f in zip(seqs, func) if f == 1][:12]) if n else b""
    q = pack([one, b"", b"ACDEFGHIACDEFGHIKLMNP"])
    assert_same_calls(calls_of(skm, db, funcs, q), oracle_ref.annotate(bdz, dat, *q, hypo_index=0))
    # the window hits of the first: every window lands on the record the oracle's search gives
    # (a BDZ DB has no key check), the kept k-mers at offsets 0, 8, .. on their own records
    qb = skm.QueryBatch(db, *q)
    qb.run(hypo_index=0)
    hoff, pos, fm = qb.window_hits()
    qb.close()
    if n:
        w = np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(np.frombuffer(one, np.uint8), 8))
        slot = bdz.search(w.view(np.uint64).ravel())
        hit = slot < n
        recs = np.frombuffer(dat, skm.STORED_DTYPE)
        np.testing.assert_array_equal(pos[:hoff[1]], np.flatnonzero(hit))
        np.testing.assert_array_equal(fm[:hoff[1]], fm_of(recs[slot[hit]]))
        assert hit[::8].all() and hoff[1] >= len(one) // 8
    else:
        assert list(hoff) == [0, 0, 0, 0]
    db.close()


# ---- 5. independence of the handle, release_work ----
def assert_is_base_db(skm, db, base, names=("own", "edge")):
    kept = base["kept"]
    np.testing.assert_array_equal(db.lookup_keys(kept.keys), base["bdz"].search(kept.keys))
    np.testing.assert_array_equal(db.lookup_keys(base["strangers"]), base["file_db"].lookup_keys(base["strangers"]))
    np.testing.assert_array_equal(db.lookup_fm(kept.keys), fm_of(kept.data))
    for name in names:
        assert_same_calls(calls_of(skm, db, base["funcs"], base["queries"][name]), base["want"][name], name)


def test_db_survives_a_rerun_of_the_builder(skm, base):
    p2, inputs2, funcs2 = synthetic(2000, 50, 9)
    b = builder_of(skm, base["inputs"], len(base["funcs"]))
    db = b.mph_db(seed=7)
    b.add_batch(*inputs2)            # a different input: the arena is rewritten
    b.run()
    assert b.counters()["kept"] != len(base["kept"].keys)
    assert_is_base_db(skm, db, base, names=())
    b.close()
    assert_is_base_db(skm, db, base)
    db.close()


def test_release_work_contract(skm, base):
    b = builder_of(skm, base["inputs"], len(base["funcs"]))
    kept = b.finish()
    np.testing.assert_array_equal(kept.keys, base["kept"].keys)
    slices = [b.finish_slice(2, s) for s in range(4)]
    flags = b.signature_flags()
    ctr = b.counters()
    db = b.mph_db(seed=7, release_work=True)
    again = b.finish()
    np.testing.assert_array_equal(again.keys, kept.keys)
    np.testing.assert_array_equal(again.data.view(np.uint8), kept.data.view(np.uint8))
    np.testing.assert_array_equal(again.distinct_functions, kept.distinct_functions)
    np.testing.assert_array_equal(again.seqs_with_func, kept.seqs_with_func)
    assert (again.n_seqs_with_signature, again.distinct_signatures, again.n_windows) == \
        (kept.n_seqs_with_signature, kept.distinct_signatures, kept.n_windows)
    for s in range(4):
        sl = b.finish_slice(2, s)
        np.testing.assert_array_equal(sl.keys, slices[s].keys)
        np.testing.assert_array_equal(sl.data.view(np.uint8), slices[s].data.view(np.uint8))
    np.testing.assert_array_equal(b.signature_flags(), flags)
    after = b.counters()
    for name in ("windows", "kept", "sequences", "grouped", "passes", "valid", "chain_jobs", "kept_cap"):
        assert after[name] == ctr[name], name
    # include/skm.h: a handle whose work buffers were released is only read out
    for call in (b.run, b.prepare, lambda: b.add_batch(*base["inputs"]), lambda: b.reserve(1000, 10)):
        with pytest.raises(skm.SkmError, match="error -6"):
            call()
    second = b.mph_db(seed=7, release_work=True)   # the arena is still there
    kdb = b.kept_db()
    b.close()
    for d in (db, second):
        assert_is_base_db(skm, d, base)
        d.close()
    np.testing.assert_array_equal(kdb.lookup_fm(kept.keys), fm_of(kept.data))
    assert (kdb.lookup_fm(base["strangers"]) == 0xFFFFFFFF).all()
    kdb.close()


# ---- 6. refusals ----
def test_refusals(skm, base, tmp_path):
    b2 = builder_of(skm, base["inputs"], len(base["funcs"]), rank=0, world_size=2)
    with pytest.raises(skm.SkmError, match="error -6"):
        b2.mph_db()
    b2.close()
    b = base["builder"]
    with pytest.raises(skm.SkmError, match="error -1"):
        b.kept_db(load_pct=5)
    with pytest.raises(skm.SkmError, match="error -4"):  # a path that cannot be written
        b.mph_db(seed=7, mph_path=str(tmp_path / "missing" / "kmer_data.mph"))
    ok = b.mph_db(seed=7)            # the handle is still usable
    assert_is_base_db(skm, ok, base, names=("edge",))
    ok.close()
