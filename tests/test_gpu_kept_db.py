"""GPU tests of the exact-key DB built on the device from a finished build (skm_build_kept_db,
SignatureBuilder.kept_db): parity with the host path (finish + KeptKmerDb) and the oracle, the
smallest tables, the wrap at the table's end, a table of more than 2^32 slots, independence from
the build handle with release_work, and the refusals."""
import numpy as np
import pytest

import oracle_ref
from signature_kmers_amd import synth

pytestmark = pytest.mark.gpu

AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
MISS = 0xFFFFFFFF
M32 = np.uint64(0xFFFFFFFF)
M64 = (1 << 64) - 1


# ---- the slot function restated (murmur3 fmix64, then the high half of hash * T) ----
def fmix64(k: int) -> int:
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & M64
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & M64
    k ^= k >> 33
    return k


def py_slot(key: int, T: int) -> int:
    return (fmix64(int(key)) * T) >> 64


def np_slot(keys: np.ndarray, T: int) -> np.ndarray:
    """py_slot over an array (64 x 64 -> high 64 bits from 32-bit halves)."""
    k = np.asarray(keys, np.uint64).copy()
    s33, s32 = np.uint64(33), np.uint64(32)
    k ^= k >> s33
    k *= np.uint64(0xff51afd7ed558ccd)
    k ^= k >> s33
    k *= np.uint64(0xc4ceb9fe1a85ec53)
    k ^= k >> s33
    t = np.uint64(T)
    xl, xh, tl, th = k & M32, k >> s32, t & M32, t >> s32
    ll, lh, hl, hh = xl * tl, xl * th, xh * tl, xh * th
    mid = (ll >> s32) + (lh & M32) + (hl & M32)
    return hh + (lh >> s32) + (hl >> s32) + (mid >> s32)


def test_np_slot_is_py_slot():
    keys = np.random.default_rng(1).integers(1, 2**64 - 1, size=2000, dtype=np.uint64)
    for T in (16, 1009, 2**32 + 12345, 4_816_666_667):
        assert [int(v) for v in np_slot(keys, T)] == [py_slot(k, T) for k in keys.tolist()]


# ---- helpers ----
def pack(seqs):
    lens = np.array([len(s) for s in seqs], np.uint32)
    off = np.zeros(len(seqs), np.uint64)
    off[1:] = np.cumsum(lens[:-1])
    return np.frombuffer(b"".join(seqs), np.uint8), off, lens


def fm_of(data):
    return (data["function_index"].astype(np.uint32) << 16) | data["mean"]


def strangers_of(keys, n, seed):
    s = np.random.default_rng(seed).integers(1, 2**63, size=n, dtype=np.uint64)
    return s[~np.isin(s, keys)]


def synthetic(n_seqs, fam, seed):
    """The make_db-size synthetic sets of tests/test_gpu_annotate.py."""
    p = synth.generate_arrays(n_seqs, fam, per_file=500, seed=seed)
    r, o, l, f, i, funcs = synth.build_inputs(p)
    return p, (r, o, l, f, i), funcs


def builder_of(skm, inputs, n_functions, **kw):
    b = skm.SignatureBuilder(n_functions, device=0, **kw)
    b.add_batch(*inputs)
    return b


def edge_queries(p):
    """The query sequences of test_gpu_annotate.test_query_edge_cases: lengths 0, 7, 8, the 16-window
    tile edges, 'X' / '*' at a window's end, start and inside, lower case, long repeats."""
    src = p.residues[p.seq_off[0]:p.seq_off[0] + p.seq_len[0]].tobytes()
    seqs = [b"", b"ACDEFGH", b"ACDEFGHI", b"ACDEFGHIX", b"XACDEFGHI", src, src[:50] + b"X" + src[50:],
            src[:40] + b"*" + src[41:], src.lower(), src * 3, b"X" * 20, src * 7, src * 12, src * 40,
            src[:23], src[:24], src[:25], src[:23] + b"X", src[:24] + b"*", b"X" + src[:24]]
    return pack(seqs)


def assert_members_and_strangers(db, keys, data, seed=11, n_strangers=100_000):
    n = len(keys)
    assert db.hash_size() == n
    np.testing.assert_array_equal(db.lookup_fm(keys), fm_of(data))
    idx = db.lookup_keys(keys)
    np.testing.assert_array_equal(np.sort(idx), np.arange(n, dtype=np.uint32))
    s = strangers_of(keys, n_strangers, seed)
    assert (db.lookup_fm(s) == MISS).all()
    assert (db.lookup_keys(s) == n).all()


@pytest.fixture(scope="module")
def base(skm, gpu):
    """One 2000-sequence build: its kept set on the host, the host-path DB, the device-built DB, and
    the oracle's recall calls over the build's own proteins and over the edge queries."""
    p, inputs, funcs = synthetic(2000, 50, 5)
    b = builder_of(skm, inputs, len(funcs))
    kept = b.finish()
    ref_db = skm.KeptKmerDb(kept.keys, kept.data)
    db = b.kept_db()
    hypo = funcs.index("hypothetical protein")
    own = (p.residues, p.seq_off, p.seq_len)
    edge = edge_queries(p)
    want = {}
    for name, q in (("own", own), ("edge", edge)):
        want[name] = oracle_ref.annotate_exact(kept.keys, kept.data, *q, hypo_index=hypo)
    d = dict(p=p, inputs=inputs, funcs=funcs, builder=b, kept=kept, ref_db=ref_db, db=db, hypo=hypo,
             queries={"own": own, "edge": edge}, want=want)
    yield d
    db.close()
    ref_db.close()
    b.close()


def assert_calls(skm, db, base, names=("own", "edge")):
    caller = skm.FunctionCaller(db, base["funcs"])
    for name in names:
        off, calls = caller.process_seqs(*base["queries"][name])
        ooff, ocalls = base["want"][name]
        np.testing.assert_array_equal(off, ooff, err_msg=name)
        np.testing.assert_array_equal(calls.view(np.uint8), ocalls.view(np.uint8), err_msg=name)
    return len(calls)


# ---- 1. parity with the host path ----
def test_parity_with_host_path_and_oracle(skm, base):
    kept, db, ref_db = base["kept"], base["db"], base["ref_db"]
    n = len(kept.keys)
    assert n > 10_000 and isinstance(db, skm.CmphKmerDb)
    want_fm = fm_of(kept.data)
    np.testing.assert_array_equal(ref_db.lookup_fm(kept.keys), want_fm)
    np.testing.assert_array_equal(db.lookup_fm(kept.keys), want_fm)
    s = strangers_of(kept.keys, 100_000, 11)
    assert (db.lookup_fm(s) == MISS).all() and (ref_db.lookup_fm(s) == MISS).all()
    assert (db.lookup_keys(s) == n).all()
    idx = db.lookup_keys(kept.keys)
    np.testing.assert_array_equal(np.sort(idx), np.arange(n, dtype=np.uint32))
    # the table: default load 40 %, range-reduced, the plan's size
    slots, nbytes, nkeys, probe, ranged = db.table_info()
    assert (slots, nbytes) == skm.kept_db_plan(n) and slots == max(16, -(-100 * n // 40))
    assert nkeys == n and ranged == 1 and probe >= 1
    assert ref_db.table_info()[4] == 0 and ref_db.table_info()[2] == n
    # the call path: byte for byte the host-path DB's and the oracle's
    ref_caller = skm.FunctionCaller(ref_db, base["funcs"])
    caller = skm.FunctionCaller(db, base["funcs"])
    for name, q in base["queries"].items():
        off, calls = caller.process_seqs(*q)
        roff, rcalls = ref_caller.process_seqs(*q)
        np.testing.assert_array_equal(off, roff, err_msg=name)
        np.testing.assert_array_equal(calls.view(np.uint8), rcalls.view(np.uint8), err_msg=name)
    assert assert_calls(skm, db, base) > 0
    assert len(base["want"]["own"][1]) > 100
    # the per-window hits of the two lookup kernels
    for name, q in base["queries"].items():
        hits = []
        for d in (db, ref_db):
            qb = skm.QueryBatch(d, *q)
            qb.run(hypo_index=base["hypo"])
            hits.append(qb.window_hits())
            qb.close()
        for a, b in zip(*hits):
            np.testing.assert_array_equal(a, b, err_msg=name)
        assert name == "edge" or len(hits[0][1]) > 10_000


def test_lookup_fm_on_a_bdz_db(skm, base, tmp_path):
    """skm_db_lookup_fm on a BDZ DB: the record word of the slot the search lands on."""
    kept = base["kept"]
    stem = str(tmp_path / "kmer_data")
    skm.mph_build(kept.keys, kept.data, stem + ".mph", stem + ".dat", seed=7)
    bdz = skm.CmphKmerDb(stem)
    np.testing.assert_array_equal(bdz.lookup_fm(kept.keys), fm_of(kept.data))
    s = strangers_of(kept.keys, 10_000, 3)
    dat = np.frombuffer(open(stem + ".dat", "rb").read(), skm.STORED_DTYPE)
    idx = bdz.lookup_keys(s)
    hit = idx < len(dat)
    got = bdz.lookup_fm(s)
    np.testing.assert_array_equal(got[hit], fm_of(dat[idx[hit]]))
    assert (got[~hit] == MISS).all()
    assert bdz.table_info() == (0, 0, 0, 0, 0)
    bdz.close()


# ---- 2. smallest shapes ----
TINY = {"none": [b"ACDEFGH"], "one": [b"ACDEFGHI"]}


@pytest.mark.parametrize("which,n", [("none", 0), ("one", 1)])
@pytest.mark.parametrize("slots", ["n+1", "n+2", 16, "default"])
def test_smallest_tables(skm, gpu, which, n, slots):
    funcs = ["hypothetical protein", "alpha"]
    r, o, l = pack(TINY[which])
    b = builder_of(skm, (r, o, l, np.array([1], np.uint16), np.array([0], np.uint32)), len(funcs))
    kept = b.finish()
    assert len(kept.keys) == n
    T = {"n+1": n + 1, "n+2": n + 2, 16: 16, "default": 0}[slots]
    db = b.kept_db(slots=T)
    b.close()
    assert db.hash_size() == n
    info = db.table_info()
    assert info[0] == (T or 16) and info[2] == n and info[4] == 1 and info[3] == n
    s = strangers_of(kept.keys, 10_000, 5)
    assert (db.lookup_fm(s) == MISS).all()
    assert (db.lookup_keys(s) == n).all()
    assert (db.lookup_fm(np.zeros(3, np.uint64)) == MISS).all()  # key 0 marks an empty slot
    if n:
        np.testing.assert_array_equal(db.lookup_fm(kept.keys), fm_of(kept.data))
        np.testing.assert_array_equal(db.lookup_keys(kept.keys), np.zeros(1, np.uint32))
    # the call path over it: the only possible hit is one window, below min_hits
    q = pack([b"ACDEFGHI", b"", b"ACDEFGHIACDEFGHIKLMNP"])
    off, calls = skm.FunctionCaller(db, funcs).process_seqs(*q)
    ooff, ocalls = oracle_ref.annotate_exact(kept.keys, kept.data, *q, hypo_index=0)
    np.testing.assert_array_equal(off, ooff)
    np.testing.assert_array_equal(calls.view(np.uint8), ocalls.view(np.uint8))
    qb = skm.QueryBatch(db, *q)
    qb.run(hypo_index=0)
    hoff, pos, fm = qb.window_hits()
    assert list(hoff) == ([0, 1, 1, 3] if n else [0, 0, 0, 0])
    if n:
        assert list(pos) == [0, 0, 8] and (fm == fm_of(kept.data)[0]).all()
    qb.close()
    db.close()


@pytest.mark.parametrize("extra", [1, 2])
def test_one_or_two_empty_slots(skm, gpu, extra):
    """A table with n + 1 (n + 2) slots over a few hundred keys: every probe sequence may run
    through most of the table and a miss ends at the only empty slot."""
    rng = np.random.default_rng(17)
    seqs = [AA[rng.integers(0, 20, 8)].tobytes() for _ in range(300)]
    r, o, l = pack(seqs)
    b = builder_of(skm, (r, o, l, (1 + np.arange(300) % 2).astype(np.uint16), np.arange(300, dtype=np.uint32)), 3)
    kept = b.finish()
    n = len(kept.keys)
    assert n == len(set(seqs))
    db = b.kept_db(slots=n + extra)
    b.close()
    assert db.table_info()[0] == n + extra
    assert_members_and_strangers(db, kept.keys, kept.data, n_strangers=10_000)
    db.close()


# ---- 3. the wrap at the table's end ----
def test_probe_sequences_wrap_at_the_end(skm, gpu):
    T = 1009
    rng = np.random.default_rng(23)
    mers = np.ascontiguousarray(AA[rng.integers(0, 20, size=(40_000, 8))]).view(np.uint64).ravel()
    mers = np.unique(mers)
    home = np_slot(mers, T)
    tail = mers[home >= T - 4][:12]           # the plant: homes in the last four slots
    body = mers[home < T - 4][:300]
    assert len(tail) >= 8 and len(tail) > 4
    keys = np.concatenate([tail, body])
    rng.shuffle(keys)
    seqs = [int(k).to_bytes(8, "little") for k in keys]
    func = (1 + np.arange(len(seqs)) % 2).astype(np.uint16)
    r, o, l = pack(seqs)
    # the plant holds in the kept set (CPU oracle), before any GPU work
    ref = oracle_ref.build(r, o, l, func, np.arange(len(seqs), dtype=np.uint32), 3)
    assert np.array_equal(ref["keys"], np.sort(keys))
    rh = np.array([py_slot(k, T) for k in ref["keys"].tolist()])
    n_tail = int((rh >= T - 4).sum())
    assert n_tail >= 8 and n_tail > 4 and len(ref["keys"]) < T
    b = builder_of(skm, (r, o, l, func, np.arange(len(seqs), dtype=np.uint32)), 3)
    kept = b.finish()
    np.testing.assert_array_equal(kept.keys, ref["keys"])
    db = b.kept_db(slots=T)
    b.close()
    assert db.table_info()[0] == T and db.table_info()[3] >= 2
    assert_members_and_strangers(db, kept.keys, kept.data, n_strangers=10_000)
    # strangers homed at the last slot walk on through slot 0
    cand = rng.integers(1, 2**63, size=200_000, dtype=np.uint64)
    last = cand[(np_slot(cand, T) == T - 1) & ~np.isin(cand, kept.keys)]
    assert len(last) >= 50
    assert (db.lookup_fm(last) == MISS).all() and (db.lookup_keys(last) == len(kept.keys)).all()
    # and through the annotate kernel: a query made of the tail k-mers and of misses
    q = pack([b"".join(int(k).to_bytes(8, "little") for k in tail), int(last[0]).to_bytes(8, "little") * 3])
    off, calls = skm.FunctionCaller(db, ["hypothetical protein", "a", "b"]).process_seqs(*q)
    ooff, ocalls = oracle_ref.annotate_exact(kept.keys, kept.data, *q, hypo_index=0)
    np.testing.assert_array_equal(off, ooff)
    np.testing.assert_array_equal(calls.view(np.uint8), ocalls.view(np.uint8))
    qb = skm.QueryBatch(db, *q)
    qb.run(hypo_index=0)
    hoff, pos, fm = qb.window_hits()
    j = np.searchsorted(kept.keys, tail)
    at = np.isin(pos[:hoff[1]], 8 * np.arange(len(tail)))
    np.testing.assert_array_equal(fm[:hoff[1]][at], fm_of(kept.data)[j])
    qb.close()
    db.close()


# ---- 4. more than 2^32 slots ----
BIG_T = 2**32 + 12345   # 68.7 GB; a plain random search over protein 8-mers finds ~3 keys per
                        # million homed at or above slot 2^32 (checked on the CPU: 13 in 4 M tries)


def test_table_above_2_to_32_slots(skm, base):
    need = 16 * BIG_T
    # hipMemGetInfo through libskm: in this process torch.cuda finds no device once libskm's HIP
    # runtime is up ("No HIP GPUs are available")
    free = skm.device_mem_info(0)[0]
    if free < 1.25 * need:
        pytest.skip(f"the device has {free} bytes free; the 2^32 + 12345 slot table needs 1.25 x {need}")
    rng = np.random.default_rng(4)
    mers = np.ascontiguousarray(AA[rng.integers(0, 20, size=(4_000_000, 8))]).view(np.uint64).ravel()
    high = np.unique(mers[np_slot(mers, BIG_T) >= np.uint64(2**32)])
    assert len(high) >= 4
    high = high[:8]
    r, o, l, f, i = base["inputs"]
    hs, ho, hl = pack([int(k).to_bytes(8, "little") for k in high])
    fn = int(f[f != 0xFFFF][0])
    inputs = (np.concatenate([r, hs]), np.concatenate([o, ho + np.uint64(len(r))]), np.concatenate([l, hl]),
              np.concatenate([f, np.full(len(high), fn, np.uint16)]),
              np.concatenate([i, int(i.max()) + 1 + np.arange(len(high), dtype=np.uint32)]))
    b = builder_of(skm, inputs, len(base["funcs"]))
    kept = b.finish()
    # members homed at or above slot 2^32, by the restated slot function
    assert np.isin(high, kept.keys).all()
    homes = np_slot(kept.keys, BIG_T)
    assert int((homes >= np.uint64(2**32)).sum()) >= 4 and py_slot(high[0], BIG_T) >= 2**32
    db = b.kept_db(slots=BIG_T)
    b.close()
    assert db.table_info()[:3] == (BIG_T, need, len(kept.keys)) and db.table_info()[4] == 1
    assert_members_and_strangers(db, kept.keys, kept.data)
    j = np.searchsorted(kept.keys, high)
    np.testing.assert_array_equal(db.lookup_fm(high), fm_of(kept.data)[j])
    # calls equal the host-path DB's over the same kept set (queries: the build's proteins, the edge
    # sequences and the planted k-mers)
    ref_db = skm.KeptKmerDb(kept.keys, kept.data)
    planted = pack([b"".join(int(k).to_bytes(8, "little") for k in high)])
    for q in (base["queries"]["own"], base["queries"]["edge"], planted):
        off, calls = skm.FunctionCaller(db, base["funcs"]).process_seqs(*q)
        roff, rcalls = skm.FunctionCaller(ref_db, base["funcs"]).process_seqs(*q)
        np.testing.assert_array_equal(off, roff)
        np.testing.assert_array_equal(calls.view(np.uint8), rcalls.view(np.uint8))
    hits = []
    for d in (db, ref_db):
        qb = skm.QueryBatch(d, *planted)
        qb.run(hypo_index=base["hypo"])
        hits.append(qb.window_hits())
        qb.close()
    for a, c in zip(*hits):
        np.testing.assert_array_equal(a, c)
    assert np.isin(8 * np.arange(len(high)), hits[0][1]).all()
    ref_db.close()
    db.close()


# ---- 5. independence of the handle, release_work ----
def test_release_work_and_independence(skm, base):
    b = builder_of(skm, base["inputs"], len(base["funcs"]))
    kept = b.finish()
    np.testing.assert_array_equal(kept.keys, base["kept"].keys)
    slices = [b.finish_slice(2, s) for s in range(4)]
    flags = b.signature_flags()
    ctr = b.counters()
    db = b.kept_db(release_work=True)
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
    assert sum(len(s.keys) for s in slices) == len(kept.keys)
    np.testing.assert_array_equal(b.signature_flags(), flags)
    after = b.counters()
    for name in ("windows", "kept", "sequences", "grouped", "passes", "valid", "chain_jobs", "kept_cap"):
        assert after[name] == ctr[name], name
    # include/skm.h: a handle whose work buffers were released is only read out; the calls that
    # need them report SKM_E_STATE (-6)
    for call in (b.run, b.prepare, lambda: b.add_batch(*base["inputs"]), lambda: b.reserve(1000, 10)):
        with pytest.raises(skm.SkmError, match="error -6"):
            call()
    second = b.kept_db(load_pct=60, release_work=True)  # the arena is still there
    assert second.table_info()[0] == skm.kept_db_plan(len(kept.keys), load_pct=60)[0]
    b.close()
    for d in (db, second):
        assert_members_and_strangers(d, kept.keys, kept.data)
        assert_calls(skm, d, base)
        d.close()


def test_db_survives_a_rerun_of_the_builder(skm, base):
    p2, inputs2, funcs2 = synthetic(2000, 50, 9)
    b = builder_of(skm, base["inputs"], len(base["funcs"]))
    db = b.kept_db()
    b.add_batch(*inputs2)            # a different input: the arena is rewritten
    b.run()
    assert b.counters()["kept"] != len(base["kept"].keys)
    assert_members_and_strangers(db, base["kept"].keys, base["kept"].data)
    b.close()
    assert_calls(skm, db, base, names=("own",))
    db.close()


# ---- 6. refusals ----
def test_refusals(skm, base):
    p, db = base["p"], base["db"]
    with pytest.raises(skm.SkmError, match="error -1"):
        skm.MatrixDistance(db, base["funcs"], p.residues, p.seq_off[:50], p.seq_len[:50])
    with pytest.raises(skm.SkmError, match="error -1"):
        skm.MatrixDistanceBatch(db, base["funcs"], p.residues, p.seq_off[:50], p.seq_len[:50],
                                np.array([0, 20, 50], np.uint64))
    b2 = builder_of(skm, base["inputs"], len(base["funcs"]), rank=0, world_size=2)
    with pytest.raises(skm.SkmError, match="error -6"):
        b2.kept_db()
    b2.close()
    b = base["builder"]
    n = len(base["kept"].keys)
    for kw in (dict(load_pct=5), dict(load_pct=96), dict(slots=n), dict(slots=n - 1)):
        with pytest.raises(skm.SkmError, match="error -1"):
            b.kept_db(**kw)
    ok = b.kept_db(load_pct=95)      # the handle is still usable
    assert ok.table_info()[0] == -(-100 * n // 95)
    assert_members_and_strangers(ok, base["kept"].keys, base["kept"].data, n_strangers=10_000)
    ok.close()
