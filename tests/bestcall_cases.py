"""Batches of calls for the best-call tests (test_best_call_cpu.py on the host batch function,
test_gpu_best_call.py on the kernel): the cases of test_host_cpu.py restated as batches, planted
cases, a fuzz of 200,000+ sequences over three function indices, and a small batch that must be
deferred.  Every batch is made once per process; the per-sequence references (skm_find_best_call
and the oracle) are computed once and shared."""
import ctypes as C
import functools
import itertools

import numpy as np

import oracle_ref

CALL = oracle_ref.CALL_DTYPE

FUNCS = sorted([f"function {i:05d}" for i in range(10)] +
               ["function 00001 / function 00003", "function 00005 / function 00002",
                "function 00007 / function 00001 / function 00004", "hypothetical protein"],
               key=lambda s: s.encode())
FUNCS_SPLIT = sorted(["alpha", "beta", "alpha / beta", "alpha / ", " / beta", "alpha / / beta", "x // y",
                      "alpha /  / beta", "beta / alpha", "alpha / beta / ", "a/b", "hypothetical protein", ""],
                     key=lambda s: s.encode())
# index order opposite to name order
FUNCS_REV = ["zeta", "mid", "alpha", "alpha / mid"]


def big_index():
    """A few hundred names: 60 (a, b, "a / b", "b / a") groups whose parts are names themselves,
    names of exactly 8 parts, "" and the hypothetical protein, then duplicates: names already
    present, again, under a second index (so the index is not sorted either)."""
    names = []
    for g in range(60):
        a, b = f"fn {2 * g:03d}", f"fn {2 * g + 1:03d}"
        names += [a, b, f"{a} / {b}", f"{b} / {a}"]
    for g in range(12):
        names.append(" / ".join(f"fn {(g + 7 * k) % 120:03d}" for k in range(8)))
    names += ["", "hypothetical protein"]
    names += [names[4 * g] for g in range(0, 60, 3)] + [names[4 * g + 2] for g in range(0, 60, 4)]
    return names


FUNCS_BIG = big_index()


def groups_of(funcs):
    """(a, b, w) index triples with w a " / " name: the shapes a fusion can take in this index."""
    i = {f: k for k, f in enumerate(funcs)}   # a duplicated name: its last index
    out = []
    for w, f in enumerate(funcs):
        p = f.split(" / ")
        if len(p) >= 2:
            out.append((i.get(p[0], 0), i.get(p[-1], 0), w))
    return out


def to_batch(seqs):
    """[[(fi, count, median), ...], ...] -> (call_off u64, calls)."""
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in seqs], dtype=np.uint64)
    c = np.zeros(int(off[-1]), CALL)
    k = 0
    for rows in seqs:
        for j, (fi, cnt, med) in enumerate(rows):
            c[k] = (10 * j, 10 * j + 40, cnt, fi, 0, med, 1.5)
            k += 1
    return off, c


def kat_seqs():
    """test_host_cpu.py:81-114 (KATs and the 40 random cases, same generators and seeds) and the
    planted cases, over FUNCS."""
    i = {f: k for k, f in enumerate(FUNCS)}
    f1, f3, f13 = i["function 00001"], i["function 00003"], i["function 00001 / function 00003"]
    f5, f7, f2 = i["function 00005"], i["function 00007"], i["function 00002"]
    seqs = [[], [(f1, 7, 300)], [(f1, 4, 300)],
            [(f1, 6, 200), (f13, 9, 500), (f3, 6, 300)],      # A W B
            [(f1, 6, 200), (f13, 9, 900), (f3, 6, 300)],      # inconsistent lengths
            [(f1, 6, 300), (f3, 2, 300), (f1, 6, 300)],       # F1 F2 F1
            [(f1, 6, 300), (f3, 5, 300)]]                     # close race
    for seed in range(40):
        rng = np.random.default_rng(seed)
        rows = []
        for _ in range(int(rng.integers(0, 9))):
            rows.append((int(rng.integers(0, len(FUNCS))), int(rng.integers(1, 25)), int(rng.integers(80, 1200))))
        if seed % 4 == 0 and len(rows) >= 3:
            a, b = int(rng.integers(150, 400)), int(rng.integers(150, 400))
            rows[:3] = [(i["function 00005"], 6, a),
                        (i["function 00005 / function 00002"], 8, a + b + int(rng.integers(-40, 40))),
                        (i["function 00002"], 5, b)]
        seqs.append(rows)
    # repeated merges F1 F2 F1 F2 F1: F2.count 4 and 5, F1 + F1 = 9 and 10
    for c2 in (4, 5):
        for first, second in ((5, 4), (5, 5), (4, 5), (9, 1)):
            for tail in (1, 6):
                seqs.append([(f1, first, 300), (f3, c2, 300), (f1, second, 300), (f3, c2, 300), (f1, tail, 300)])
    # W A W B W, and with a trailing extra key
    seqs.append([(f13, 6, 500), (f1, 6, 200), (f13, 9, 500), (f3, 6, 300), (f13, 3, 500)])
    seqs.append([(f13, 6, 500), (f1, 6, 200), (f13, 9, 500), (f3, 6, 300), (f13, 3, 500), (f5, 2, 100)])
    seqs.append([(f13, 6, 500), (f1, 6, 200), (f1, 1, 210), (f13, 9, 520), (f3, 6, 300)])
    # frac_dif at the float nearest 0.1 (100 / 1000 -> 0.1f > 0.1): not a fusion; just inside is
    seqs.append([(f1, 6, 400), (f13, 9, 1000), (f3, 6, 500)])
    seqs.append([(f1, 6, 400), (f13, 9, 1000), (f3, 6, 501)])
    seqs.append([(f1, 6, 450), (f13, 9, 1000), (f3, 6, 650)])   # + 0.1
    # sums that round in float: medians near 2^25
    seqs.append([(f1, 6, 2**24 + 1), (f1 + 0, 1, 3), (f13, 9, 2**25 + 3), (f3, 6, 2**24 + 1)])
    seqs.append([(f1, 6, 2**24 + 1), (f13, 9, 2**25 - 1), (f3, 6, 2**24 - 3), (f13, 9, 2**25 + 5)])
    # three and four functions with ties among the top three, in every assignment of counts to
    # indices (by_func is in index order: these are the partial_sort leftovers)
    for fs in ((f1, f3, f5), (f7, f2, f13)):
        for cs in itertools.product((5, 6, 7, 8), repeat=3):
            seqs.append([(f, c, 300) for f, c in zip(fs, cs)])
    for cs in itertools.product((6, 7, 9), repeat=4):
        seqs.append([(f, c, 300) for f, c in zip((f7, f1, f5, f3), cs)])
    for cs in itertools.permutations((9, 8, 6, 6, 5)):      # pair_offset 2 and 3 in every order
        seqs.append([(f, c, 300) for f, c in zip((f1, f2, f3, f5, f7), cs)])
    seqs.append([(f1, 9, 300), (f3, 8, 300), (f5, 6, 300)])   # pair_offset 2: no call
    seqs.append([(f1, 9, 300), (f3, 8, 300), (f5, 5, 300)])   # pair_offset 3: "f1 ?? f3"
    return seqs


def split_seqs():
    """test_host_cpu.py:197-211 over FUNCS_SPLIT."""
    seqs = []
    i = {f: k for k, f in enumerate(FUNCS_SPLIT)}
    for seed in range(30):
        rng = np.random.default_rng(1000 + seed)
        rows = [(int(rng.integers(0, len(FUNCS_SPLIT))), int(rng.integers(1, 15)), int(rng.integers(80, 900)))
                for _ in range(int(rng.integers(1, 7)))]
        if seed % 3 == 0:
            w = ["alpha / beta", "alpha / / beta", "alpha / ", " / beta"][seed % 4]
            rows = [(i["alpha"], 6, 200), (i[w], 9, 500), (i["beta"], 6, 300)] + rows[:2]
        seqs.append(rows)
    return seqs


def rev_seqs():
    """Two functions whose name order is the opposite of their index order, both call orders."""
    seqs = []
    for a, b in itertools.permutations(range(len(FUNCS_REV)), 2):
        for ca, cb in ((6, 5), (5, 6), (6, 6), (9, 7)):
            seqs.append([(a, ca, 300), (b, cb, 300)])
            seqs.append([(a, ca, 300), (b, cb, 300), (0xFFFF, 2, 300)])
    return seqs


def fuzz_batch(funcs, n, seed):
    """n sequences of 0-12 calls.  Each draws from a palette of its own -- a fusion triple
    (a, b, "a / b") of the index, another fusion name and one index from anywhere, the indices
    past the table and 0xFFFF included -- so that runs, F1 F2 F1 shapes, fusions and ties are
    common.  Counts 1-24 (half of them below 7); medians up to 2^25 with the fusion's near a + b."""
    rng = np.random.default_rng(seed)
    nf = len(funcs)
    gr = np.array(groups_of(funcs), np.int64)
    ncalls = rng.integers(0, 13, n)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(ncalls, dtype=np.uint64)
    tot = int(off[-1])
    seq = np.repeat(np.arange(n), ncalls)
    g = gr[rng.integers(0, len(gr), n)]
    anyidx = rng.integers(0, nf + 3, n)
    anyidx[rng.random(n) < 0.05] = 0xFFFF
    pal = np.stack([g[:, 0], g[:, 1], g[:, 2], gr[rng.integers(0, len(gr), n), 2], anyidx], axis=1)
    big = rng.random(n) < 0.2
    ma = np.where(big, rng.integers(2**23, 2**24, n), rng.integers(80, 1200, n))
    mb = np.where(big, rng.integers(2**23, 2**24, n), rng.integers(80, 1200, n))
    mw = ma + mb + ((ma + mb) * rng.uniform(-0.15, 0.15, n)).astype(np.int64)
    med = np.stack([ma, mb, mw, np.where(big, rng.integers(2**24, 2**25, n), rng.integers(80, 2400, n)),
                    rng.integers(80, 1200, n)], axis=1)
    slot = rng.choice(5, size=tot, p=[0.3, 0.25, 0.25, 0.1, 0.1])
    c = np.zeros(tot, CALL)
    j = np.arange(tot) - np.repeat(off[:-1].astype(np.int64), ncalls)
    c["start"] = 10 * j
    c["end"] = 10 * j + 40
    c["count"] = np.where(rng.random(tot) < 0.5, rng.integers(1, 7, tot), rng.integers(1, 25, tot))
    c["function_index"] = pal[seq, slot]
    c["protein_length_median"] = np.minimum(med[seq, slot] + rng.integers(-3, 4, tot), 2**25)
    c["protein_length_med_avg_dev"] = 1.5
    return off, c


def defer_seqs():
    """(funcs, seqs, expected deferred): more than 64 calls or a name of more than 8 parts."""
    funcs = ["aa", "bb", "aa / bb", " / ".join(f"p{k}" for k in range(9)), " / ".join(["aa", "bb"] + [f"p{k}" for k in range(6)]), "cc"]
    seqs = [[(k % 2, 1, 300) for k in range(70)],                       # 70 calls: 35 vs 35 -> "bb ?? aa"
            [(0, 6, 200), (3, 9, 500), (1, 6, 300)],                    # a 9-part name
            [(0, 6, 200), (2, 9, 500), (1, 6, 300)],
            [(k % 3, 2, 300) for k in range(65)],
            [(k % 3, 2, 300) for k in range(64)],                       # 64 calls: not deferred
            [],
            [(3, 7, 300)],
            [(0, 6, 200), (4, 9, 500), (1, 6, 300)],                    # 8 parts: not deferred
            [(5, 3, 100)] * 66 + [(0, 2, 100)]]                         # 67 raw calls (2 collapsed)
    return funcs, seqs, np.array([1, 1, 0, 1, 0, 0, 1, 0, 1], np.uint8)


@functools.lru_cache(maxsize=None)
def batch(name):
    """name -> (funcs, call_off, calls)."""
    if name == "kat":
        return (FUNCS,) + to_batch(kat_seqs())
    if name == "split":
        return (FUNCS_SPLIT,) + to_batch(split_seqs())
    if name == "rev":
        return (FUNCS_REV,) + to_batch(rev_seqs())
    if name == "defer":
        return (defer_seqs()[0],) + to_batch(defer_seqs()[1])
    if name == "fuzz_funcs":
        return (FUNCS,) + fuzz_batch(FUNCS, 60000, 11)
    if name == "fuzz_split":
        return (FUNCS_SPLIT,) + fuzz_batch(FUNCS_SPLIT, 60000, 12)
    if name == "fuzz_big":
        return (FUNCS_BIG,) + fuzz_batch(FUNCS_BIG, 90000, 13)
    raise KeyError(name)


FUZZ = ("fuzz_funcs", "fuzz_split", "fuzz_big")
SMALL = ("kat", "split", "rev")


def _reference(fn, funcs, off, calls):
    arr = (C.c_char_p * max(1, len(funcs)))(*[s.encode("latin-1") for s in funcs])
    n = len(off) - 1
    fi = np.zeros(n, np.uint16)
    score = np.zeros(n, np.float32)
    offset = np.zeros(n, np.float32)
    names = []
    buf = C.create_string_buffer(4096)
    base = calls.ctypes.data
    cf, cs, co = C.c_uint16(), C.c_float(), C.c_float()
    rf, rs, ro = C.byref(cf), C.byref(cs), C.byref(co)
    o = off.astype(np.int64).tolist()
    lf, ls, lo = [], [], []
    for s in range(n):
        a, b = o[s], o[s + 1]
        fn(C.c_void_p(base + 24 * a), b - a, arr, len(funcs), rf, rs, ro, buf, 4096)
        lf.append(cf.value)
        ls.append(cs.value)
        lo.append(co.value)
        names.append(buf.value)
    fi[:], score[:], offset[:] = lf, ls, lo
    return fi, score, offset, names


@functools.lru_cache(maxsize=None)
def reference(name, which):
    """Per-sequence find_best_call over a batch: which = "skm" (skm_find_best_call) or "oracle"
    (oracle_find_best_call) -> (fi u16, score f32, offset f32, [name bytes])."""
    import signature_kmers_amd as skm
    funcs, off, calls = batch(name)
    if which == "skm":
        fn = skm.lib().skm_find_best_call
    else:
        fn = oracle_ref.olib().oracle_find_best_call
    return _reference(fn, funcs, off, calls)


def assert_equal_to_reference(best, names, ref, what):
    """Field for field, floats as bits, names as bytes."""
    fi, score, offset, rnames = ref
    bad = np.flatnonzero((best["fi"] != fi) | (best["score"].view(np.uint32) != score.view(np.uint32)) |
                         (best["offset"].view(np.uint32) != offset.view(np.uint32)))
    assert len(bad) == 0, (what, len(bad), int(bad[0]), best[bad[0]], fi[bad[0]], score[bad[0]], offset[bad[0]])
    nb = [k for k, (a, b) in enumerate(zip(names, rnames)) if a.encode("latin-1") != b]
    assert not nb, (what, len(nb), nb[0], names[nb[0]], rnames[nb[0]])
