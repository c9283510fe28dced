"""CPU proof of the planted chain catalogue (tests/planted_chains.py): every build's chains are
recounted from the input arrays (windows, hashes, buckets, sub-buckets, groups -- not from the
planter's bookkeeping) and are exactly the planted ones; pyref's recurrences over every chain's
samples equal the oracle's median and var bit for bit, are nonzero and differ between any two chains
of one pass; the model of the scheduler's decisions (constants asserted against the text of
skm_build.hip) reaches every edge a build declares.  The last test prints which build holds which
edge.  The GPU side is tests/test_gpu_chain_edges.py."""
import numpy as np
import pytest

import oracle_ref
import planted_chains as pc
from planted import CAP, kmer_of

_facts = {}


def facts(name):
    """(build, recount, oracle result) of a build, computed once."""
    if name not in _facts:
        b = pc.BUILDS[name][0]()
        _facts[name] = (b, pc.facts(b.arrays, b.pass_bits), oracle_ref.build(*b.arrays, pc.NF))
    return _facts[name]


def sets(m, field, which="main"):
    return [m["sets"][(p, which)][field] for p in range(m["P"])]


def test_mirrored_constants_equal_the_source():
    pc.check_source()
    assert pc.CHAIN_B == 16 and pc.DEFER_MIN == 3 and pc.PLAN_WG == 1024 and pc.LONG_JOBS_MIN == 4096


def test_batch_arithmetic():
    """run_once's nb / per / slot arithmetic, restated: the cases the builds run."""
    slot, fl = pc.batch_of_pass(16, 2)
    assert fl == [(7, 0)] and slot == [0] * 8 + [16] * 8
    slot, fl = pc.batch_of_pass(16, 3)
    assert fl == [(4, 0), (9, 1), (14, 2)] and slot == [0] * 5 + [1] * 5 + [2] * 5 + [16]
    slot, fl = pc.batch_of_pass(16, 16)
    assert fl == [(p, p) for p in range(15)] and slot == list(range(15)) + [16]
    assert pc.batch_of_pass(16, 1) == ([16] * 16, [])
    slot, fl = pc.batch_of_pass(64, 16)
    assert fl == [(4 * k + 3, k) for k in range(15)] and slot[59] == 14 and slot[60:] == [16] * 4
    assert pc.batch_of_pass(2, 2) == ([0, 16], [(0, 0)])
    assert pc.batch_of_pass(4, 2) == ([0, 0, 16, 16], [(1, 0)])
    o = dict(lane_long=40, lane_tail=20)
    assert [pc.lane_threshold(16, s, o) for s in (0, 14, 16)] == [40, 40, 20]
    assert [pc.lane_threshold(4, s, o) for s in (0, 16)] == [20, 20]
    assert pc.lane_threshold(16, 0, dict(o, lane_long=0)) == 0
    assert sum(pc.chunk_sizes(257)) == 257 and pc.chunk_sizes(257)[:3] == [2, 2, 2] and pc.chunk_sizes(257)[129] == 0
    assert pc.chunk_sizes(256) == [1] * 256 and pc.chunk_sizes(255) == [1] * 255 + [0]
    assert [pc.job_class(n) for n in (1, 3, 4, 7, 8, 4095, 4096)] == [0, 1, 2, 2, 3, 11, 12]


@pytest.mark.parametrize("name", list(pc.BUILDS))
def test_inputs_are_the_planted_ones(name):
    b, F, _ = facts(name)
    # every window is a planted occurrence, every key the planted one, in the planted pass and bucket
    assert F.windows == sum(n + o for _, _, n, o, _ in b.decl)
    want = {}
    for sc, code, n, other, f in b.decl:
        want[int.from_bytes(kmer_of(code), "little")] = (n + other, n, f if n > other else None, sc.prefix, sc.pas)
    assert len(want) == len(b.decl) == len(F.keys)
    for k, key in enumerate(F.keys):
        n, cb, f, prefix, pas = want[int(key)]
        assert (F.n[k], F.cb[k], F.bucket[k], F.pas[k]) == (n, cb, prefix, pas), (name, k)
        assert f is None or F.best_f[k] == f
        assert len(F.samples[k]) == cb and F.kept[k]
    # the buckets are of the kinds their names state, recounted
    for sc in b.scs:
        ks = np.nonzero(F.bucket == sc.prefix)[0]
        total = int(F.n[ks].sum())
        kind = sc.name.split("_")[1]
        assert total == sc.planted, sc.name
        if kind in ("recs", "none"):
            assert total <= CAP and set(F.source[ks]) <= {"recs", "big"}, sc.name
            assert all((F.source[k] == "big") == (F.n[k] >= pc.BIG_MIN) for k in ks)
        elif kind == "tmp":
            assert total > CAP and set(F.source[ks]) == {"tmp"}, sc.name
        else:
            assert set(F.source[ks]) == {"lens"} and len(set(F.entry[ks])) == 1 and total > CAP, sc.name
    assert len(F.entries) == sum(1 for sc in b.scs if sc.name.split("_")[1] in ("lens", "heavy"))


@pytest.mark.parametrize("name", list(pc.BUILDS))
def test_pyref_equals_the_oracle_and_tells_chains_apart(name):
    b, F, ref = facts(name)
    exp = pc.expected(F)
    assert len(ref["keys"]) == len(F.keys)  # every planted key is kept
    at = np.searchsorted(ref["keys"], F.keys)
    assert np.array_equal(ref["keys"][at], F.keys)
    seen = {}
    for k, (med, var) in exp.items():
        row = ref["data"][at[k]]
        assert (int(row["median"]), int(row["var"])) == (med, var), (name, k, row, med, var)
        assert med != 0 and var != 0, (name, k)
        used = seen.setdefault(int(F.pas[k]), set())
        assert (med, var) not in used, (name, k, med, var)
        used.add((med, var))
    # and the keys without a chain keep what the group-by wrote
    rest = np.setdiff1d(np.arange(len(F.keys)), np.fromiter(exp, np.int64, len(exp)))
    assert np.all(F.cb[rest] < pc.DEFER_MIN)


def test_main_build_reaches_its_edges():
    b, F, _ = facts("main")
    m = pc.model(F, pc.MAIN_OPTS["base"])
    # c. job_chunk: the main set's job counts
    assert sets(m, "nj")[:6] == [0, 1, 255, 256, 257, 513]
    # d. nlong, nlong == nj, a second scan round and more jobs than k_long_stash has workgroups
    nl = sets(m, "nlong")
    assert [nl[p] for p in (0, 1, 6, 7, 8, 9)] == [0, 1, 1023, 1024, 1025, 2049] and nl[9] > pc.LONG_GRID
    assert sets(m, "rounds")[6:10] == [1, 1, 2, 3]
    assert all(m["sets"][(p, "main")]["nj"] == nl[p] for p in (1, 7)) and nl[2] == nl[13] == nl[14] == 0
    assert m["sets"][(10, "main")]["nlong"] > 0 and m["sets"][(10, "ovf")]["nlong"] > 0  # two streams reserve
    src = {}
    for k, s in m["stashed"].items():
        src.setdefault(s["source"], set()).add(s["pas"])
    assert src["tmp"] == {4} and src["big"] == {3, 10, 12} and src["lens"] == {10, 11} and len(src["recs"]) >= 9
    # b. class boundaries and a job in every class 1..12
    both = m["sets"][(10, "main")]["hist"], m["sets"][(10, "ovf")]["hist"]
    assert all(both[0][c] + both[1][c] > 0 for c in range(1, 13))
    assert [c for c, v in enumerate(m["sets"][(2, "main")]["hist"]) if v] == [1]
    p3 = m["sets"][(3, "main")]["lengths"]
    assert {3, 4, 5, 63, 64, 65} <= set(p3)
    # a. the per-lane blocks
    assert m["sets"][(2, "main")]["last_block"] == 63 and m["sets"][(14, "main")]["last_block"] == 1
    assert [nl[p] % 64 for p in (6, 8, 9)] == [63, 1, 1]
    m6 = pc.model(F, pc.MAIN_OPTS["class_6"])
    lane6 = [n for n in m6["sets"][(3, "main")]["lengths"] if n < 64]
    assert set(pc.BLOCK_EDGES) <= set(lane6)
    p15 = m6["sets"][(15, "main")]
    assert p15["nj"] == 19 and p15["nlong"] == 0 and set(pc.BLOCK_EDGES) <= set(p15["lengths"])  # one block holds them
    assert m6["sets"][(3, "main")]["nlong"] == 2 and m6["counters"]["demand_long_jobs"] == 11
    m13 = pc.model(F, pc.MAIN_OPTS["class_13"])
    assert m13["sets"][(11, "ovf")]["nj"] == 64 and m13["sets"][(11, "ovf")]["nlong"] == 0
    assert m13["sets"][(11, "ovf")]["lengths"][-2:] == [15, 3000] and m13["arena_total"] == 0
    # f. the thresholds' edges in an early batch and in the tail batch
    for name, early in (("base", 0), ("batches_3", 0), ("batches_16_streams_4", 3)):
        mm = pc.model(F, pc.MAIN_OPTS[name])
        for pas, slot, thr in ((3, early, pc.T_LONG), (15, pc.TAIL_SLOT, pc.T_TAIL)):
            got = {s["n"]: s["kernel"] for s in mm["stashed"].values() if s["pas"] == pas}
            assert all(s["slot"] == slot and s["threshold"] == thr for s in mm["stashed"].values() if s["pas"] == pas)
            for n in pc.T_EDGES:
                assert got[n] == ("lane" if n < thr else "pair"), (name, pas, n)
    assert set(s["kernel"] for s in pc.model(F, pc.MAIN_OPTS["lane_long_0"])["stashed"].values()) == {"pair"}
    # e. empty batches before and after non-empty ones
    bt = pc.model(F, pc.MAIN_OPTS["batches_16_streams_4"])["batches"]
    assert [bt[s] == 0 for s in (0, 1, 2, 3, 12, 13, 14)] == [True, False, True, False, False, True, True]
    assert bt[pc.TAIL_SLOT] > 0 and sum(bt.values()) == m["long_jobs"]
    assert pc.model(F, pc.MAIN_OPTS["batches_1"])["batches"] == {pc.TAIL_SLOT: m["long_jobs"]}


def test_arena_build_fits_to_the_element():
    b, F, _ = facts("arena")
    m = pc.model(F, pc.ARENA)
    assert len(F.entries) == 0 and m["scratch"] == 0 and m["split"] == 0
    st = sets(m, "stash")
    assert pc.work_buffer(m) == m["arena_total"] == sum(st) and st[1] == 0
    # one element short: passes 0 and 2 still fit, the reservation of pass 3 does not
    assert st[0] > 0 and st[0] + st[2] <= m["arena_total"] - 1 < sum(st) and st[3] > 1
    assert m["long_jobs"] < pc.LONG_JOBS_MIN  # the job slots cannot run out (the module's docstring)
    for pas in (0, 3):
        got = {s["n"]: s for s in m["stashed"].values() if s["pas"] == pas}
        assert all(got[n]["threshold"] == pc.T_TAIL and got[n]["kernel"] == ("lane" if n < pc.T_TAIL else "pair")
                   for n in pc.T_EDGES)


def test_small_pass_counts():
    b, F, _ = facts("passes_64")
    m = pc.model(F, pc.P64)
    assert [p for p in range(64) if m["sets"][(p, "main")]["nlong"]] == [0, 3, 4, 20, 62, 63]
    assert [s for s, n in m["batches"].items() if n] == [0, 1, 5, pc.TAIL_SLOT] and len(m["batches"]) == 16
    b, F, _ = facts("passes_2")
    m = pc.model(F, pc.P2)
    assert m["flushes"] == [(0, 0)] and all(v > 0 for v in m["batches"].values())
    assert set(s["threshold"] for s in m["stashed"].values()) == {pc.T_TAIL}


def test_giant_builds():
    b, F, _ = facts("giant")
    m = pc.model(F, pc.BUILDS["giant"][1]["giant_6"])
    assert [len(m["giants"][p]) for p in range(4)] == [1, 2, 3, 1025]
    n3 = sorted(int(F.cb[k]) for k in m["giants"][3])
    assert n3.count(64) > 900 and n3[-1] == 100 == m["counters"]["giant_max"] and n3.count(70) > 1
    assert sets(m, "nj", "ovf") == [33] * 4 == sets(m, "nlong", "ovf") and set(F.source) == {"lens"}
    assert m["counters"]["chain_samples"] == 4 * 33 * 60
    b, F, _ = facts("giant_4097")
    m = pc.model(F, pc.BUILDS["giant_4097"][1]["giant_6"])
    assert [len(m["giants"][p]) for p in range(2)] == [pc.GORD_MAX + 1, 0]


def test_print_the_edge_table(capsys):
    lines, held = [], set()
    for name, (make, opts) in pc.BUILDS.items():
        b = make()
        lines.append(f"build {name} ({len(b.arrays[2])} proteins): option sets {', '.join(opts)}")
        for letter, text in b.edges:
            lines.append(f"  {letter}. {text}")
            held.add(letter)
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert held == set("abcdefgh")
