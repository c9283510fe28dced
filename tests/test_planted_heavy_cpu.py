"""CPU proof of the planted heavy-key catalogue (tests/planted_heavy.py): every scenario's windows
are exactly the planted ones and lie in one overflow sub-bucket of the declared size, the planned
sequence indices are the ones the input has, the model of the kernels' decisions (constants asserted
against the text of skm_build.hip) reaches every edge a scenario declares, and the hand-written
expectations equal the oracle, which equals pyref on the scenarios pyref can take.  The last test
prints which scenario holds which edge.  The GPU side is tests/test_gpu_heavy_edges.py."""
import numpy as np
import pytest

import oracle_ref
import planted_heavy as ph
import pyref
from planted import CAP, b2_of, hash_of_keys

_facts = {}


def facts(name):
    """(scenarios, arrays, n_total, oracle result) of a build, computed once."""
    if name not in _facts:
        scs, arrays, nt = ph.BUILDS[name][0]()
        _facts[name] = (scs, arrays, nt, oracle_ref.build(*arrays, scs[0].nf))
    return _facts[name]


def key_int(kmer):
    return int.from_bytes(kmer, "little")


def test_mirrored_constants_equal_the_source():
    src = ph.source_constants()
    for name in ph.MIRRORED:
        assert src[name] == getattr(ph, name), name
    text = ph.source_text()
    assert ph.SPLIT_HASH_TEXT in text and 'static_assert(SPLIT_TAB == 4096, "split_hash yields 12 bits");' in text
    assert "int ovf_heavy = %d;" % ph.OVF_HEAVY in text                       # option overflow_heavy_min's default
    assert "reinterpret_cast<uint32_t*>(s_hi), 2 * CAP, s_wave, r)" in text   # group_block's run-head capacity
    assert "? 14 : 0);" in text and "while (NBK < HV_NBK && NBK * 256u < n) NBK <<= 1;" in text
    assert "uint32_t kk = n / 2, d = 0;" in text and "if ((float)cb < float(n) * 0.8f) continue;" in text


def test_fillers_have_no_window():
    assert len(oracle_ref.kmer_windows(b"X")) == 0
    res, off, lens = ph.pack([b"X", b"X"])
    assert lens.tolist() == [1, 1] and off.tolist() == [0, 1]


@pytest.mark.parametrize("name", list(ph.BUILDS))
def test_inputs_are_the_planted_ones(name):
    scs, arrays, nt, _ = facts(name)
    res, off, lens, funcs, ids = arrays
    assert len(lens) == nt and len(set(sc.prefix for sc in scs)) == len(scs)
    used = np.zeros(nt, bool)
    for sc in scs:
        # the planned sequence indices, and the proteins at them
        idx = sc.index
        assert not used[idx].any() and len(np.unique(idx)) == len(idx), sc.name
        used[idx] = True
        for k, at in enumerate(sc.plan):
            assert at is None or idx[k] == at, (sc.name, k)
        assert np.array_equal(lens[idx], [len(s) for s in sc.seqs]) and np.array_equal(funcs[idx], sc.funcs), sc.name
        for k in range(0, len(idx), max(1, len(idx) // 200)):
            o = int(off[idx[k]])
            assert res[o:o + len(sc.seqs[k])].tobytes() == sc.seqs[k], (sc.name, k)
        # the windows: the planted groups and nothing else, in one sub-bucket of the declared size
        km, fn, sq, of, ln = ph.members_of(sc)
        h = hash_of_keys(km)
        g = sc.geom
        assert np.all(g.prefix_of(h) == np.uint64(sc.prefix)), sc.name
        assert np.all(g.sub_of(h, 11) == np.uint64(sc.deep[1])), sc.name
        assert len(km) == sc.total == sc.n_elements() > CAP and sc.b2 == b2_of(sc.total), sc.name
        got = np.bincount(g.sub_of(h, sc.b2).astype(np.int64), minlength=1 << sc.b2)
        assert tuple(int(x) for x in got) == tuple(sc.sub_sizes), sc.name
        keys, cnt = np.unique(km, return_counts=True)
        want = {key_int(k): len(f) for k, f in sc.groups}
        assert dict(zip((int(k) for k in keys), (int(c) for c in cnt))) == want, sc.name
        for kmer, f in sc.groups:
            if len(f) > 1:
                assert sorted(fn[km == np.uint64(key_int(kmer))].tolist()) == sorted(f), sc.name
    # everything else is a filler
    assert np.all(lens[~used] == 1) and np.all(res[off[~used].astype(np.int64)] == ord("X"))


def key_claim(sc, nt, k, sel, field, want):
    km, fn, sq, of, ln = ph.members_of(sc)
    sq, of, ln, best = sq[sel], of[sel], ln[sel], fn[sel] == k["best_f"]
    n = int(np.count_nonzero(sel))
    if field == "has_buckets":
        have = list(k["sorted_buckets"])
        for b in want:
            assert b in have, (sc.name, field, b)
            have.remove(b)
    elif field == "empty_best":
        assert int(np.count_nonzero(k["bests"] == 0)) == want
    elif field == "best_buckets":
        assert np.nonzero(k["bests"])[0].tolist() == want
    elif field == "members":
        assert k["members"].tolist() == want
    elif field == "at_boundaries":
        for b in range(k["nbk"]):
            lo, hi = -(-b * nt // k["nbk"]), -(-(b + 1) * nt // k["nbk"])
            assert hi - 1 in sq and (b == 0 or lo in sq), (sc.name, b)
            assert (hi - 1) * k["nbk"] // nt == b and hi * k["nbk"] // nt == b + 1
    elif field == "median_on_edge":
        o = of & 0xFFFF
        hi = np.bincount(o >> 8, minlength=256)
        kk, d = n // 2, 0
        on_high = kk in np.cumsum(hi)[hi > 0].tolist()
        while kk >= hi[d]:
            kk -= hi[d]
            d += 1
        lo = np.bincount(o[(o >> 8) == d] & 255, minlength=256)
        on_low = kk > 0 and kk in np.cumsum(lo)[lo > 0].tolist()
        assert (on_high, on_low) == ((True, False) if want == "high" else (False, True)), (sc.name, on_high, on_low)
    elif field == "high_bytes":
        assert sorted(set(((of & 0xFFFF) >> 8).tolist())) == want
    elif field == "wraps":
        assert int(np.count_nonzero(of > 0xFFFF)) == want
    elif field == "length_sum":
        assert int(ln[best].sum()) == want
    else:
        assert k[field] == want, (sc.name, field, k[field], want)


@pytest.mark.parametrize("name", list(ph.BUILDS))
def test_model_reaches_the_declared_edges(name):
    scs, arrays, nt, _ = facts(name)
    for sc in scs:
        m = ph.model(sc, nt, sc.nf, sc.under)
        km = ph.members_of(sc)[0]
        for what, want in sc.claims.items():
            if what in ("entry", "overflow"):
                have = m if what == "entry" else m["overflow"]
                for field, v in want.items():
                    assert have[field] == v, (sc.name, what, field, have[field], v)
            else:
                key = key_int(sc.names[what])
                for field, v in want.items():
                    key_claim(sc, nt, m["keys"][key], km == np.uint64(key), field, v)
    if name == "plan":
        for opts, nsplit in ((ph.PLAN_OPTS["split_min_mid"], 6 + sum(1 for j in range(1030) if j % 40 >= 20)), (ph.PLAN_OPTS["unsplit"], 0)):
            ms = [ph.model(sc, nt, sc.nf, opts) for sc in scs]
            assert sum(m["split"] for m in ms) == nsplit and len(ms) > 1024
            assert sorted(m["stream"] for m in ms).count(2) == 2


def test_probe_chains_wrap_past_the_last_slot():
    """probe_wrap's 640 keys have their split_hash homes (restated from the source text asserted
    above, not process_sub's table hash) in 4000..4095, which has room for at most 96 of them: the
    others' probe chains cross from slot 4095 to slot 0.  The full table of distinct_4096 wraps too."""
    scs, arrays, nt, _ = facts("main")
    by_name = {sc.name: sc for sc in scs}
    m = ph.model(by_name["probe_wrap"], nt, ph.NF, ph.HEAVY16, table=True)
    assert m["distinct"] == 640 and 4000 <= m["home_min"] and m["home_max"] <= ph.SPLIT_TAB - 1
    assert m["probe_wrapped"] == 640 - (ph.SPLIT_TAB - m["home_min"]) >= 544
    full = ph.model(by_name["distinct_4096"], nt, ph.NF, {}, table=True)
    assert full["distinct"] == ph.SPLIT_TAB and not full["fail"] and full["probe_wrapped"] >= 1


def test_model_counts_follow_the_options():
    """The same main build under its option sets: what the counters must report differs as stated."""
    scs, arrays, nt, _ = facts("main")
    c = {k: ph.counters_of(scs, nt, ph.NF, o) for k, o in ph.MAIN_OPTS.items()}
    assert c["default"]["giant_chains"] == 0 and c["giant_10"]["giant_max"] == 4096
    assert c["giant_10"]["chain_jobs"] == c["default"]["chain_jobs"] - c["giant_10"]["giant_chains"]
    assert c["heavy_lsd"] == c["default"] and c["heavy_lsd_16"] == c["heavy_min_16"]
    assert c["heavy_min_16"]["overflow_light_subbuckets"] == c["default"]["overflow_light_subbuckets"] + 3
    assert c["ovf_light_0"]["overflow_light_elements"] == 0 == c["unsplit"]["overflow_light_elements"]
    assert len(set(x["overflow_elements"] for x in c.values())) == 1
    scs, arrays, nt, _ = facts("overflow")
    a = ph.counters_of(scs, nt, scs[0].nf, ph.OVF_OPTS["unsplit"])
    b = ph.counters_of(scs, nt, scs[0].nf, ph.OVF_OPTS["unsplit_inline_16"])
    assert b["chain_samples"] == a["chain_samples"] and a["chain_jobs"] - b["chain_jobs"] >= ph.OVF_INLINE_CAP
    m = ph.model(next(s for s in scs if s.name == "chains_520"), nt, scs[0].nf, ph.OVF_OPTS["unsplit_inline_16"])
    assert m["inline"] == ph.OVF_INLINE_CAP and m["jobs"] == 520 - ph.OVF_INLINE_CAP


@pytest.mark.parametrize("name", list(ph.BUILDS))
def test_oracle_agrees_with_expectations(name):
    scs, arrays, nt, ref = facts(name)
    rows = dict(zip((int(k) for k in ref["keys"]), ref["data"]))
    for sc in scs:
        wrong = [k for k, is_kept in sc.expect.items() if (key_int(k) in rows) != is_kept]
        assert not wrong, (sc.name, wrong[:5], len(wrong))
        for kmer, funcs in sc.groups:
            assert sc.expect[kmer] == ph.kept_rule(int(max(np.bincount(funcs))), len(funcs)), (sc.name, kmer)
        for kmer, f in sc.best.items():
            assert rows[key_int(kmer)]["function_index"] == f, (sc.name, kmer)
        for kmer, v in sc.avg.items():
            assert rows[key_int(kmer)]["avg_from_end"] == v, (sc.name, kmer, rows[key_int(kmer)], v)
        for kmer, v in sc.mean.items():
            assert rows[key_int(kmer)]["mean"] == v, (sc.name, kmer, rows[key_int(kmer)], v)
    assert len(rows) == sum(sum(sc.expect.values()) for sc in scs)


PYREF_RESIDUES = 400000   # pyref walks every residue in Python: the scenarios below this many


@pytest.mark.parametrize("name", ["main", "overflow", "wide"])
def test_oracle_agrees_with_pyref(name):
    """A scenario's proteins alone, in the order of their sequence indices, give its keys the same
    records as the whole build (the visit order is the relative order): pyref on those."""
    scs, arrays, nt, ref = facts(name)
    rows = dict(zip((int(k) for k in ref["keys"]), ref["data"]))
    done = 0
    for sc in scs:
        if sum(len(s) for s in sc.seqs) > PYREF_RESIDUES or sc.total > 6000:
            continue
        order = np.argsort(sc.index)
        out = pyref.build_py([sc.seqs[k] for k in order], [sc.funcs[k] for k in order], list(range(len(order))),
                             sc.nf)[0]
        assert set(out) == set(key_int(k) for k, kept in sc.expect.items() if kept), sc.name
        for key, rec in out.items():
            assert tuple(int(x) for x in rows[key]) == rec, (sc.name, key, rows[key], rec)
        done += 1
    assert done >= (8 if name == "main" else 1)


def test_print_the_edge_table(capsys):
    lines = []
    for name, (make, opts) in ph.BUILDS.items():
        scs = make()[0]
        lines.append(f"build {name}: option sets {', '.join(opts)}")
        if name == "main_passes4":
            lines.append("  (the scenarios of main, planted for two pass bits and spread over the four passes)")
            assert sorted(set(sc.prefix >> 12 for sc in scs)) == [0, 1, 2, 3]
            continue
        for sc in scs:
            for e in sc.edges:
                lines.append(f"  {sc.name:24s} {e}")
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert sum(1 for ln in lines if ln.startswith("  ")) >= 45
