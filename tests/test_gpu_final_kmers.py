"""GPU tests of final.kmers written from the resident arena (skm_build_write_final_kmers,
SignatureBuilder.write_final_kmers) and of the statistics without the kept set (skm_build_stats).

The expected bytes of every file are built here with numpy and str from finish() of the same
handle or of a twin handle -- key bytes via .view(np.uint8), decimals via str -- never by the code
under test."""
import os

import numpy as np
import pytest

import planted
from signature_kmers_amd import synth

pytestmark = pytest.mark.gpu

AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)


def expected(kept) -> bytes:
    """KMER \\t avg_from_end \\t function_index \\t \\n per kept k-mer, in finish()'s (ascending key) order."""
    kb = np.ascontiguousarray(kept.keys, dtype="<u8").view(np.uint8).reshape(-1, 8)
    a, f = kept.data["avg_from_end"], kept.data["function_index"]
    return b"".join(kb[i].tobytes() + b"\t" + str(int(a[i])).encode() + b"\t" + str(int(f[i])).encode() + b"\t\n"
                    for i in range(len(kb)))


def read(path) -> bytes:
    with open(path, "rb") as fh:
        return fh.read()


def builder_of(skm, inputs, n_functions, **kw):
    b = skm.SignatureBuilder(n_functions, device=0, **kw)
    b.add_batch(*inputs)
    return b


def write(b, path):
    st = b.write_final_kmers(str(path))
    return read(path), st


@pytest.fixture(scope="module")
def c1(skm, gpu):
    """The C1 build (1000 proteins, 40 families, lower-case residues and B/Z/U among them): its
    inputs, its kept set from finish() and the expected text."""
    p = synth.generate_arrays(1000, 40, per_file=100, extras=True)
    r, o, l, f, i, funcs = synth.build_inputs(p)
    b = builder_of(skm, (r, o, l, f, i), len(funcs))
    kept = b.finish()
    d = dict(inputs=(r, o, l, f, i), nf=len(funcs), builder=b, kept=kept, want=expected(kept))
    yield d
    b.close()


# ---- 1. C1 synth ----
def test_c1_file_equals_the_expected_bytes(skm, c1, tmp_path):
    kept = c1["kept"]
    assert len(kept.keys) > 100_000
    raw = kept.keys.view(np.uint8)
    assert ((raw >= ord("a")) & (raw <= ord("z"))).any()  # lower-case residues reach the file as they are
    got, st = write(c1["builder"], tmp_path / "final.kmers")
    assert got == c1["want"]
    assert st["n_kmers"] == len(kept.keys) and st["bytes"] == len(got) == os.path.getsize(tmp_path / "final.kmers")
    assert st["chunks"] >= 1 and st["pieces"] >= st["chunks"] and st["wide_index"] == 0 and st["gather_ms"] == 0
    # the host formatter over the same kept set: the function the kernels run
    assert skm.final_kmers_host(kept.keys, kept.data) == c1["want"]


# ---- 2. digit widths, planted ----
def test_every_digit_width_in_both_columns(skm, gpu, tmp_path):
    rng = np.random.default_rng(41)
    nf = 65534
    seqs = [AA[rng.integers(0, 20, 10_010)].tobytes()]
    funcs = [10000]
    for fn in (0, 9, 10, 99, 100, 999, 1000, 9999, 65533):
        seqs.append(AA[rng.integers(0, 20, 12)].tobytes())
        funcs.append(fn)
    a, bb = 10, 65536 - 8  # one valid window whose distance from the end is 65536: avg_from_end wraps to 0
    seqs.append(b"X" * a + b"MKVLAAGI" + b"X" * bb)
    funcs.append(1000)
    r, o, l = planted.pack(seqs)
    b = builder_of(skm, (r, o, l, np.array(funcs, np.uint16), np.arange(len(seqs), dtype=np.uint32)), nf)
    kept = b.finish()
    want = expected(kept)
    # the plant holds: every width 1..5 in both columns, and the value 0 in both
    for col in ("avg_from_end", "function_index"):
        widths = {len(str(int(v))) for v in kept.data[col]}
        assert widths == {1, 2, 3, 4, 5}, (col, widths)
        assert (kept.data[col] == 0).any(), col
    zero = kept.data[kept.keys == np.frombuffer(b"MKVLAAGI", "<u8")[0]]
    assert len(zero) == 1 and zero["avg_from_end"][0] == 0 and b"MKVLAAGI\t0\t1000\t\n" in want
    assert {len(x) + 1 for x in want.split(b"\n")[:-1]} >= {14, 22}
    got, st = write(b, tmp_path / "final.kmers")
    b.close()
    assert got == want and st["n_kmers"] == len(kept.keys) and st["bytes"] == len(want)


# ---- 3. tile edges ----
def test_tile_edges(skm, gpu, tmp_path):
    L = skm.final_kmers_info()[0]
    rng = np.random.default_rng(43)
    codes = np.unique(rng.integers(0, planted.NCODES, 3 * L, dtype=np.int64))
    rng.shuffle(codes)
    assert len(codes) > 2 * L + 1
    for n in (1, L - 1, L, L + 1, 2 * L + 1):
        seqs = [planted.kmer_of(c) for c in codes[:n]]
        r, o, l = planted.pack(seqs)
        func = (np.arange(n) * 37 % 1201).astype(np.uint16)
        b = builder_of(skm, (r, o, l, func, np.arange(n, dtype=np.uint32)), 1201)
        kept = b.finish()
        assert len(kept.keys) == n  # one valid window each, every one kept
        got, st = write(b, tmp_path / f"final_{n}.kmers")
        b.close()
        assert got == expected(kept), n
        assert st["n_kmers"] == n and st["bytes"] == len(got)


# ---- 4. chunks, wide indices, pieces ----
def test_small_chunks_wide_indices_small_pieces(skm, c1, tmp_path):
    b = builder_of(skm, c1["inputs"], c1["nf"])
    plain, st0 = write(b, tmp_path / "plain.kmers")
    b.set_option("handoff_max_chunk", 64)
    b.set_option("handoff_index_limit", 1)
    b.set_option("final_kmers_piece_kb", 1)   # the smallest piece: lines straddle the pieces
    got, st = write(b, tmp_path / "chunked.kmers")
    b.close()
    assert st["chunks"] > 4 and st["pieces"] > st["chunks"] and st["wide_index"] == 1
    assert st0["wide_index"] == 0
    assert got == plain
    assert got == c1["want"]
    for bad in (-1, (1 << 20) + 1):
        with pytest.raises(skm.SkmError, match="error -1"):
            c1["builder"].set_option("final_kmers_piece_kb", bad)


# ---- 5. empty and overwrite ----
def test_no_kept_kmer_truncates_the_file(skm, gpu, tmp_path):
    path = tmp_path / "final.kmers"
    path.write_bytes(b"junk" * (1 << 18))
    assert os.path.getsize(path) == 1 << 20
    r, o, l = planted.pack([b"ACDEFGH"])
    b = builder_of(skm, (r, o, l, np.array([1], np.uint16), np.array([0], np.uint32)), 2)
    got, st = write(b, path)
    assert len(b.finish().keys) == 0
    b.close()
    assert got == b"" and os.path.getsize(path) == 0
    assert st["n_kmers"] == 0 and st["bytes"] == 0 and st["chunks"] == 0 and st["pieces"] == 0


# ---- 6. after release ----
@pytest.mark.parametrize("which", ["kept_db", "mph_db"])
def test_after_release_work(skm, c1, tmp_path, which):
    twin = builder_of(skm, c1["inputs"], c1["nf"])
    b = builder_of(skm, c1["inputs"], c1["nf"])
    for x in (twin, b):  # options first: setting one after a release asks for a rerun (SKM_E_STATE)
        x.set_option("handoff_max_chunk", 1 << 15)
        x.set_option("final_kmers_piece_kb", 256)
    want, st_twin = write(twin, tmp_path / "twin.kmers")
    twin.close()
    db = b.kept_db(release_work=True) if which == "kept_db" else b.mph_db(release_work=True)
    got, st = write(b, tmp_path / "released.kmers")
    with pytest.raises(skm.SkmError, match="error -6"):
        b.run()  # the handle is released indeed
    b.close()
    db.close()
    assert got == want == c1["want"]
    assert (st["n_kmers"], st["bytes"], st["chunks"]) == (st_twin["n_kmers"], st_twin["bytes"], st_twin["chunks"])
    assert st["chunks"] > 4


# ---- 7. stats() ----
def assert_stats_equal_finish(s, k):
    assert len(s.keys) == 0 and len(s.data) == 0
    assert s.keys.dtype == k.keys.dtype and s.data.dtype == k.data.dtype
    assert s.n == len(k.keys) == k.n
    np.testing.assert_array_equal(s.distinct_functions, k.distinct_functions)
    np.testing.assert_array_equal(s.seqs_with_func, k.seqs_with_func)
    assert (s.n_seqs_with_signature, s.distinct_signatures, s.n_windows, s.n_records) == \
        (k.n_seqs_with_signature, k.distinct_signatures, k.n_windows, k.n_records)


@pytest.mark.parametrize("collide", [False, True])
def test_stats_equal_finish(skm, c1, collide):
    r, o, l, f, i = c1["inputs"]
    if collide:  # every sequence under one seq id: n_seqs_with_signature counts distinct ids
        i = np.full(len(i), 7, np.uint32)
    b = builder_of(skm, (r, o, l, f, i), c1["nf"])
    s0 = b.stats()             # runs the build itself, as finish() does
    k = b.finish()
    assert_stats_equal_finish(s0, k)
    assert_stats_equal_finish(b.stats(), k)
    assert k.n_seqs_with_signature == (1 if collide else c1["kept"].n_seqs_with_signature)
    assert k.n_seqs_with_signature > 0 and k.distinct_signatures == len(k.keys) and k.n_records > len(k.keys)
    db = b.kept_db(release_work=True)
    assert_stats_equal_finish(b.stats(), k)
    assert_stats_equal_finish(b.stats(), b.finish())
    db.close()
    b.close()


# ---- 8. errors ----
def test_io_error_leaves_the_handle_usable(skm, c1, tmp_path):
    b = c1["builder"]
    bad = str(tmp_path / "no_such_dir" / "final.kmers")
    with pytest.raises(skm.SkmError, match="error -4") as e:
        b.write_final_kmers(bad)
    assert bad in str(e.value)
    assert not os.path.exists(os.path.dirname(bad))
    k = b.finish()
    np.testing.assert_array_equal(k.keys, c1["kept"].keys)
    np.testing.assert_array_equal(k.data.view(np.uint8), c1["kept"].data.view(np.uint8))
    got, _ = write(b, tmp_path / "good.kmers")
    assert got == c1["want"]


def test_more_than_one_rank_is_refused_before_anything_runs(skm, c1, tmp_path):
    p = str(tmp_path / "final.kmers")
    b = builder_of(skm, c1["inputs"], c1["nf"], rank=0, world_size=2)
    with pytest.raises(skm.SkmError, match="error -6"):
        b.write_final_kmers(p)
    assert not os.path.exists(p)
    with pytest.raises(skm.SkmError, match="error -6"):
        b.stats()
    b.close()
