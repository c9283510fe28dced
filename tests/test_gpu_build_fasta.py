"""skm_build_add_fasta (SignatureBuilder.add_fasta): the build's input parsed and selected on the
device.  The resident input (debug_input) against the Python restatement of the selected layout
(build_fasta_util.Layout over oracle/front_ref.py: parse_fasta) and against a second handle fed the
same selection through add_batch; the kernel's tile edges; every alignment of the destination; the
build's results; the errors."""
import os

import numpy as np
import pytest

import build_fasta_util as bu
import fasta_device_util as fu
import oracle_ref
from conftest import TESTS
from signature_kmers_amd import synth

pytestmark = pytest.mark.gpu

UNDEF = bu.UNDEF
NF = 3


def input_of(b):
    b.prepare()
    res, meta = b.debug_input()
    return res.tobytes(), meta.view(np.uint8).tobytes(), b.resident_seqs(), b.counters()["windows"]


def check_table(tab, blobs, recs):
    """the table over every parser record, selected or not"""
    data, off = fu.pack(blobs)
    assert tab.n_files == len(blobs) and tab.n_recs == len(recs) and tab.residues is None
    np.testing.assert_array_equal(tab.seq_len, np.array([len(s) for _, s in recs], np.uint32))
    assert tab.n_residues == sum(len(s) for _, s in recs)
    assert tab.n_windows == sum(max(len(s) - 7, 0) for _, s in recs)
    hp = tab.hdr_pos.astype(np.int64)
    assert np.all(data[hp] == ord(">")) and np.all(np.diff(hp) > 0)
    assert tab.file_rec[0] == 0 and tab.file_rec[-1] == len(recs) and np.all(np.diff(tab.file_rec.astype(np.int64)) >= 0)
    f_of = np.searchsorted(tab.file_rec.astype(np.int64), np.arange(len(recs)), side="right") - 1
    assert np.all(hp >= off[f_of].astype(np.int64)) and np.all(hp < off[f_of + 1].astype(np.int64))


def check_layout(skm, blobs, func, recs=None, rec_id=None):
    """add_fasta + prepare gives the restatement byte for byte, and what add_batch gives for the same
    selection from the host parse"""
    recs = bu.records_of(blobs) if recs is None else recs
    func = np.asarray(func, np.uint16)
    lay = bu.Layout(recs, func, rec_id)
    b = skm.SignatureBuilder(NF, device=0)
    tab = b.add_fasta(blobs, func, rec_id)
    got = input_of(b)
    b.close()
    check_table(tab, blobs, recs)
    assert got[0] == lay.packed
    assert got[1] == lay.meta.view(np.uint8).tobytes()
    assert got[2] == (len(lay.lens), len(lay.packed)) and got[3] == lay.windows
    h = skm.SignatureBuilder(NF, device=0)
    h.add_batch(lay.res, lay.off, lay.lens, lay.meta["func"], lay.seq_id)
    want = input_of(h)
    h.close()
    assert got == want
    return lay


# ------------------------------------------------------------------ 1. layout
@pytest.mark.parametrize("mask", ["all", "none", "first", "last", "alternating", "alternating_odd"])
def test_rules_text_under_masks(skm, gpu, mask):
    check_layout(skm, [fu.RULES_TEXT], bu.mask_func(4, mask))


@pytest.mark.parametrize("r", range(4))
def test_rules_text_each_record_alone_and_left_out(skm, gpu, r):
    """every rule of the parser with the record that holds it unselected, then the only one selected"""
    alone = np.full(4, UNDEF, np.uint16)
    alone[r] = 1
    left_out = bu.mask_func(4, "all")
    left_out[r] = UNDEF
    for f in (alone, left_out):
        check_layout(skm, [fu.RULES_TEXT, b"\r\r" + fu.RULES_TEXT], np.concatenate([f, f[::-1]]))


def test_reference_vectors_a_third_unselected(skm, gpu):
    """the reference parser's own outputs (tests/golden/ref_fasta.npz) as the expectation"""
    z = np.load(os.path.join(TESTS, "golden", "ref_fasta.npz"))
    un = lambda h: b"" if h == "-" else bytes.fromhex(h)  # noqa: E731
    blobs, recs = [], []
    for k in range(len(z["blob_off"]) - 1):
        blobs.append(z["blobs"][z["blob_off"][k]:z["blob_off"][k + 1]].tobytes())
        for ln in z["out"][z["out_off"][k]:z["out_off"][k + 1]].tobytes().decode().splitlines():
            c = ln.split(" ")
            if c[0] == "R" and un(c[1]):
                recs.append((un(c[1]), un(c[3])))
    assert len(recs) > 1000
    rng = np.random.default_rng(3)
    func = rng.integers(0, NF, size=len(recs)).astype(np.uint16)
    func[rng.random(len(recs)) < 1 / 3] = UNDEF
    lay = check_layout(skm, blobs, func, recs=recs, rec_id=np.arange(len(recs), dtype=np.uint32) * 3 + 5)
    assert 0 < len(lay.lens) < len(recs)


@pytest.mark.parametrize("case", ["empty_ids_between", "zero_length", "no_record", "no_files", "no_final_newline"])
def test_layout_cases(skm, gpu, case):
    if case == "empty_ids_between":  # not parser records: no rec_func entry, their residues go nowhere
        blobs = [b">a\nACDEFGHIK\n>\nWWWW\n> d\nWWWWW\n>b\nLMNPQRSTV\n>\nWWW", b">\nWW\n>c x\nYYACDEFGHI\n"]
        for f in ([0, 1, 2], [0, UNDEF, 2], [UNDEF, 1, UNDEF]):
            lay = check_layout(skm, blobs, f)
            assert b"W" not in lay.packed
    elif case == "zero_length":
        blobs = [b">a\n\n>b\n\n>c\nACDEFGHIKL\n>d\n\n>e\n", b">f\n", b">g\nMN\n>h\n\n"]
        for m in ("all", "alternating", "alternating_odd", "first", "last"):
            lay = check_layout(skm, blobs, bu.mask_func(8, m))
            assert 0 in lay.lens.tolist()
    elif case == "no_record":
        check_layout(skm, [b"junk only\nno record here\n"], [])
        check_layout(skm, [b">a\nACDEFGHIKLMN\n", b"", b"junk\n", b">\nWWWW\n", b">b\nPQRSTVWY\n"], [1, 2])
    elif case == "no_files":
        check_layout(skm, [], [])
    else:
        for m in ("all", "last", "first"):
            check_layout(skm, [b">a\nACDEFGHIKLMN\n>b\nPQRSTVWYAC", b">c\nDEFGHIKLM\nNPQ"], bu.mask_func(3, m))


# ------------------------------------------------------------------ 2. tile edges
@pytest.mark.parametrize("name", sorted(bu.planted_cases()))
def test_planted_tile_edges(skm, gpu, name):
    """(what edge each input holds is proven in tests/test_build_fasta_cpu.py)"""
    assert skm.fasta_parse_info()[1:] == (bu.WAVE, bu.TILE)
    blob, func = bu.planted_cases()[name]
    check_layout(skm, [blob], func)
    # the same file after another one: every tile gets a nonzero base in both scans
    other = b">o1\nACDEFGHIKLMNPQRSTVWY\n" + b"\r" * (bu.TILE - 24)
    check_layout(skm, [other, blob], np.concatenate([[2], func]).astype(np.uint16))


@pytest.mark.parametrize("mask", ["alternating", "alternating_odd"])
def test_text_start_at_every_chunk_boundary_selected(skm, gpu, mask):
    """the sweep of test_gpu_fasta_device.py: test_text_start_at_every_chunk_boundary (the rules text
    after i bytes of '\\r', one file per i) under an alternating selection"""
    _, w, t = skm.fasta_parse_info()
    ii = set(range(0, 2 * w + 1))
    for k in (1, 2):
        ii |= set(range(k * t - w, k * t + w + 1))
    blobs = [b"\r" * i + fu.RULES_TEXT for i in sorted(ii)]
    recs = fu.RULES_RECORDS * len(blobs)  # '\r' is dropped in every state
    assert bu.records_of(blobs[:3] + blobs[-2:]) == fu.RULES_RECORDS * 5
    func = bu.mask_func(len(recs), mask)
    b = skm.SignatureBuilder(NF, device=0)
    tab = b.add_fasta(blobs, func)
    got = input_of(b)
    b.close()
    lay = bu.Layout(recs, func)
    assert tab.n_recs == len(recs) and np.array_equal(tab.file_rec, np.arange(len(blobs) + 1) * 4)
    assert got[0] == lay.packed and got[1] == lay.meta.view(np.uint8).tobytes()
    assert got[2] == (len(lay.lens), len(lay.packed)) and got[3] == lay.windows


# ------------------------------------------------------------------ 3. destination alignment
FILES_A = [fu.RULES_TEXT, b">s1\nACDEFGHIKLMNPQRSTVWY\n>s2\nWYWYWYWYW\n"]
FILES_B = [b">t1\nMNPQRSTVW\n>t2\n\n>t3\nACDEFGHIKL\nMNPQRSTVWY\nAC"]
FUNC_A, FUNC_B = [0, UNDEF, 1, 2, UNDEF, 0], [1, 2, 0]


def _first(k):
    """one sequence of k residues: the next one starts at packed offset k + 1"""
    seq = bytes(bu.AA[np.arange(k) % 20])
    return (np.frombuffer(seq, np.uint8), np.zeros(1, np.uint64), np.array([k], np.uint32), np.array([1], np.uint16),
            np.array([0], np.uint32)), seq + b"\0"


def _expect(parts):
    """parts: [(recs, func)] added one after the other"""
    packed, metas, windows = b"", [], 0
    for recs, func in parts:
        lay = bu.Layout(recs, func, base=len(packed))
        packed += lay.packed
        metas.append(lay.meta)
        windows += lay.windows
    meta = np.concatenate(metas)
    return packed, meta.view(np.uint8).tobytes(), (len(meta), len(packed)), windows


def test_every_alignment_two_add_fasta_calls(skm, gpu):
    ra, rb = bu.records_of(FILES_A), bu.records_of(FILES_B)
    seen = set()
    for k in range(16):
        first, _ = _first(k)
        b = skm.SignatureBuilder(NF, device=0)
        b.add_batch(*first)
        seen.add(b.resident_seqs()[1] % 16)
        b.add_fasta(FILES_A, FUNC_A)
        b.add_fasta(FILES_B, FUNC_B)
        got = input_of(b)
        b.close()
        assert got == _expect([([(b"x", first[0].tobytes())], [1]), (ra, FUNC_A), (rb, FUNC_B)]), k
    assert seen == set(range(16))


def test_every_alignment_interleaved_with_add_batch(skm, gpu):
    """add_batch / add_fasta / add_batch: the staging buffer is partly filled when add_fasta is
    called, and again after it"""
    ra = bu.records_of(FILES_A)
    lb = bu.Layout(bu.records_of(FILES_B), FUNC_B)
    for k in range(16):
        first, _ = _first(k)
        b = skm.SignatureBuilder(NF, device=0)
        b.add_batch(*first)
        b.add_fasta(FILES_A, FUNC_A)
        b.add_batch(lb.res, lb.off, lb.lens, lb.meta["func"])
        b.add_fasta(FILES_B, FUNC_B)
        got = input_of(b)
        b.close()
        want = _expect([([(b"x", first[0].tobytes())], [1]), (ra, FUNC_A), (bu.records_of(FILES_B), FUNC_B),
                        (bu.records_of(FILES_B), FUNC_B)])
        assert got == want, k


@pytest.mark.parametrize("k", [5, 15])
def test_resident_buffer_grows_inside_the_call(skm, gpu, k):
    """no reserve: the first allocation is 64 MB, the call needs more and has to keep what is there
    (k = 15: the destination is 16-byte aligned)"""
    first, _ = _first(k)
    rng = np.random.default_rng(9)
    lens = np.full(100, 1_000_000, np.uint32)
    lens[::7] = 999_983
    res = bu.AA[rng.integers(0, 20, size=int(lens.sum()))]
    ids = [b"big%d" % k for k in range(len(lens))]
    blob = synth.fasta_bytes(ids, res, lens)
    func = bu.mask_func(len(lens), "all")
    func[3::5] = UNDEF
    ends = np.cumsum(lens.astype(np.int64))
    raw = res.tobytes()
    recs = [(ids[k], raw[ends[k] - lens[k]:ends[k]]) for k in range(len(lens))]
    want = _expect([([(b"x", first[0].tobytes())], [1]), (recs, func)])
    assert want[2][1] > 64 << 20
    b = skm.SignatureBuilder(NF, device=0)
    b.add_batch(*first)
    tab = b.add_fasta([blob], func)
    got = input_of(b)
    b.close()
    np.testing.assert_array_equal(tab.seq_len, lens)
    assert got[1:] == want[1:]
    assert got[0] == want[0]


# ------------------------------------------------------------------ 4. results
@pytest.fixture(scope="module")
def synth_set():
    """about 2,000 proteins with 'X' / '*' among them in files of 250, a third unselected at random;
    the oracle's build of the selected ones (computed once)"""
    p = synth.generate_arrays(2000, 50, per_file=250, seed=5, extras=True)
    r, o, l, f, i, funcs = synth.build_inputs(p)
    f = f.copy()
    f[np.random.default_rng(21).random(len(f)) < 1 / 3] = UNDEF
    blobs, file_rows = [], []
    for fl in np.unique(p.file_of):
        idx = np.nonzero(p.file_of == fl)[0]
        a, e = int(o[idx[0]]), int(o[idx[-1]] + l[idx[-1]])
        blobs.append(synth.fasta_bytes([b"fig|%d.1.peg.%d" % (fl, k + 1) for k in range(len(idx))], r[a:e], l[idx]))
        file_rows.append(idx)
    ref = oracle_ref.build(r, o, l, f, i, len(funcs))
    assert len(ref["keys"]) > 1000 and (np.isin(r, [ord("X"), ord("*")])).sum() > 0
    return dict(arrays=(r, o, l, f, i), funcs=funcs, blobs=blobs, file_rows=file_rows, ref=ref)


def _same_as_oracle(got, ref):
    np.testing.assert_array_equal(got.keys, ref["keys"])
    np.testing.assert_array_equal(got.data.view(np.uint8), ref["data"].view(np.uint8))
    np.testing.assert_array_equal(got.distinct_functions, ref["distinct_functions"])
    np.testing.assert_array_equal(got.seqs_with_func, ref["seqs_with_func"])
    assert got.n_seqs_with_signature == ref["n_seqs_with_signature"]
    assert got.distinct_signatures == ref["distinct_signatures"]


def _same_kept(a, b):
    np.testing.assert_array_equal(a.keys, b.keys)
    np.testing.assert_array_equal(a.data.view(np.uint8), b.data.view(np.uint8))
    np.testing.assert_array_equal(a.distinct_functions, b.distinct_functions)
    np.testing.assert_array_equal(a.seqs_with_func, b.seqs_with_func)
    assert (a.n_seqs_with_signature, a.distinct_signatures) == (b.n_seqs_with_signature, b.distinct_signatures)


@pytest.mark.parametrize("passes", [0, 4])
def test_build_from_fasta_equals_build_from_arrays_and_the_oracle(skm, gpu, synth_set, passes):
    r, o, l, f, i = synth_set["arrays"]
    nf = len(synth_set["funcs"])
    bf, ba = skm.SignatureBuilder(nf, device=0), skm.SignatureBuilder(nf, device=0)
    for b in (bf, ba):
        if passes:
            b.set_option("key_range_passes", passes)
    tab = bf.add_fasta(synth_set["blobs"], f, i)
    ba.add_batch(r, o, l, f, i)
    np.testing.assert_array_equal(tab.seq_len, l)
    kf, ka = bf.finish(), ba.finish()
    _same_kept(kf, ka)
    _same_as_oracle(kf, synth_set["ref"])
    np.testing.assert_array_equal(bf.signature_flags(), ba.signature_flags())
    cf, ca = bf.counters(), ba.counters()
    assert cf["passes"] == ca["passes"] == (passes or 1)
    for name in ("windows", "valid", "sequences", "kept"):
        assert cf[name] == ca[name], name
    assert cf["windows"] == oracle_ref.count_windows(l, f)
    assert bf.resident_seqs() == ba.resident_seqs() == (int((f != UNDEF).sum()), int(l[f != UNDEF].sum() + (f != UNDEF).sum()))
    assert cf["add_fasta_us"] > 0 and ca["add_fasta_us"] == 0 and cf["add_batch_us"] >= cf["add_fasta_us"] // 2
    if not passes:  # the recall over the resident sequences (one DB serves both handles)
        db = ba.kept_db()
        tables = skm.FunctionIndexTables(synth_set["funcs"], device=0)
        want, got = ba.recall(db, tables), bf.recall(db, tables)
        np.testing.assert_array_equal(got.best.view(np.uint8), want.best.view(np.uint8))
        assert (got.best["fi"] != UNDEF).sum() > 500 and got.stats["n_seqs"] == want.stats["n_seqs"]
        tables.close()
        db.close()
    bf.close()
    ba.close()


def test_two_ranks_each_adding_its_own_files(skm, gpu, synth_set):
    r, o, l, f, i = synth_set["arrays"]
    nf, blobs, rows = len(synth_set["funcs"]), synth_set["blobs"], synth_set["file_rows"]
    half = len(blobs) // 2
    calls = [[(0, half - 1), (half - 1, half)], [(half, len(blobs))]]  # rank 0 adds its last file in a call of its own
    bs = []
    for rank in range(2):
        b = skm.SignatureBuilder(nf, device=0, rank=rank, world_size=2)
        n_sel = 0
        for a, e in calls[rank]:
            idx = np.concatenate(rows[a:e])
            b.add_fasta(blobs[a:e], f[idx], i[idx])
            n_sel += int((f[idx] != UNDEF).sum())
        assert b.resident_seqs()[0] == n_sel > 0
        bs.append(b)
    skm.group_run(bs)
    outs = [b.finish() for b in bs]
    for b in bs:
        b.close()
    _same_as_oracle(outs[0], synth_set["ref"])
    assert outs[1].distinct_signatures == synth_set["ref"]["distinct_signatures"]


# ------------------------------------------------------------------ 5. errors
def _arg_error(skm, call, match):
    with pytest.raises(skm.SkmError, match=r"error -1.*" + match):
        call()


def test_errors_leave_the_handle_as_it_was(skm, gpu):
    """every refusal is SKM_E_ARG, and the build continued on the same handle is the build without
    the refused calls"""
    ra = bu.records_of(FILES_A)
    lb = bu.Layout(bu.records_of(FILES_B), FUNC_B)
    first, _ = _first(6)
    b = skm.SignatureBuilder(NF, device=0)
    b.add_batch(*first)
    _arg_error(skm, lambda: b.add_fasta(FILES_A, FUNC_A[:-1]), "6 records.*describes 5")
    _arg_error(skm, lambda: b.add_fasta(FILES_A, FUNC_A + [0]), "6 records.*describes 7")
    b.add_fasta(FILES_A, FUNC_A)
    _arg_error(skm, lambda: b.add_fasta(FILES_B, [1, NF, 0]), "rec_func out of range")
    b.add_fasta(FILES_B, [1, NF, 0][:1] + [UNDEF, UNDEF])  # (an unselected entry is never range-checked: 0xFFFF)
    data, off = fu.pack(FILES_B)
    _arg_error(skm, lambda: b.add_fasta((data, np.array([0, 9, 4], np.uint64)), [1]), "file_off must ascend")
    _arg_error(skm, lambda: b.add_fasta((data, np.array([1, len(data)], np.uint64)), FUNC_B), r"file_off\[0\]")
    b.prepare()
    before = b.debug_input()
    _arg_error(skm, lambda: b.add_fasta(FILES_A, [0]), "6 records.*describes 1")  # a prepared handle too
    after = b.debug_input()  # (SKM_E_STATE unless the handle is still prepared)
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
    b.add_batch(lb.res, lb.off, lb.lens, lb.meta["func"])
    got = input_of(b)
    b.close()
    rb = bu.records_of(FILES_B)
    want = _expect([([(b"x", first[0].tobytes())], [1]), (ra, FUNC_A), (rb, [1, UNDEF, UNDEF]), (rb, FUNC_B)])
    assert got == want


def test_record_of_2_to_the_20_residues(skm, gpu):
    """a selected record of 1,048,576 residues is refused (the window index has 20 bits), the same
    record unselected is accepted, and so is a selected one of 1,048,575"""
    n = 1 << 20
    seq = bu.AA[np.random.default_rng(4).integers(0, 20, size=n)]
    blob = synth.fasta_bytes([b"a", b"big", b"c"], np.concatenate([bu.AA[:12], seq, bu.AA[:9]]),
                             np.array([12, n, 9], np.uint32))
    small = [(b"a", bu.AA[:12].tobytes()), (b"big", seq.tobytes()), (b"c", bu.AA[:9].tobytes())]
    b = skm.SignatureBuilder(NF, device=0)
    _arg_error(skm, lambda: b.add_fasta([blob], [0, 1, 2]), "1,048,575")
    assert b.resident_seqs() == (0, 0)
    tab = b.add_fasta([blob], [0, UNDEF, 2])
    assert tab.seq_len.tolist() == [12, n, 9]
    got = input_of(b)
    assert got == _expect([(small, [0, UNDEF, 2])])
    blob1 = synth.fasta_bytes([b"big"], seq[:-1], np.array([n - 1], np.uint32))
    b.add_fasta([blob1], [1])
    got = input_of(b)
    b.close()
    assert got == _expect([(small, [0, UNDEF, 2]), ([(b"big", seq[:-1].tobytes())], [1])])
