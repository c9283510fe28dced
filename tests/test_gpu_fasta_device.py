"""The device FASTA parser (skm_fasta.hip) against the reference's own parser output
(tests/golden/ref_fasta.npz) and the pinned restatement oracle/front_ref.py: parse_fasta, at the
kernel's chunk boundaries, and as the front of a resident annotate query."""
import os

import numpy as np
import pytest

import fasta_device_util as fu
from conftest import TESTS

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ 1. the reference's vectors
@pytest.fixture(scope="module")
def ref_vectors():
    z = np.load(os.path.join(TESTS, "golden", "ref_fasta.npz"))
    un = lambda h: b"" if h == "-" else bytes.fromhex(h)  # noqa: E731
    blobs, want = [], []
    for k in range(len(z["blob_off"]) - 1):
        blobs.append(z["blobs"][z["blob_off"][k]:z["blob_off"][k + 1]].tobytes())
        recs = []
        for ln in z["out"][z["out_off"][k]:z["out_off"][k + 1]].tobytes().decode().splitlines():
            c = ln.split(" ")
            if c[0] == "R" and un(c[1]):  # callers skip records with an empty id
                recs.append((un(c[1]), un(c[3])))
        want.append(recs)
    assert len(blobs) == 1821 and any(len(b) == 0 for b in blobs)
    return blobs, want


@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_reference_vectors_in_one_call(skm, gpu, ref_vectors, order):
    blobs, want = ref_vectors
    if order == "reverse":  # every blob meets other chunk offsets
        blobs, want = blobs[::-1], want[::-1]
    tab = skm.fasta_parse_device(blobs, want_residues=True)
    fu.check_table(tab, blobs, want)
    assert tab.n_recs > 1000 and tab.parse_ms > 0


# ------------------------------------------------------------------ 2. boundary sweep
def _sweep_offsets(skm):
    _, w, t = skm.fasta_parse_info()
    ii = set(range(0, 2 * w + 1))
    for k in (1, 2):
        ii |= set(range(k * t - w, k * t + w + 1))
    return sorted(ii), w, t


def _same_records_as(tab, pstart, f, f0, shift):
    """file f of tab holds file f0's records, its header positions `shift` bytes further on"""
    a, b = int(tab.file_rec[f]), int(tab.file_rec[f + 1])
    a0, b0 = int(tab.file_rec[f0]), int(tab.file_rec[f0 + 1])
    if b - a != b0 - a0:
        return False
    return (np.array_equal(tab.seq_len[a:b], tab.seq_len[a0:b0])
            and np.array_equal(tab.residues[pstart[a]:pstart[b]], tab.residues[pstart[a0]:pstart[b0]])
            and np.array_equal(tab.hdr_pos[a:b].astype(np.int64), tab.hdr_pos[a0:b0].astype(np.int64) + shift))


def test_text_start_at_every_chunk_boundary(skm, gpu):
    """The rules text after i bytes of '\\r' (ignored in every state), one file per i, all in one
    call: every file parses to file 0's records, and file 0's are the restatement's."""
    offsets, _, _ = _sweep_offsets(skm)
    assert offsets[0] == 0
    blobs = [b"\r" * i + fu.RULES_TEXT for i in offsets]
    data, off = fu.pack(blobs)
    tab = skm.fasta_parse_device((data, off), want_residues=True)
    want0 = fu.expected(fu.RULES_TEXT)
    assert want0 == fu.RULES_RECORDS
    fu.check_table(tab, blobs, [want0] * len(blobs))  # (also compares every file with the restatement)
    pstart = np.zeros(tab.n_recs + 1, np.int64)
    pstart[1:] = np.cumsum(tab.seq_len.astype(np.int64) + 1)
    bad = [i for f, i in enumerate(offsets) if not _same_records_as(tab, pstart, f, 0, int(off[f]) + i)]
    assert not bad, bad[:20]


def test_file_boundary_at_every_chunk_boundary(skm, gpu):
    """Pairs of files (the first ends in mid-record, the second starts with what would continue
    it) placed so that the boundary between them falls at every offset of the sweep."""
    offsets, w, t = _sweep_offsets(skm)
    first = b">a1 d\r\nACDEFGHIKL\nMNP"                      # ends inside a sequence line
    second = b"QRS\n>b1\nTTTT\n>\nWWW\n>b2 x\nYYYYYYYYY"       # "QRS" is junk before this file's first '>'
    period = 4 * t
    assert period > offsets[-1]
    stride = len(first) + len(second)
    blobs, cur = [], 0
    for i in sorted(offsets, key=lambda i: (i % stride, i)):     # little padding between pairs
        pad = (i - cur - len(first)) % period
        blobs += [b"\r" * pad + first, second]
        cur += pad + stride
        assert (cur - len(second)) % period == i
    data, off = fu.pack(blobs)
    assert len(data) < 64 << 20
    tab = skm.fasta_parse_device((data, off), want_residues=True)
    wa, wb = fu.expected(first), fu.expected(second)
    assert wa == [(b"a1", b"ACDEFGHIKLMNP")] and wb == [(b"b1", b"TTTT"), (b"b2", b"YYYYYYYYY")]
    fu.check_table(tab, blobs, [wa, wb] * (len(blobs) // 2))


# ------------------------------------------------------------------ 3. fuzz
def test_fuzz_against_the_restatement(skm, gpu):
    rng = np.random.default_rng(20240611)
    alphabet = np.frombuffer(b">\n\r \tAc*1-\x80", dtype=np.uint8)
    # '>' , '\n' and letters a little more often than the rest, so that records form
    p = np.array([3, 4, 1, 1, 1, 4, 4, 1, 1, 1, 1], float)
    blobs = [alphabet[rng.choice(len(alphabet), size=int(n), p=p / p.sum())].tobytes()
             for n in rng.integers(0, 301, size=5000)]
    want = [fu.expected(b) for b in blobs]
    assert sum(len(w) for w in want) > 2000 and any(not w for w in want)
    tab = skm.fasta_parse_device(blobs, want_residues=True)
    fu.check_table(tab, blobs, want)


# ------------------------------------------------------------------ 4. long records, many records
def test_long_and_tiny_records(skm, gpu):
    rng = np.random.default_rng(7)
    aa = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
    seq = aa[rng.integers(0, 20, size=200_000)].tobytes()
    wrapped = b">long one\n" + b"".join(seq[c:c + 59] + b"\n" for c in range(0, len(seq), 59))  # 60-byte lines
    single = b">single\n" + seq                                                               # no final newline
    tiny_lens = rng.integers(0, 4, size=20_000)
    tiny = b"".join(b">t%d\n%s\n" % (k, seq[k:k + n]) for k, n in enumerate(tiny_lens.tolist()))
    blobs = [wrapped, single, tiny]
    want = [fu.expected(b) for b in blobs]
    assert want[0] == [(b"long", seq)] and want[1] == [(b"single", seq)] and len(want[2]) == 20_000
    tab = skm.fasta_parse_device(blobs, want_residues=True)
    fu.check_table(tab, blobs, want)


# ------------------------------------------------------------------ 5./6. a resident query
@pytest.fixture(scope="module")
def small_db(skm, gpu, tmp_path_factory):
    from signature_kmers_amd import synth
    p = synth.generate_arrays(3000, 40, per_file=500, seed=17)
    r, o, l, f, i, funcs = synth.build_inputs(p)
    b = skm.SignatureBuilder(len(funcs), device=0)
    b.add_batch(r, o, l, f, i)
    kept = b.finish()
    b.close()
    base = str(tmp_path_factory.mktemp("fasta_db") / "kmer_data")
    skm.mph_build(kept.keys, kept.data, base + ".mph", base + ".dat", seed=1)
    assert len(kept.keys) > 1000
    return base, funcs


def _query_files(n_seqs, seed):
    """FASTA files of fresh sequences of the DB's families (with '*', 'X' and short ones), and the
    host-parsed arrays of their kept records"""
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


def _host_arrays(blobs):
    seqs = [s for b in blobs for _, s in fu.expected(b)]
    lens = np.array([len(s) for s in seqs], np.uint32)
    off = np.zeros(len(seqs), np.uint64)
    if len(seqs):
        off[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    return np.frombuffer(b"".join(seqs), dtype=np.uint8), off, lens


def _hypo(funcs):
    return funcs.index("hypothetical protein")


@pytest.mark.parametrize("case", ["files", "no_kept_records", "no_files"])
def test_query_from_fasta_equals_query_from_arrays(skm, gpu, small_db, case):
    base, funcs = small_db
    db = skm.CmphKmerDb(base, device=0)
    if case == "files":
        blobs, (res, off, lens) = _query_files(1500, seed=17)
        blobs = blobs[:2] + [b""] + blobs[2:]  # an empty file among them
    else:
        blobs = [b"junk only\n", b">\nACDEFGHIKLMNP\n", b""] if case == "no_kept_records" else []
        res, off, lens = _host_arrays(blobs)
    host = skm.QueryBatch(db, res, off, lens)
    dev = skm.QueryBatch.from_fasta(db, blobs)
    assert dev.table.n_files == len(blobs) and dev.table.n_recs == len(lens)
    np.testing.assert_array_equal(dev.table.seq_len, lens)
    assert dev.table.n_windows == int(np.maximum(lens.astype(np.int64) - 7, 0).sum())
    for q in (host, dev):
        q.run(_hypo(funcs))
    (hoff, hcalls), (doff, dcalls) = host.calls(), dev.calls()
    np.testing.assert_array_equal(doff, hoff)
    assert dcalls.tobytes() == hcalls.tobytes()
    for a, b in zip(dev.window_hits(), host.window_hits()):
        np.testing.assert_array_equal(a, b)
    if case == "files":
        assert len(hcalls) > 100 and len(host.window_hits()[1]) > 1000
        dev.run(_hypo(funcs), ignore_hypo=True)  # an ordinary query: it runs again without a new parse
        host.run(_hypo(funcs), ignore_hypo=True)
        assert dev.calls()[1].tobytes() == host.calls()[1].tobytes()
    else:
        assert len(lens) == 0 and len(dcalls) == 0
    host.close()
    dev.close()
    db.close()


def test_annotate_fasta_reuses_the_dbs_query(skm, gpu, small_db):
    """skm_annotate_fasta on a large then a small batch, plain skm_annotate, skm_annotate_fasta
    again -- one DB, each result the host path's (a second DB handle) for the same input."""
    base, funcs = small_db
    db, db_host = skm.CmphKmerDb(base, device=0), skm.CmphKmerDb(base, device=0)
    caller, host = skm.FunctionCaller(db, funcs), skm.FunctionCaller(db_host, funcs)
    large, small = _query_files(1500, seed=17), _query_files(250, seed=17)
    assert len(large[1][2]) > 4 * len(small[1][2]) > 0

    def check_fasta(blobs, arrays):
        file_rec, seq_len, hdr_pos, off, calls = caller.process_fasta(blobs)
        hoff, hcalls = host.process_seqs(*arrays)
        np.testing.assert_array_equal(seq_len, arrays[2])
        assert int(file_rec[-1]) == len(arrays[2]) == len(hdr_pos)
        np.testing.assert_array_equal(off, hoff)
        assert calls.tobytes() == hcalls.tobytes() and len(calls) > 0

    check_fasta(*large)
    check_fasta(*small)
    off, calls = caller.process_seqs(*large[1])  # plain skm_annotate on the same DB
    hoff, hcalls = host.process_seqs(*large[1])
    np.testing.assert_array_equal(off, hoff)
    assert calls.tobytes() == hcalls.tobytes()
    check_fasta(*small)
    check_fasta(*large)
    db.close()
    db_host.close()
