"""Shared by the device FASTA parser's tests: inputs that exercise every parser rule, and the
comparison of a FastaTable against the pinned restatement oracle/front_ref.py: parse_fasta."""
import numpy as np

import oracle.front_ref as fr

# every rule of the parser in one short text: junk before the first '>', CRLF lines, a '>' in a
# definition line, '*' inside a line and at a line start, a blank line, lower case, a '>' in
# mid-sequence, a digit and a byte 0x80 in the data, ">>x", a '>' with an empty id followed by
# residues (blank after '>' and newline after '>'), a record without a body, a tab before the
# definition, no trailing newline
RULES_TEXT = (b"junk line\n"
              b">r1 first def > with gt\r\n"
              b"ACDE*FG\r\n"
              b"*HIK\r\n"
              b"\r\n"
              b"lmn>pq\n"
              b"A1B\x80C\n"
              b">>x\nWWWW\n"
              b"> emptyid def\nAAAA\nCCCC\n"
              b">nobody\n\n"  # (without the blank line the next '>' would be a bad data character)
              b">\nGGGG\n"
              b">last\tdef\nTTTT\nVV")
RULES_RECORDS = [(b"r1", b"ACDE*FGHIKlmnpqABC"), (b">x", b"WWWW"), (b"nobody", b""), (b"last", b"TTTTVV")]


def expected(blob: bytes):
    """[(id, seq)] of the kept records of one file."""
    return [(i, s) for i, _, s in fr.parse_fasta(blob)]


def pack(blobs):
    data = np.frombuffer(b"".join(blobs), dtype=np.uint8)
    off = np.zeros(len(blobs) + 1, np.uint64)
    off[1:] = np.cumsum([len(b) for b in blobs], dtype=np.uint64)
    return data, off


def check_table(tab, blobs, want):
    """tab (with residues) is the parse of blobs; want[f] = [(id, seq)] of file f."""
    data, off = pack(blobs)
    counts = np.array([len(w) for w in want], np.uint64)
    file_rec = np.zeros(len(blobs) + 1, np.uint64)
    file_rec[1:] = np.cumsum(counts)
    assert tab.n_files == len(blobs) and tab.n_recs == int(file_rec[-1])
    np.testing.assert_array_equal(tab.file_rec, file_rec)
    recs = [r for w in want for r in w]
    lens = np.array([len(s) for _, s in recs], np.uint32)
    np.testing.assert_array_equal(tab.seq_len, lens)
    assert tab.n_residues == int(lens.sum(dtype=np.uint64))
    assert tab.n_windows == int(np.maximum(lens.astype(np.int64) - 7, 0).sum())
    # the packed layout: record s at pstart[s] = sum over t < s of (len[t] + 1), a 0 after each
    packed = b"".join(s + b"\0" for _, s in recs)
    assert tab.residues is not None and tab.residues.tobytes() == packed
    # hdr_pos: the '>' that opened the record, inside the record's file, the id right after it
    hp = tab.hdr_pos.astype(np.int64)
    assert len(hp) == len(recs)
    if len(hp):
        assert np.all(data[hp] == ord(">"))
        f_of = np.repeat(np.arange(len(blobs)), counts.astype(np.int64))
        assert np.all(hp >= off[f_of].astype(np.int64)) and np.all(hp < off[f_of + 1].astype(np.int64))
        assert np.all(np.diff(hp) > 0)
        raw = data.tobytes()
        for p, (rid, _) in zip(hp.tolist(), recs):
            q, span = p + 1, len(rid)
            while raw[q:q + span].count(b"\r") + len(rid) > span:  # '\r' is dropped from an id
                span = raw[q:q + span].count(b"\r") + len(rid)
            assert raw[q:q + span].replace(b"\r", b"") == rid, (p, rid)
