"""Shared by the tests of skm_build_add_fasta (the build's input parsed and selected on the device):
the selected layout restated in Python from oracle/front_ref.py: parse_fasta and a mask, a
position-tracking restatement of the parser to prove where a planted input's records fall in the
kernel's tiles, and the planted inputs themselves."""
import numpy as np

import fasta_device_util as fu

UNDEF = 0xFFFF
TILE, WAVE = 4096, 1024  # skm_fasta_parse_info (checked by the tests that use them)
META_DTYPE = np.dtype([("pstart", np.uint64), ("len", np.uint32), ("func", np.uint16), ("pad", np.uint16)])
AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)


# ------------------------------------------------------------------ the selected layout
class Layout:
    """What the build holds after the selected records of `recs` ([(id, seq)] per parser record, in
    order) were added at packed offset `base` as sequences `first`, first + 1, ...: the packed bytes
    (residues and a 0 after each), the sequence table, the windows."""

    def __init__(self, recs, func, rec_id=None, base=0, first=0):
        func = np.asarray(func, np.uint16)
        assert len(func) == len(recs)
        keep = [r for r in range(len(recs)) if func[r] != UNDEF]
        self.keep = np.array(keep, np.int64)
        seqs = [recs[r][1] for r in keep]
        self.packed = b"".join(s + b"\0" for s in seqs)
        self.lens = np.array([len(s) for s in seqs], np.uint32)
        self.pstart = np.zeros(len(seqs), np.uint64)
        if len(seqs):
            self.pstart[1:] = np.cumsum(self.lens[:-1].astype(np.uint64) + np.uint64(1))
        self.meta = np.zeros(len(seqs), META_DTYPE)
        self.meta["pstart"] = self.pstart + np.uint64(base)
        self.meta["len"] = self.lens
        self.meta["func"] = func[self.keep] if len(keep) else np.zeros(0, np.uint16)
        self.windows = int(np.maximum(self.lens.astype(np.int64) - 7, 0).sum())
        self.seq_id = (np.arange(first, first + len(seqs), dtype=np.uint32) if rec_id is None
                       else np.asarray(rec_id, np.uint32)[self.keep])
        # the same selection as skm_build_add_batch takes it from the host parse
        self.res = np.frombuffer(b"".join(seqs), np.uint8) if seqs else np.zeros(0, np.uint8)
        self.off = np.zeros(len(seqs), np.uint64)
        if len(seqs):
            self.off[1:] = np.cumsum(self.lens[:-1], dtype=np.uint64)


def records_of(blobs):
    """[(id, seq)] of the parser records (non-empty id) of the files, in file order."""
    return [r for b in blobs for r in fu.expected(b)]


def mask_func(n, mask, n_functions=3):
    """rec_func of n parser records under a named mask; selected records get functions 0, 1, 2, 0, ..."""
    sel = {"all": np.ones(n, bool), "none": np.zeros(n, bool), "first": np.arange(n) == 0,
           "last": np.arange(n) == n - 1, "alternating": np.arange(n) % 2 == 0,
           "alternating_odd": np.arange(n) % 2 == 1}[mask]
    f = (np.arange(n) % n_functions).astype(np.uint16)
    f[~sel] = UNDEF
    return f


# ------------------------------------------------------------------ where records fall
def trace(blob: bytes):
    """The parser restated with positions: per parser record (non-empty id) the position of its id's
    first byte and the positions of its residues.  Checked against parse_fasta on every call, so it
    claims nothing parse_fasta does not."""
    out = []
    st = 0  # 0 start, 1 id, 2 defline, 3 data, 4 id_or_data (the states of front_ref.parse_fasta)
    cur = None
    for p, c in enumerate(blob):
        if c == 13:
            continue
        if st == 0:
            if c == 62:
                st, cur = 1, dict(id_pos=-1, res=[])
        elif st == 1:
            if c in (32, 9):
                st = 2
            elif c == 10:
                st = 3
            else:
                if cur["id_pos"] < 0:
                    cur["id_pos"] = p
                    out.append(cur)
        elif st == 2:
            if c == 10:
                st = 3
        elif st == 3:
            if c == 10:
                st = 4
            elif (65 <= (c & ~32) <= 90 and c < 128) or c == 42:
                cur["res"].append(p)
        else:
            if c == 62:
                st, cur = 1, dict(id_pos=-1, res=[])
            elif c == 10:
                pass
            elif 65 <= (c & ~32) <= 90 and c < 128:
                st = 3
                cur["res"].append(p)
    want = fu.expected(blob)
    assert [bytes(blob[q] for q in r["res"]) for r in out] == [s for _, s in want], "trace disagrees with parse_fasta"
    return out


def tile_facts(blob: bytes, func):
    """(per parser record: (tile, byte in tile) of its id's first byte, first and last tile holding one
    of its residues or None; per tile: the selected events -- selected residues + selected record
    starts -- the kernel's output bytes of that tile)."""
    tr = trace(blob)
    assert len(tr) == len(func)
    nt = (len(blob) + TILE - 1) // TILE
    ev = np.zeros(nt, np.int64)
    recs = []
    for r, f in zip(tr, func):
        res = r["res"]
        recs.append(dict(start=(r["id_pos"] // TILE, r["id_pos"] % TILE),
                         res_tiles=(res[0] // TILE, res[-1] // TILE) if res else None, selected=f != UNDEF))
        if f != UNDEF:
            ev[r["id_pos"] // TILE] += 1
            for q in res:
                ev[q // TILE] += 1
    return recs, ev


# ------------------------------------------------------------------ planted inputs
def _body(n, seed, width=60):
    seq = AA[np.random.default_rng(seed).integers(0, 20, size=n)].tobytes()
    return seq, b"".join(seq[c:c + width] + b"\n" for c in range(0, n, width))


def _pad_to(text: bytes, pos: int) -> bytes:
    """text, then '\\r' (ignored in every state) up to length pos"""
    assert len(text) <= pos, (len(text), pos)
    return text + b"\r" * (pos - len(text))


def planted_cases():
    """{name: (blob, rec_func)}: one file each; the edge each case holds is proven from its bytes by
    tests/test_build_fasta_cpu.py: test_planted_inputs_hold_their_edges."""
    c = {}
    head = b">p0\nACDEFGHIKLMNP\n"
    tail = b">z9\nWWWWYYYYHHHHKKKK\n"
    # the id's first byte at tile byte 0 / 4095 (its '>' one byte before)
    c["id_at_tile_byte_0"] = (_pad_to(head, TILE - 1) + b">q1\nMNPQRSTVWYAC\n" + tail, [0, 1, 2])
    c["id_at_tile_byte_4095"] = (_pad_to(head, TILE - 2) + b">q1\nMNPQRSTVWYAC\n" + tail, [0, 1, 2])
    # a selected record whose header ends with its tile: the body starts in the next one
    hdr = b">q2 a definition line\n"
    c["body_in_next_tile"] = (_pad_to(head, 2 * TILE - len(hdr)) + hdr + b"GHIKLMNPQRSTV\nACDEFG\n" + tail, [0, 1, 2])
    # a record over three whole tiles (and parts of the two around them), unselected between two
    # selected ones, then selected
    _, body = _body(4 * TILE, seed=11)
    long_blob = _pad_to(head, TILE - 300) + b">long\n" + body + tail
    c["unselected_over_three_tiles"] = (long_blob, [0, UNDEF, 2])
    c["selected_over_three_tiles"] = (long_blob, [UNDEF, 1, UNDEF])
    c["selected_over_three_tiles_all"] = (long_blob, [0, 1, 2])
    # tile 1 is record starts only, as densely as the grammar allows: 1024 records ">a\n\n" (the
    # blank line takes the parser from the data state, where a '>' is a bad data character, to a line
    # start, where it opens a record); residues before and after them
    many = _pad_to(head, TILE) + b">a\n\n" * 1024 + b">b\nCDEFGHIKLMNPQ\n" + tail
    n = 1 + 1024 + 1 + 1
    c["tile_of_starts_all"] = (many, mask_func(n, "all"))
    c["tile_of_starts_none"] = (many, mask_func(n, "none"))
    c["tile_of_starts_alternating"] = (many, mask_func(n, "alternating"))
    c["tile_of_starts_alternating_odd"] = (many, mask_func(n, "alternating_odd"))
    # tile 1 is ">a\n" 1365 times and a '>': every second '>' stands in the data state and is
    # dropped and the 'a' after it is a residue, so these are 683 records "a" of one residue, a start
    # or a residue on every third byte
    lit = _pad_to(head, TILE) + b">a\n" * 1366 + b"CDEFGHIKLMNPQ\n" + tail
    c["tile_of_gt_a_nl_all"] = (lit, mask_func(685, "all"))
    c["tile_of_gt_a_nl_alternating"] = (lit, mask_func(685, "alternating"))
    # (the selection leaves out every record of tile 1, and the record before and after it: the tile's
    # output is 0 bytes while R and S advance on every third byte)
    none = mask_func(685, "none")
    none[0], none[684] = 0, 1
    c["tile_of_gt_a_nl_none"] = (lit, none)
    c["tile_of_gt_a_nl_none_at_all"] = (lit, mask_func(685, "none"))
    # a line without a newline over three tiles: tiles 1 and 2 are 4096 residues each, the most a
    # tile can put out
    w = _pad_to(head, TILE - 100) + b">w\n" + _body(3 * TILE, seed=13)[0] + b"\n" + tail
    c["unwrapped_line_selected"] = (w, [UNDEF, 1, 2])
    c["unwrapped_line_all"] = (w, [0, 1, 2])
    # tile 1 gives no output (an unselected record's residues), tiles 0 and 2 do
    _, body2 = _body(TILE + 600, seed=12)
    c["empty_tile_between"] = (_pad_to(head, TILE - 200) + b">u\n" + body2 + tail, [0, UNDEF, 1])
    return {k: (b, np.asarray(f, np.uint16)) for k, (b, f) in c.items()}
