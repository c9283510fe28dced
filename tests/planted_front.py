"""Planted window layouts for the build's extraction front end -- a plain helper module of the tests.

The front end (k_pass_ids, k_sel_scan, k_pass_emit<G>, k_pass_hist, k_extract_stage_pos<R> with
key-range passes; k_extract, k_extract_stage, k_split_stage, k_blk2seq with one pass) decides which
windows exist, which pass, bucket and sequence each belongs to, and at which offset.  A Layout holds
filler proteins of X and writes residue islands at chosen absolute positions of the packed residue
buffer (every kept sequence followed by one separator byte, the sequences with the undefined
function left out -- the buffer the kernels read), so a window can be put on a chosen emission row,
tile, chunk and lane byte.  Islands come from one seeded generator and no 8-mer repeats across
islands, so every window is a singleton: always kept, its avg_from_end = (len - i) mod 2^16 and its
function name the window's offset and sequence, and a bit-for-bit compare with the oracle sees
every lost, extra or misplaced window.  The only repeated 8-mers are the declared homopolymers.

The geometry restated here (skm_build.hip: size_local, prepare_local, set_geometry):
  rp        = sum of len + 1 over the sequences with a defined function
  sel_wg    = max(SEL_WG, ceil(rp / (2^REL_BITS - 16)))        emission rows
  sel_span  = 16 * ceil(ceil(rp / sel_wg) / 16)                windows per emission row
  k_pass_emit walks a row in tiles of TILE = 64 lanes x CHUNK windows; a lane loads LANE_BYTES.
test_planted_front_cpu.py proves the layouts are what they claim from the packed arrays alone."""
import functools

import numpy as np

from planted import KEY_BITS, LETTERS, NCODES, Geometry, codes, hash_of_keys, kmer_of, mix43, unmix43

CHUNK = 16                 # windows per lane per tile (one 16-byte load + halo)
LANE_BYTES = 24            # residue bytes a lane's 16 windows cover
TILE = 1024                # windows per k_pass_emit tile (64 lanes)
SEL_WG = 8192              # emission rows, at least
REL_BITS = 21              # pass entry: the window's offset in its row
BLOCK = 64                 # blk2seq granularity
SC_ROUND, SC_ROUND_HALF = 4096, 2048   # elements staged per round (stage_round 0 / 1)
EX_THREADS = 512
EX_POS_PER_THREAD = 16
EX_MAX_WG = 512
ELEM_I_BITS = 20
MAX_LEN = (1 << ELEM_I_BITS) - 1   # the longest accepted protein
UNDEF = 0xFFFF
PASSES = (4, 16, 64)

_UP = np.frombuffer(LETTERS[:20], np.uint8)
_LOW = np.frombuffer(LETTERS[20:], np.uint8)
_ALL = np.frombuffer(LETTERS, np.uint8)
VALID = np.zeros(256, bool)
VALID[_ALL] = True
INVALID_BYTES = (ord("X"), ord("*"), ord("B"), ord("7"), 0x80, ord("x"))


def ceil_div(a, b):
    return -(-a // b)


def sel_geometry(rp):
    """(sel_wg, sel_span) of a shard of rp packed bytes."""
    sel_wg = max(SEL_WG, ceil_div(max(rp, 1), (1 << REL_BITS) - 16))
    return sel_wg, CHUNK * ceil_div(ceil_div(max(rp, 1), sel_wg), CHUNK)


def front_geometry(rp, passes, pass_max, emit_group=0, stage_round=1, world=1):
    """What SignatureBuilder.debug_front() must return: pass_max is the largest pass's window count
    (routing off)."""
    step = EX_THREADS * EX_POS_PER_THREAD
    nwg = max(1, min(EX_MAX_WG, ceil_div(rp or 1, step)))
    span = ceil_div(ceil_div(rp or 1, nwg), step) * step
    pass_bits = passes.bit_length() - 1
    owner_bits = (world - 1).bit_length()
    g = dict(rp=rp, sel_wg=0, sel_span=0, emit_g=0, pf_span=0, pf_nwg=0, nwg=ceil_div(rp or 1, span), span=span,
             pass_bits=pass_bits, owner_bits=owner_bits, b1_bits=Geometry(pass_bits, owner_bits).b1_bits)
    if pass_bits:
        w = max(pass_max, 1)
        g["sel_wg"], g["sel_span"] = sel_geometry(rp)
        g["emit_g"] = max(1, min(passes, emit_group or 4))
        pf = max(1, min(4 * EX_MAX_WG if stage_round == 1 else EX_MAX_WG, ceil_div(w, SC_ROUND * 4)))
        g["pf_span"] = ceil_div(ceil_div(w, pf), SC_ROUND) * SC_ROUND
        g["pf_nwg"] = max(1, ceil_div(w, g["pf_span"]))
    return g


def keys_at(buf, pos):
    """The 8 residue bytes at each position as a little-endian u64 (the builder's key)."""
    if len(pos) == 0:
        return np.zeros(0, np.uint64)
    w = np.lib.stride_tricks.sliding_window_view(buf, 8)[np.asarray(pos, np.int64)]
    return np.ascontiguousarray(w).view("<u8").ravel().astype(np.uint64)


class Windows:
    """Every valid window of a shard, from the input arrays alone: rp, buf (the packed bytes), and
    per window pos (packed position), seq (index into the input arrays), i (offset in the sequence),
    key and hash; positions = the shard's window positions, valid or not (the `windows` counter)."""

    def __init__(self, arrays, sel=None):
        res, off, lens, funcs, _ = arrays
        kept = [s for s in range(len(lens)) if funcs[s] != UNDEF and (sel is None or sel[s])]
        self.kept = np.array(kept, np.int64)
        kl = lens[self.kept].astype(np.int64) if kept else np.zeros(0, np.int64)
        self.pstart = np.zeros(len(kept), np.int64)
        self.pstart[1:] = np.cumsum(kl[:-1] + 1)
        self.rp = int(np.sum(kl + 1))
        self.positions = int(np.sum(np.maximum(kl - 7, 0)))
        self.buf = np.zeros(self.rp + 8, np.uint8)  # separators (and the tail) are 0
        for k, s in enumerate(kept):
            a, n = int(off[s]), int(lens[s])
            self.buf[self.pstart[k]:self.pstart[k] + n] = res[a:a + n]
        run = np.zeros(self.rp + 9, np.int32)
        np.cumsum(VALID[self.buf], dtype=np.int32, out=run[1:])
        self.pos = np.nonzero(run[8:] - run[:-8] == 8)[0].astype(np.int64)
        k = np.searchsorted(self.pstart, self.pos, "right") - 1
        self.seq = self.kept[k] if len(kept) else np.zeros(0, np.int64)
        self.i = self.pos - self.pstart[k] if len(kept) else np.zeros(0, np.int64)
        self.keys = keys_at(self.buf, self.pos)
        self.hash = hash_of_keys(self.keys)
        self.n = len(self.pos)

    def pass_counts(self, passes):
        pb = passes.bit_length() - 1
        return np.bincount((self.hash >> np.uint64(KEY_BITS - pb)).astype(np.int64), minlength=passes)

    def has(self, p):
        k = np.searchsorted(self.pos, p)
        return k < self.n and self.pos[k] == p

    def count_in(self, a, e):
        return int(np.searchsorted(self.pos, e) - np.searchsorted(self.pos, a))


class Layout:
    """Phase 1 declares the sequences in input order (seq, fill_to); freeze() lays the kept ones out
    in the packed buffer; phase 2 writes islands at absolute packed positions (put, island, window,
    homopolymer); finish() scans the result and stores every window and the per-pass counts."""

    def __init__(self, seed, nf):
        self.rng = np.random.default_rng(seed)
        self.nf = nf
        self.content, self.funcs = [], []   # per input sequence: bytes or a filler length; function
        self.pos = 0                        # packed position of the next kept sequence
        self.used = set()                   # every 8-mer (key) an island has taken
        self.buf = None
        self.claims = {}                    # what the layout declares, checked by the CPU test
        self.homo = []                      # (kmer, packed position, windows, input sequence)

    # -- phase 1: sequences ---------------------------------------------------------------------
    def func(self):
        return int((7 * len(self.content) + 3) % self.nf)

    def seq(self, content, func=None):
        """A kept sequence: bytes, or an int for that many X.  Returns (input index, packed start)."""
        n = content if isinstance(content, int) else len(content)
        assert self.buf is None and n <= MAX_LEN
        self.content.append(content)
        self.funcs.append(self.func() if func is None else func)
        start = self.pos
        self.pos += n + 1
        return len(self.content) - 1, start

    def undefined(self, content):
        """A sequence with the undefined function: dropped at add_batch, no packed bytes."""
        assert self.buf is None
        self.content.append(content)
        self.funcs.append(UNDEF)

    def fill_to(self, pos):
        """A filler protein that ends so that the next kept sequence starts at packed `pos`."""
        assert pos - self.pos >= 1
        return self.seq(pos - self.pos - 1)

    def freeze(self):
        self.rp = self.pos
        self.sel_wg, self.span = sel_geometry(self.rp)
        self.buf = np.full(self.rp, ord("X"), np.uint8)
        self.kept = [s for s, f in enumerate(self.funcs) if f != UNDEF]
        self.pstart, p = [], 0
        for s in self.kept:
            c = self.content[s]
            n = c if isinstance(c, int) else len(c)
            if not isinstance(c, int):
                self.buf[p:p + n] = np.frombuffer(c, np.uint8)
            self.buf[p + n] = 0
            self.pstart.append(p)
            p += n + 1
        assert p == self.rp
        self.pstart = np.array(self.pstart, np.int64)
        self.written = np.zeros(self.rp, bool)
        for k, s in enumerate(self.kept):
            if not isinstance(self.content[s], int):
                self.written[self.pstart[k]:self.pstart[k] + len(self.content[s]) + 1] = True
        self.written[self.buf == 0] = True

    # -- residues -------------------------------------------------------------------------------
    def fresh(self, n, letters=_ALL):
        """n random valid residues none of whose 8-mers any island has used."""
        for _ in range(100):
            b = letters[self.rng.integers(0, len(letters), n)]
            if n >= 8:
                ks = keys_at(b, np.arange(n - 7)).tolist()
                if len(set(ks)) < len(ks) or not self.used.isdisjoint(ks):
                    continue
                self.used.update(ks)
            return b.tobytes()
        raise AssertionError("no fresh residues")

    # -- phase 2: islands -----------------------------------------------------------------------
    def row(self, r, offset=0):
        return r * self.span + offset

    def seq_at(self, p):
        """(input index, offset) of the kept sequence that holds packed position p."""
        k = int(np.searchsorted(self.pstart, p, "right")) - 1
        return self.kept[k], p - int(self.pstart[k])

    def put(self, p, data, cross=False):
        """Writes data at packed position p, over untouched filler only.  An island that would cross
        a separator is refused unless cross: then the separator stays and that byte of data is lost.
        The bytes next to the island must not be residues of another island."""
        data = np.frombuffer(data, np.uint8)
        n = len(data)
        assert self.buf is not None and 0 <= p and p + n <= self.rp, (p, n)
        seps = self.buf[p:p + n] == 0
        assert cross or not seps.any(), ("island crosses a separator", p, n)
        assert not self.written[p:p + n][~seps].any(), ("island overlaps another", p, n)
        for q in (p - 1, p + n):
            assert q < 0 or q >= self.rp or not VALID[self.buf[q]], ("island touches another", p, n)
        self.buf[p:p + n][~seps] = data[~seps]
        self.written[p:p + n] = True

    def island(self, p, n, invalid=None, letters=_ALL, cross=False):
        """n fresh residues at p; invalid = (offset, byte) plants one invalid residue."""
        b = bytearray(self.fresh(n, letters))
        if invalid is not None:
            b[invalid[0]] = invalid[1]
        self.put(p, bytes(b), cross)
        return bytes(b)

    def window(self, p):
        """One isolated window at p."""
        return self.island(p, 8)

    def homopolymer(self, p, letter, n):
        """n residues of one letter at p: n - 7 windows of one key in one sequence."""
        kmer = bytes([letter]) * 8
        key = int.from_bytes(kmer, "little")
        assert key not in self.used
        self.used.add(key)
        self.put(p, bytes([letter]) * n)
        self.homo.append((kmer, p, n - 7, self.seq_at(p)[0]))

    # -- the input ------------------------------------------------------------------------------
    def finish(self):
        seqs = []
        kept_at = {s: k for k, s in enumerate(self.kept)}
        for s, c in enumerate(self.content):
            if s in kept_at:
                n = c if isinstance(c, int) else len(c)
                a = int(self.pstart[kept_at[s]])
                seqs.append(self.buf[a:a + n].tobytes())
            else:
                seqs.append(c)
        lens = np.array([len(s) for s in seqs], np.uint32)
        off = np.zeros(len(seqs), np.uint64)
        off[1:] = np.cumsum(lens[:-1].astype(np.uint64))
        self.arrays = (np.frombuffer(b"".join(seqs), np.uint8), off, lens, np.array(self.funcs, np.uint16),
                       np.arange(len(seqs), dtype=np.uint32))
        self.windows = Windows(self.arrays)
        assert self.windows.rp == self.rp
        self.pass_counts = {P: self.windows.pass_counts(P) for P in PASSES}
        # every window is a singleton, the declared homopolymers aside
        homo = np.array([int.from_bytes(h[0], "little") for h in self.homo], np.uint64)
        single = self.windows.keys[~np.isin(self.windows.keys, homo)]
        assert len(np.unique(single)) == len(single)
        self.distinct = len(single) + len(self.homo)
        return self


def homopolymer_hash(letter):
    code = 0
    for _ in range(8):
        code = code * 40 + LETTERS.index(letter)
    return int(mix43(np.array([code], np.uint64))[0])


def upper_half_letter():
    """The first letter whose homopolymer's hash has its top bit set: the upper half of the passes
    at every pass count."""
    for c in LETTERS:
        if homopolymer_hash(c) >> (KEY_BITS - 1):
            return c
    raise AssertionError


# ---------------------------------------------------------------------------------------------
# Layout G: rows of more than two tiles
# ---------------------------------------------------------------------------------------------
G_SPAN = 2 * TILE + CHUNK        # the smallest row with a third, short tile
G_RP = SEL_WG * G_SPAN - G_SPAN - 1001   # the last row lies past rp, the one before is cut short; rp mod 16 = 7
G_NF = 1000
EDGE_DENSE = 30
G_SWEEP_ROW, G_POLYA_ROW, G_UPPER_ROW, G_DENSE_ROW = 10, 30, 40, 50
G_UPPER_LEN = 2 * G_SPAN + 7     # two full rows of one key
G_EDGE_ROWS = (0, 4000, SEL_WG - 14)
G_BIG_I = (0, 65527, 65528, 65536, MAX_LEN - 8)


def small_run(L, n, empties):
    """n sequences of 0..7 residues, sequences with the undefined function among them, then --
    from the next 64-byte boundary -- `empties` sequences of 0, 0, 1, ... residues (dozens of
    sequences within one block), then directly an 8-residue sequence.
    Returns (input index, packed start) of that sequence."""
    lens = [int(x) for x in L.rng.integers(0, 8, n)]
    lens[0], lens[1] = 0, 7
    for k, n_res in enumerate(lens):
        L.seq(L.fresh(n_res))
        if k % 9 == 4:
            L.undefined(L.fresh(int(L.rng.integers(8, 40))))  # its windows must not appear
    if empties:
        while L.pos % BLOCK:
            L.seq(L.fresh(min(-L.pos % BLOCK, 8) - 1))
        for k in range(empties):
            L.seq(L.fresh(1 if k % 3 == 2 else 0))
    return L.seq(L.fresh(8))


@functools.lru_cache(maxsize=None)
def layout_g():
    L = Layout(20241, G_NF)
    c = L.claims
    # --- sequences ---
    b1 = BLOCK * 15624
    L.fill_to(b1)                                   # protein 0 starts on row 0
    c["run1"] = (b1, small_run(L, 100, 30))         # starts on a 64-byte boundary
    L.undefined(b"X" * 500)
    b2 = BLOCK * 31250 - 3
    L.fill_to(b2)
    c["run2"] = (b2, small_run(L, 100, 0))          # starts just before a 64-byte boundary
    c["eights"] = [L.seq(L.fresh(8)) for _ in range(64)]   # 64 sequences of exactly 8 residues
    L.undefined(L.fresh(200))
    c["big"] = L.seq(MAX_LEN)                       # the longest accepted protein
    k = 0
    while G_RP - L.pos > 1_600_000:
        L.seq(999_999 - 37 * k)
        if k % 3 == 0:
            L.undefined(L.fresh(64 + k))
        k += 1
    c["cross"] = L.pos + (G_RP - L.pos) // 2        # an island laid across this boundary
    L.fill_to(c["cross"] + 1)
    L.fill_to(G_RP)
    L.freeze()
    assert L.span == G_SPAN and L.sel_wg == SEL_WG and L.rp == G_RP
    span = L.span
    # --- row and tile edges: rows r, r + 1, r + 2 of every group ---
    c["must"], c["isolated"], c["dense"] = {}, [], []
    for r in G_EDGE_ROWS:
        ranges = []   # window offsets [at - 30, at + 30); the last two merge when the third tile is short
        for at in (TILE, 2 * TILE, span):
            if ranges and at - EDGE_DENSE <= ranges[-1][1] + 8:
                ranges[-1][1] = at + EDGE_DENSE
            else:
                ranges.append([at - EDGE_DENSE, at + EDGE_DENSE])
        for lo, hi in ranges:
            L.island(L.row(r, lo), hi - lo + 7)
            c["dense"].append((L.row(r, lo), hi - lo))
        for rr, at in ((r, 0), (r + 1, TILE - 1), (r + 1, span - 1), (r + 2, TILE)):
            L.window(L.row(rr, at))     # the window at span - 1 has its residues in the next row
            c["isolated"].append(L.row(rr, at))
            c["must"][f"row {rr} offset {at}"] = L.row(rr, at)
        for at in (TILE - 1, TILE, span - 1):
            c["must"][f"row {r} offset {at}"] = L.row(r, at)
    assert L.seq_at(0) == (0, 0)       # the first protein starts on a window
    # --- alignment sweep: start a mod 16, one invalid byte at j ---
    c["sweep"] = []
    p = L.row(G_SWEEP_ROW)
    n = 0
    for a in range(CHUNK):
        for j in list(range(LANE_BYTES)) + [None, "lower"]:
            q = p + (a - p) % CHUNK
            if j is None:
                b = L.island(q, LANE_BYTES)
            elif j == "lower":
                b = L.island(q, LANE_BYTES, letters=_LOW)
            else:
                b = L.island(q, LANE_BYTES, invalid=(j, INVALID_BYTES[n % len(INVALID_BYTES)]))
                n += 1
            c["sweep"].append((q, a, j, b))
            p = q + LANE_BYTES + 17
    c["sweep_end_row"] = (p + span - 1) // span
    assert c["sweep_end_row"] + 5 <= G_POLYA_ROW
    # --- full tiles ---
    L.homopolymer(L.row(G_POLYA_ROW), ord("A"), TILE + 2 * CHUNK + 7)   # hash 0: pass 0, bucket 0, rem 0
    c["upper"] = upper_half_letter()
    L.homopolymer(L.row(G_UPPER_ROW), c["upper"], G_UPPER_LEN)
    c["full_tiles"] = [(G_POLYA_ROW, 0), (G_UPPER_ROW, 0), (G_UPPER_ROW, 1), (G_UPPER_ROW + 1, 0),
                       (G_UPPER_ROW + 1, 1)]
    c["dense_stretch"] = (L.row(G_DENSE_ROW, 5), span + TILE)
    L.island(c["dense_stretch"][0], span + TILE)
    # --- the longest protein: every bit of the 20-bit i, and (len - i) mod 2^16 around a wrap ---
    big, start = c["big"]
    L.window(start)
    L.island(start + 65527, 65536 - 65527 + 8)      # windows 65527 .. 65536
    L.window(start + MAX_LEN - 8)
    # --- an island across a separator: windows on both sides, none spans it ---
    L.island(c["cross"] - 15, 31, cross=True)
    # --- empty rows (at least 5 in a row between occupied ones, 3 * span of X after the last) ---
    c["empty_rows"] = [(3, G_SWEEP_ROW), (c["sweep_end_row"], G_POLYA_ROW), (G_POLYA_ROW + 2, G_UPPER_ROW),
                       (G_UPPER_ROW + 3, G_DENSE_ROW), (G_DENSE_ROW + 3, G_DENSE_ROW + 400),
                       (G_EDGE_ROWS[1] - 6, G_EDGE_ROWS[1]), (G_EDGE_ROWS[1] + 3, G_EDGE_ROWS[1] + 9),
                       (G_EDGE_ROWS[2] - 6, G_EDGE_ROWS[2]), (G_EDGE_ROWS[2] + 3, SEL_WG)]
    c["last_row"] = G_EDGE_ROWS[2] + 2
    return L.finish()


# ---------------------------------------------------------------------------------------------
# Layout E: empty passes.  Small: rows are one chunk of 16 windows.
# ---------------------------------------------------------------------------------------------
E_NF = 50
E_LEN = 340


def largest_valid_hash():
    h = (1 << KEY_BITS) - 1
    while int(unmix43(np.array([h], np.uint64))[0]) >= NCODES:
        h -= 1
    return h


def _layout_e(seed, passes, natural):
    """Five proteins of X with isolated 8-mers 9 apart whose passes cycle through `natural`; the
    last of `natural` only in the last row that holds a window, twice."""
    L = Layout(seed, E_NF)
    starts = [L.seq(E_LEN)[1] for _ in range(5)]
    L.freeze()
    assert L.span == CHUNK
    pb = passes.bit_length() - 1
    body, last = natural[:-1] or natural, natural[-1]
    pool = {p: [int(x) for x in codes(pb, p, 200, L.rng)] for p in set(natural)}
    extreme = {0: 0, passes - 1: int(unmix43(np.array([largest_valid_hash()], np.uint64))[0])}
    taken = set()

    def kmer(p):
        code = extreme.pop(p) if p in extreme and p in natural else pool[p].pop()
        assert code not in taken
        taken.add(code)
        key = int.from_bytes(kmer_of(code), "little")
        assert key not in L.used
        L.used.add(key)
        return kmer_of(code)

    n = 0
    for s, ps in enumerate(starts):
        for k in range(20 if s == 4 else 30):
            L.put(ps + (3 * CHUNK if s == 0 else 2) + 9 * k, kmer(body[n % len(body)]))
            n += 1
    row = (starts[4] + 2 + 9 * 20 + 8) // CHUNK + 2
    L.put(L.row(row), kmer(last))
    L.put(L.row(row, 9), kmer(last))
    L.claims.update(passes=passes, natural=sorted(set(natural)), last_pass=last, last_row=row,
                    leading=3 * CHUNK)
    assert L.rp - L.row(row + 1) >= 3 * CHUNK
    return L.finish()


@functools.lru_cache(maxsize=None)
def layout_e64():
    """64 passes, windows in passes 0, 37 and 63 only; poly-A (hash 0) and the largest hash with a
    valid code among them; pass 63 only in the last occupied row."""
    return _layout_e(311, 64, (0, 37, 63))


@functools.lru_cache(maxsize=None)
def layout_e4():
    """4 passes, windows in pass 2 only."""
    return _layout_e(312, 4, (2,))


@functools.lru_cache(maxsize=None)
def layout_one():
    """One single window in total."""
    L = Layout(313, E_NF)
    L.seq(100)
    _, s = L.seq(100)
    L.seq(100)
    L.freeze()
    L.window(s + 41)
    return L.finish()


@functools.lru_cache(maxsize=None)
def layout_none():
    """No valid window at all: filler, sequences shorter than a window, 8 residues with an invalid
    one, and a valid window in a sequence with the undefined function."""
    L = Layout(314, E_NF)
    L.seq(100)
    L.seq(L.fresh(7))
    L.seq(b"")
    L.undefined(L.fresh(30))
    L.seq(L.fresh(4) + b"X" + L.fresh(7))
    L.seq(L.fresh(7) + b"*" + L.fresh(7) + b"1" + L.fresh(7))
    L.seq(60)
    L.freeze()
    return L.finish()


TAIL_MODS = (0, 1, 7, 8, 9, 15)


@functools.lru_cache(maxsize=None)
def layout_tail(mod):
    """Fewer than 64 residues; the last sequence ends in a valid 8-mer on the last residue and
    rp mod 16 == mod."""
    L = Layout(400 + mod, E_NF)
    L.seq(L.fresh(10))
    L.seq(b"X" * ((mod - 20) % CHUNK) + L.fresh(8))
    L.freeze()
    assert L.rp % CHUNK == mod and L.rp < BLOCK
    return L.finish()
