"""Planted hits for the HitSet call path -- a plain helper module of the tests.

The call path (k_lookup, k_calls_scan, k_seg_process in skm_annotate.hip) consumes one word per
query window: function_index << 16 | mean of the window's DB record, or NO_HIT.  Over an exact-key
DB (KeptKmerDb, the only kind that can miss) that array can be written by hand: a Scenario is one
sequence, (length, [(window position, function, mean), ...]); Batch draws `length` random residues
per scenario and puts into the DB exactly the 8-mers found at the planted positions, each with
its planted record.  Batch.distinct() states that the 8-mers of all windows of all sequences are
pairwise distinct (about 4e4 windows against 20^8 keys: a collision is a seed to change), so a
planted window hits its own record and every other window misses.

Functions are symbolic until a scenario has its place in the batch: "A" is the sequence's own
function (FUNC_BASE + its index, so a hit read from a neighbour is a stranger), ("S", k) a
stranger shared by all sequences, "H" the hypothetical protein.

catalogue(min_hits, max_gap) is the batch of one option set: the state-machine scenarios are laid
out for that min_hits / max_gap, the rest is the same for every option set.  Each scenario states
what it claims (`claims`: the n, span and R of its segment) and, where it can be written by hand,
what the reference must answer (`expect`); tests/test_planted_hits_cpu.py proves both.

matrix_cases() plants one shared 8-mer per case (record: function, mean, var) into sequences of
chosen lengths, for the length filter of the matrix distance (k_md_hits in skm_matrix.hip).
"""
from __future__ import annotations

import functools

import numpy as np

import oracle_ref

AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
HYPO = 7              # index of "hypothetical protein" in function_index()
FUNC_BASE = 1000      # a sequence's own function: FUNC_BASE + its index in the batch
STRANGER_BASE = 60000
N_FUNCTIONS = 60100
NO_HIT = 0xFFFFFFFF
SEG_CAP = 1024        # k_seg_process: hits of one segment held in LDS; histogram selects up to this R
SC_TILE = 2048        # the u32 -> u64 scans' tile
MIN_SEQS = 2 * SC_TILE + 1
STRADDLES = (64, 256, SC_TILE, 2 * SC_TILE)  # k_calls_scan's block, the 256-thread kernels, the scan tiles
TILE_NWIN = (1, 2, 3, 4, 12, 13, 15, 16, 17, 19, 20, 31, 32, 33, 48, 49)
SLOT_M = (2, 3, 4, 5, 6)
SLOT_NWIN = 600
LDS_N = (2, 3, 4, 5, 7, 8, 31, 32, 33, 35, 36, 63, 64, 65, 255, 256, 257, 260, 1021, 1022, 1023, 1024)
RANGE_R = (1, 2, 64, 65, 1023, 1024, 1025, 1026, 4097, 65536)
RANGE_N = (6, 7, 130, 131)

# (min_hits, max_gap, ignore_hypo, mean_mode, mad_mode)
OPTION_SETS = [(2, 200, 0, 0, 0), (3, 7, 0, 0, 0), (5, 200, 0, 0, 0), (5, 1, 0, 0, 0), (5, 0, 0, 0, 0),
               (6, 200, 0, 0, 0), (4, 3, 0, 0, 0), (5, 200, 1, 0, 0), (5, 200, 0, 1, 0), (5, 200, 0, 0, 1),
               (5, 200, 0, 1, 1), (2, 200, 0, 0, 1)]


def opt_id(o):
    return "m%d-g%d-h%d-mean%d-mad%d" % o


def function_index():
    fi = ["f%d" % i for i in range(N_FUNCTIONS)]
    fi[HYPO] = "hypothetical protein"
    return fi


class Scenario:
    """One sequence.  hits: [(window position, function symbol, mean)] in window order; kind: the
    catalogue part it belongs to; claims: what its segment is built to be (n, span, R); expect:
    None, or f(min_hits, max_gap, ignore_hypo) -> the calls the reference must make, as a list of
    (start, end, count, function symbol) or, where only that is stated, their number."""

    def __init__(self, name, length, hits, kind, claims=None, expect=None):
        self.name, self.length, self.hits, self.kind = name, int(length), list(hits), kind
        self.claims = claims or {}
        self.expect = expect
        nwin = max(0, self.length - 7)
        pos = [h[0] for h in self.hits]
        assert pos == sorted(set(pos)) and (not pos or (pos[0] >= 0 and pos[-1] < nwin)), name
        assert all(0 <= h[2] <= 0xFFFF for h in self.hits), name

    @property
    def nwin(self):
        return max(0, self.length - 7)

    @property
    def dense(self):  # every window planted: the scenario also runs over a BDZ DB
        return len(self.hits) == self.nwin


def resolve(sym, index):
    if sym == "A":
        return FUNC_BASE + index
    if sym == "H":
        return HYPO
    assert sym[0] == "S"
    return STRANGER_BASE + sym[1]


# ---- means ------------------------------------------------------------------------------------

def sym_means(n, centre, half, rng):
    """n means symmetric around `centre` (pairs centre +/- d, d in [1, half]; an odd n adds the
    centre itself) in random order: their mean is the centre, so a sequence of that length passes
    the length filter whatever the MAD."""
    d = rng.integers(1, half + 1, n // 2)
    v = np.concatenate([centre + d, centre - d, np.full(n & 1, centre)])
    rng.shuffle(v)
    assert v.min() >= 0 and v.max() <= 0xFFFF
    return [int(x) for x in v]


def range_means(n, length, R, rng):
    """n >= 2 means with max - min + 1 == R exactly, both ends present.  Where the range fits
    around the sequence length it is centred there and filled symmetrically; a wider one starts at
    0 and is filled mostly at its two ends, so that the MAD is about R / 2 and every length inside
    the range passes the filter."""
    if R == 1:
        return [length] * n
    vmin = length - (R - 1) // 2
    wide = vmin < 0
    if wide:
        vmin = 0
    v = [0, R - 1]
    while len(v) + 2 <= n:
        x = 0 if (wide and rng.random() < 0.8) else int(rng.integers(0, R))
        v += [x, R - 1 - x]
    if len(v) < n:
        v.append((R - 1) // 2)
    v = np.array(v) + vmin
    rng.shuffle(v)
    assert v.max() <= 0xFFFF and v.max() - v.min() + 1 == R
    return [int(x) for x in v]


# ---- the state machine (process_aa_seq, call_functions.tcc:259-338) ----------------------------

def state_machine(m, g):
    """The named events of process_aa_seq for min_hits m and max_gap g.  Hits of a run are one
    window apart and carry the sequence length as their mean (MAD 0 -> 30: every call passes the
    length filter).  With max_gap 0 two hits never chain, so nothing is ever called; the layouts
    are then those of max_gap 1."""
    lay = max(g, 1)
    out = []
    S = lambda k: ("S", k)

    def add(name, runs, tail, expect):
        """runs: [(first position, [function symbols])]; the sequence ends `tail` windows after the
        last hit."""
        hits = [(p + k, f) for p, fs in runs for k, f in enumerate(fs)]
        nwin = hits[-1][0] + 1 + tail
        length = nwin + 7

        def ex(mm, gg, ignore, _e=expect):
            if gg == 0:
                return []
            return [c for c in _e(bool(ignore), gg) if c is not None]
        out.append(Scenario("sm_" + name, length, [(p, f, length) for p, f in hits], "sm", expect=ex))

    def call(first, last_cur, count, f="A"):
        return (first, last_cur + 7, count, f) if count >= m else None

    # two runs of m whose last and first hits are exactly g apart / g + 1 apart
    p2 = 3 + m - 1 + lay
    add("gap_eq", [(3, ["A"] * m), (p2, ["A"] * m)], 5, lambda ig, gg: [call(3, p2 + m - 1, 2 * m)])
    add("gap_gt", [(3, ["A"] * m), (p2 + 1, ["A"] * m)], 5,
        lambda ig, gg: [call(3, 3 + m - 1, m), call(p2 + 1, p2 + m, m)])
    # the first run one hit short: a gap of g joins them, a gap of g + 1 clears it silently
    q2 = 3 + m - 2 + lay
    add("short_eq", [(3, ["A"] * (m - 1)), (q2, ["A"] * m)], 5, lambda ig, gg: [call(3, q2 + m - 1, 2 * m - 1)])
    add("short_gt", [(3, ["A"] * (m - 1)), (q2 + 1, ["A"] * m)], 5, lambda ig, gg: [call(q2 + 1, q2 + m, m)])
    # a lone stranger as the last hit of the segment: end = last A + 7
    add("lone_stranger", [(2, ["A"] * m + [S(1)])], 4, lambda ig, gg: [call(2, 2 + m - 1, m)])
    # A x m, B, B: the call for A, then the kept pair (a call of its own only when m == 2)
    add("pair_after", [(2, ["A"] * m + [S(1)] * 2)], 4,
        lambda ig, gg: [call(2, 2 + m - 1, m), call(2 + m, 2 + m + 1, 2, S(1))])
    # A x m, B x m: the second call starts at the first B
    add("pair_grows", [(2, ["A"] * m + [S(1)] * m)], 4,
        lambda ig, gg: [call(2, 2 + m - 1, m), call(2 + m, 2 + 2 * m - 1, m, S(1))])
    # A, A, B x m: no call for A when m > 2, but the pair (B, B) is still kept
    add("short_then_pair", [(2, ["A"] * 2 + [S(1)] * m)], 4,
        lambda ig, gg: [call(2, 3, 2), call(4, 4 + m - 1, m, S(1))])
    # count >= m with fewer than m hits of the current function (A S1 A S2 ... A S(m-1)), ended by
    # the end of the sequence and by a gap
    mixed = [x for k in range(1, m) for x in ("A", S(k))]
    add("mixed_end", [(2, mixed)], 6, lambda ig, gg: [])
    r2 = 2 + len(mixed) - 1 + lay + 1
    add("mixed_gap", [(2, mixed), (r2, ["A"] * m)], 6, lambda ig, gg: [call(r2, r2 + m - 1, m)])
    # hypothetical hits: invisible when ignored
    h1 = 2 + m - 1 + lay
    a2 = h1 + lay
    add("hypo_bridge", [(2, ["A"] * m), (h1, ["H"]), (a2, ["A"] * m)], 5,
        lambda ig, gg: [call(2, 2 + m - 1, m), call(a2, a2 + m - 1, m)] if ig else [call(2, a2 + m - 1, 2 * m)])
    add("hypo_interleaved", [(2, [x for _ in range(m) for x in ("A", "H")])], 5,
        lambda ig, gg: [] if ig and gg < 2 else [call(2, 2 + 2 * m - 2, m)])
    add("hypo_run", [(2, ["H"] * m)], 5, lambda ig, gg: [] if ig else [call(2, 2 + m - 1, m, "H")])
    # the first and the last window; a run that is the entire sequence (end == len - 1)
    e2 = m - 1 + lay + 1
    add("both_ends", [(0, ["A"] * m), (e2, ["A"] * m)], 0, lambda ig, gg: [call(0, m - 1, m), call(e2, e2 + m - 1, m)])
    add("whole_sequence", [(0, ["A"] * m)], 0, lambda ig, gg: [call(0, m - 1, m)])
    return out


# ---- load tiling, scans, segment slots -----------------------------------------------------------

def dense(name, nwin, kind, expect=None):
    """Every window a hit of the sequence's own function, mean = the sequence length."""
    length = nwin + 7
    return Scenario(name, length, [(i, "A", length) for i in range(nwin)], kind, claims=dict(n=nwin),
                    expect=expect or (lambda m, g, ig, _n=nwin: [(0, _n + 6, _n, "A")] if _n >= m and g else []))


def filler(k):
    """The tiny sequences between the others: 0, 1, 7 and 8 residues (the last has one window)."""
    length = (0, 1, 7, 8)[k % 4]
    if length == 8:
        return Scenario("fill8", 8, [(0, "A", 8)], "fill", expect=lambda m, g, ig: [])
    return Scenario("fill%d" % length, length, [], "fill", expect=lambda m, g, ig: [])


def load_tiling(pstart0):
    """Dense sequences of every nwin in TILE_NWIN at every pstart & 3, pstart being the running
    sum of len + 1 from pstart0 on: before each, one filler of the cycling kinds and then empty
    sequences (one byte each) until the start has the wanted alignment."""
    out, p, k = [], pstart0, 0
    for nwin in TILE_NWIN:
        for mis in range(4):
            f = filler(k)
            k += 1
            out.append(f)
            p += f.length + 1
            while p & 3 != mis:
                out.append(filler(0))
                p += 1
            out.append(dense("tile_n%d_mis%d" % (nwin, mis), nwin, "tile"))
            p += nwin + 8
    return out


def slots(mm):
    """SLOT_NWIN windows, every one a hit, in runs of exactly mm of two alternating functions: with
    min_hits == mm every run is a call, the densest a sequence can be (SLOT_NWIN // mm calls)."""
    length = SLOT_NWIN + 7
    hits = [(i, "A" if (i // mm) % 2 == 0 else ("S", 2), length) for i in range(SLOT_NWIN)]
    return Scenario("slots_m%d" % mm, length, hits, "slots", claims=dict(runs=mm))


# ---- k_seg_process -------------------------------------------------------------------------------

def seg_scenarios(rng):
    out = []

    def one(name, nwin, pos, means, claims, ncalls=None, extra=(), length=None):
        """A sequence whose hits of its own function are pos / means, plus `extra` stranger hits;
        ncalls: the calls at max_gap 200 as a function of min_hits (default: one if n >= min_hits)."""
        length = length or nwin + 7
        hits = sorted([(p, "A", v) for p, v in zip(pos, means)] + list(extra))
        n = len(pos)
        nc = ncalls or (lambda m, _n=n: int(_n >= m))
        out.append(Scenario("seg_" + name, length, hits, "seg", claims=claims,
                            expect=lambda m, g, ig, _nc=nc: _nc(m) if g == 200 else None))

    # the LDS path: n around the four-lane mean's 8- and 64-step blocks, n % 4 tails, up to SEG_CAP
    for n in LDS_N:
        one("n%d" % n, n, range(n), sym_means(n, n + 7, min(20, n + 7), rng), dict(n=n, span=n))
    # the sequential path; three such segments back to back through kept pairs share the pool
    one("n1025", 1025, range(1025), sym_means(1025, 1032, 20, rng), dict(n=1025, span=1025))
    ns = (1025, 1026, 2049)
    nwin = sum(ns)
    hits, p = [], 0
    for f, n in zip(("A", ("S", 3), ("S", 4)), ns):
        hits += [(p + i, f, v) for i, v in enumerate(sym_means(n, nwin + 7, 20, rng))]
        p += n
    out.append(Scenario("seg_seq3", nwin + 7, hits, "seg", claims=dict(ns=ns),
                        expect=lambda m, g, ig: 3 if g == 200 else None))
    # a window range wider than SEG_CAP with n < SEG_CAP (the 64-at-a-time walk): every other window
    for span in (1024, 1025, 1088, 1089):
        pos = sorted(set(range(0, span, 2)) | {span - 1})
        one("span%d" % span, span + 3, pos, sym_means(len(pos), span + 10, 20, rng), dict(n=len(pos), span=span))
    # one hit every third window: max_gap 3 chains them (n = 1034, sequential), max_gap 2 does not
    for nwin, n in ((3100, 1034), (3070, 1024)):
        pos = list(range(0, nwin, 3))
        assert len(pos) == n
        one("third_n%d" % n, nwin, pos, sym_means(n, nwin + 7, 20, rng), dict(n=n, span=pos[-1] + 1))
    # strangers: single hits of other functions at segment offsets 63, 64 and 1023 and as the last
    # two hits of the span (end = last own hit + 7); LDS path (with a hole) and sequential path
    for name, nwin, hole in (("strangers_lds", 1030, range(500, 510)), ("strangers_seq", 1100, ())):
        sp = [63, 64, 1023, nwin - 2, nwin - 1]
        extra = [(p, ("S", 10 + k), nwin + 7) for k, p in enumerate(sp)]
        pos = [p for p in range(nwin) if p not in sp and p not in hole]
        one(name, nwin, pos, sym_means(len(pos), nwin + 7, 20, rng),
            dict(n=len(pos), span=nwin, end=nwin - 3 + 7), extra=extra)
    # the range of the means: histogram selects up to R == SEG_CAP, radix selects above
    for R in RANGE_R:
        for n in RANGE_N:
            one("R%d_n%d" % (R, n), n, range(n), range_means(n, n + 7, R, rng), dict(n=n, span=n, R=R))
    for n in (10, 11, 130):
        L = n + 7
        one("two_valued_n%d" % n, n, range(n), [L - 5 if i % 2 == 0 else L + 5 for i in range(n)],
            dict(n=n, R=11, mad=30.0 if n & 1 else 5.0))
        one("all_but_one_n%d" % n, n, range(n), [L + 100 if i == n // 2 else L for i in range(n)],
            dict(n=n, R=101, mad=30.0))
    # an even n whose middle pair differs by an odd number (C2 odd, fractional median and MAD) and by
    # an even number
    for name, up, mad in (("c2_odd", 1, 3.5), ("c2_even", 2, 4.0)):
        n, L = 10, 17
        v = [L - 2 - i for i in range(5)] + [L + up + i for i in range(5)]
        rng.shuffle(v)
        one(name, n, range(n), v, dict(n=n, mad=mad, c2=(L - 2) + (L + up)))
    # the inclusive cut-offs: constant means (MAD 0 -> 30), mean -/+ 60 kept, -/+ 61 dropped
    for d, kept in ((60, 1), (-60, 1), (61, 0), (-61, 0)):
        n, L = 8, 100
        one("cut%+d" % d, L - 7, range(n), [L + d] * n, dict(n=n, R=1, mad=30.0),
            ncalls=lambda m, _k=kept: _k * int(8 >= m), length=L)
    # a fractional MAD with the length exactly on mean - 2 mad: the means (c-3, c-1, c+2, c+2) twice
    # have mean c exactly (each lane of the four-lane mean sees one value), median c + 0.5, MAD 1.5
    for name, c, kept in (("cut_frac_on", 103, 1), ("cut_frac_off", 104, 0)):
        n, L = 8, 100
        one(name, L - 7, range(n), [c - 3, c - 1, c + 2, c + 2] * 2, dict(n=n, mad=1.5, c2=2 * c + 1),
            ncalls=lambda m, _k=kept: _k * int(8 >= m), length=L)
    return out


def catalogue(min_hits, max_gap, seed=1):
    """The batch of one option set, in order: state machine, segment statistics, the five slot
    sequences each between dense call makers, load tiling, fillers up to MIN_SEQS, the slot
    sequences again with that of min_hits as the very last; dense call makers then take the
    indices on both sides of every boundary in STRADDLES."""
    rng = np.random.default_rng(seed)
    head = state_machine(min_hits, max_gap) + seg_scenarios(rng)
    for mm in SLOT_M:
        head += [dense("mid_before_m%d" % mm, 20, "tile"), slots(mm)]
    head.append(dense("mid_after", 20, "tile"))
    head += load_tiling(sum(s.length + 1 for s in head))
    tail = [slots(mm) for mm in SLOT_M if mm != min_hits] + [slots(min_hits)] if min_hits in SLOT_M else \
        [slots(mm) for mm in SLOT_M]
    k = 0
    while len(head) + len(tail) + 2 * len(STRADDLES) < MIN_SEQS + 8:
        head.append(filler(k))
        k += 1
    seqs = head + tail
    for b in STRADDLES:  # 28 bytes each with the separator: no later pstart & 3 changes
        seqs.insert(b - 1, dense("straddle_%d_lo" % b, 20, "straddle"))
        seqs.insert(b, dense("straddle_%d_hi" % b, 20, "straddle"))
    return seqs


# ---- materialise ---------------------------------------------------------------------------------

def window_keys(flat):
    """The little-endian u64 of the 8 bytes at every position of a byte array (len - 7 of them)."""
    if len(flat) < 8:
        return np.zeros(0, np.uint64)
    return np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(flat, 8)).view("<u8").ravel()


class Batch:
    """A materialised list of scenarios.
    residues / seq_off / seq_len     the sequences back to back (seq_off[s] = sum of len)
    p_residues / p_seq_off           the packed layout, seq_off[s] = sum of len + 1; the byte after
                                     sequence s is a residue that completes, with its last 7, the
                                     trap key of s (in the DB with s's own function): a separator
                                     taken for a residue makes a hit
    keys / data                      the DB, keys ascending: planted windows and trap keys
    hit_off / hit_pos / hit_fm       the planted hits per sequence as skm_query_window_hits gives them
    pstart                           the device's packed start of each sequence"""

    def __init__(self, scens, seed=5):
        self.scens = scens
        rng = np.random.default_rng(seed)
        n = len(scens)
        self.seq_len = np.array([s.length for s in scens], np.uint32)
        lens = self.seq_len.astype(np.int64)
        total = int(lens.sum())
        self.seq_off = np.zeros(n, np.uint64)
        self.seq_off[1:] = np.cumsum(lens[:-1])
        self.pstart = np.zeros(n, np.uint64)
        self.pstart[1:] = np.cumsum(lens[:-1] + 1)
        self.p_seq_off = self.pstart.copy()
        self.residues = AA[rng.integers(0, 20, total)]
        gap = AA[rng.integers(0, 20, n)]
        self.p_residues = np.zeros(total + n, np.uint8)
        off = self.seq_off.astype(np.int64)
        poff = self.pstart.astype(np.int64)
        src = np.arange(total) + np.repeat(poff - off, lens)
        self.p_residues[src] = self.residues
        self.p_residues[poff + lens] = gap
        # every window of every sequence
        wk = window_keys(self.residues)
        valid = np.zeros(len(wk), bool)
        for s in range(n):
            if lens[s] >= 8:
                valid[off[s]:off[s] + lens[s] - 7] = True
        self.all_window_keys = wk[valid]
        self.n_windows = int(valid.sum())
        # planted records
        pk, pf, pm, hoff, hpos = [], [], [], [0], []
        for s, sc in enumerate(scens):
            for p, f, v in sc.hits:
                pk.append(wk[off[s] + p])
                pf.append(resolve(f, s))
                pm.append(v)
                hpos.append(p)
            hoff.append(len(hpos))
        self.hit_off = np.array(hoff, np.uint64)
        self.hit_pos = np.array(hpos, np.uint32)
        self.hit_fm = (np.array(pf, np.uint32) << 16) | np.array(pm, np.uint32)
        self.planted_keys = np.array(pk, np.uint64)
        # trap keys: last 7 residues + the gap byte
        tk, tf, tm = [], [], []
        for s in range(n):
            if lens[s] >= 7:
                b = self.p_residues[poff[s] + lens[s] - 7:poff[s] + lens[s] + 1].tobytes()
                tk.append(int.from_bytes(b, "little"))
                tf.append(FUNC_BASE + s)
                tm.append(int(lens[s]))
        self.trap_keys = np.array(tk, np.uint64)
        keys = np.concatenate([self.planted_keys, self.trap_keys])
        data = np.zeros(len(keys), oracle_ref.STORED_DTYPE)
        data["function_index"] = np.concatenate([pf, tf]) if len(keys) else []
        data["mean"] = np.concatenate([pm, tm]) if len(keys) else []
        o = np.argsort(keys, kind="stable")
        self.keys, self.data = keys[o], data[o]

    def distinct(self):
        """All windows pairwise distinct, and no trap key among them."""
        u = np.unique(self.all_window_keys)
        return len(u) == self.n_windows and len(np.unique(self.keys)) == len(self.keys) and \
            not np.isin(self.trap_keys, u).any()

    def hits_of(self, s):
        """Sequence s's planted hits as (position, function_index, mean)."""
        a, e = int(self.hit_off[s]), int(self.hit_off[s + 1])
        return [(int(p), int(w >> 16), int(w & 0xFFFF)) for p, w in zip(self.hit_pos[a:e], self.hit_fm[a:e])]

    def subset(self, idx):
        """(residues, seq_off, seq_len) of the sequences idx, back to back."""
        parts = [self.residues[int(self.seq_off[s]):int(self.seq_off[s]) + int(self.seq_len[s])] for s in idx]
        lens = np.array([len(p) for p in parts], np.uint32)
        off = np.zeros(len(parts), np.uint64)
        off[1:] = np.cumsum(lens[:-1].astype(np.int64))
        return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)), off, lens


@functools.lru_cache(maxsize=None)
def batch_for(min_hits, max_gap):
    """The materialised catalogue of (min_hits, max_gap), made once and shared (never modified)."""
    return Batch(catalogue(min_hits, max_gap))


def oracle_opts(opt):
    return dict(min_hits=opt[0], max_gap=opt[1], ignore_hypo=opt[2], hypo_index=HYPO, mean_mode=opt[3],
                mad_mode=opt[4])


@functools.lru_cache(maxsize=None)
def oracle_calls(opt):
    """(call_off, calls) of the C++ oracle over the exact DB for one option set, computed once."""
    b = batch_for(opt[0], opt[1])
    return oracle_ref.annotate_exact(b.keys, b.data, b.residues, b.seq_off, b.seq_len, **oracle_opts(opt))


def first_difference(scens, off_a, calls_a, off_b, calls_b):
    """The first sequence whose calls differ between two CSR results, for an assertion message."""
    for s, sc in enumerate(scens):
        a = calls_a[int(off_a[s]):int(off_a[s + 1])]
        b = calls_b[int(off_b[s]):int(off_b[s + 1])]
        if len(a) != len(b) or a.tobytes() != b.tobytes():
            return "sequence %d (%s): got %r, expected %r" % (s, sc.name, a[:4], b[:4])
    return None


# ---- the matrix distance's length filter -------------------------------------------------------

def matrix_cases():
    """[(name, mean, var, [(sequence length, kept by hand or None)])]: one shared 8-mer per case.
    var a square: lengths mean -/+ 2 sqrt(var) are kept, one further is dropped; var not a square:
    the lengths on both sides of 2 sqrt(var); var 0 (sd = 0.1 seqlen, decided in doubles, so no
    hand-written answer): the lengths around mean / 1.2 and mean / 0.8."""
    import math
    cases = []
    for var, mean in ((1, 40), (4, 40), (9, 40), (65025, 600)):
        r = 2 * math.isqrt(var)
        cases.append(("var%d" % var, mean, var, [(mean - r - 1, False), (mean - r, True), (mean, True),
                                                  (mean + r, True), (mean + r + 1, False)]))
    for var, mean in ((2, 40), (3, 40), (65535, 600)):
        r = math.isqrt(4 * var)  # floor(2 sqrt(var)); 4 var is no square
        assert r * r < 4 * var < (r + 1) * (r + 1)
        cases.append(("var%d" % var, mean, var, [(mean - r - 1, False), (mean - r, True), (mean, True),
                                                  (mean + r, True), (mean + r + 1, False)]))
    for seqlen in (30, 35, 45, 100):
        for fac in (12, 8):
            mean = seqlen * fac // 10
            assert mean * 10 == seqlen * fac
            lens = sorted({seqlen - 1, seqlen, seqlen + 1, round(mean / 1.2) - 1, round(mean / 1.2),
                           round(mean / 1.2) + 1, round(mean / 0.8) - 1, round(mean / 0.8), round(mean / 0.8) + 1})
            cases.append(("var0_len%d_mean%d" % (seqlen, mean), mean, 0, [(x, None) for x in lens]))
    return cases


class MatrixBatch:
    """matrix_cases() materialised: random sequences of the stated lengths with the case's 8-mer
    written at a random position; the DB holds one record (function, mean, var) per case."""

    def __init__(self, seed=9):
        rng = np.random.default_rng(seed)
        self.cases = matrix_cases()
        seqs, self.case_of, self.kept = [], [], []
        keys = []
        for c, (name, mean, var, lens) in enumerate(self.cases):
            kmer = AA[rng.integers(0, 20, 8)]
            keys.append(int.from_bytes(kmer.tobytes(), "little"))
            for length, kept in lens:
                assert length >= 8
                s = AA[rng.integers(0, 20, length)]
                p = int(rng.integers(0, length - 7))
                s[p:p + 8] = kmer
                seqs.append(s.tobytes())
                self.case_of.append(c)
                self.kept.append(kept)
        self.seqs = seqs
        self.seq_len = np.array([len(s) for s in seqs], np.uint32)
        self.seq_off = np.zeros(len(seqs), np.uint64)
        self.seq_off[1:] = np.cumsum(self.seq_len[:-1].astype(np.int64))
        self.residues = np.frombuffer(b"".join(seqs), np.uint8)
        keys = np.array(keys, np.uint64)
        data = np.zeros(len(keys), oracle_ref.STORED_DTYPE)
        data["function_index"] = FUNC_BASE + np.arange(len(keys))
        data["mean"] = [c[1] for c in self.cases]
        data["var"] = [c[2] for c in self.cases]
        o = np.argsort(keys)
        self.keys, self.data = keys[o], data[o]

    def distinct(self):
        """Every window is either its case's 8-mer (once per sequence) or in no DB record."""
        for s, c in zip(self.seqs, self.case_of):
            w = window_keys(np.frombuffer(s, np.uint8))
            hit = np.isin(w, self.keys)
            if hit.sum() != 1:
                return False
        return len(np.unique(self.keys)) == len(self.keys)

    def expected_by_hand(self):
        """{(id1, id2): 1} over the pairs of kept sequences of the cases with a hand-written answer."""
        out = {}
        for c in range(len(self.cases)):
            ids = [i for i in range(len(self.seqs)) if self.case_of[i] == c]
            if any(self.kept[i] is None for i in ids):
                continue
            k = [i for i in ids if self.kept[i]]
            for a in range(len(k)):
                for b in range(a + 1, len(k)):
                    out[(k[a], k[b])] = 1
        return out
