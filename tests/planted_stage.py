"""Planted pass sizes for the staging's exact starts -- a plain helper module of the tests.

With key-range passes, staging workgroup w of a pass stages the pass's entries [w * pf_span,
(w + 1) * pf_span) (the pass's windows in position order) and owns [wstart[w][d], wstart[w + 1][d])
of every level-0 slice d: k_pass_hist counts each span's entries per destination, k_pass_starts
scans the columns, k_extract_stage_pos appends from them without a global atomic.  stage_table()
restates that table from planted_front.Windows alone; the layouts here give chosen pass sizes:
isolated 8-mers (one window each, a filler X between two) whose hashes are drawn per pass, so a pass
holds exactly the planted number of entries, in position order at random destinations.
test_stage_starts_cpu.py proves the layouts and the restatement without a GPU."""
import functools

import numpy as np

import planted_front as pf
from planted import KEY_BITS, LETTERS, NCODES, Geometry, unmix43

N0 = 64                   # level-0 destinations (SC_L0_BITS = 6)
MIN_SPAN = 4 * pf.SC_ROUND   # entries per staging workgroup that size_local aims at: 16,384
PH_TILE = 2048            # k_pass_hist: entries per workgroup iteration (512 threads x 4)
PASSES = 4
NF = 40
PER_SEQ = 100             # planted 8-mers per protein

_LETTERS = np.frombuffer(LETTERS, np.uint8)


def pass_codes(rng, pass_bits, p, n, taken):
    """n distinct valid codes of pass p at random hashes below the pass bits, none in `taken`."""
    low = KEY_BITS - pass_bits
    out = []
    while len(out) < n:
        h = (np.uint64(p) << np.uint64(low)) | rng.integers(0, 1 << low, 2 * (n - len(out)) + 16, dtype=np.uint64)
        for c in unmix43(h).tolist():
            if c < NCODES and c not in taken and len(out) < n:
                taken.add(c)
                out.append(c)
    return out


def kmers_of(codes):
    """(n, 8) residue bytes of base-40 codes, the first residue the most significant digit."""
    c = np.asarray(codes, np.uint64)
    out = np.zeros((len(c), 8), np.uint8)
    for j in range(7, -1, -1):
        out[:, j] = _LETTERS[(c % np.uint64(40)).astype(np.int64)]
        c = c // np.uint64(40)
    return out


class Planted:
    """arrays (the build's input), nf, windows (planted_front.Windows), distinct kept keys."""

    def __init__(self, seqs, funcs, nf, distinct):
        lens = np.array([len(s) for s in seqs], np.uint32)
        off = np.zeros(len(seqs), np.uint64)
        off[1:] = np.cumsum(lens[:-1].astype(np.uint64))
        self.arrays = (np.frombuffer(b"".join(seqs), np.uint8), off, lens, np.array(funcs, np.uint16),
                       np.arange(len(seqs), dtype=np.uint32))
        self.nf = nf
        self.windows = pf.Windows(self.arrays)
        self.distinct = distinct


def proteins(kmers, per):
    """Proteins of `per` 8-mers each, an X after every 8-mer but the protein's last."""
    rows = np.full((len(kmers), 9), ord("X"), np.uint8)
    rows[:, :8] = kmers
    return [rows[a:a + per].tobytes()[:-1] for a in range(0, len(kmers), per)]


def _layout_s(seed, counts):
    """counts[p] isolated windows in pass p of 4, the passes shuffled together in position order."""
    rng = np.random.default_rng(seed)
    taken, codes = set(), []
    for p, n in enumerate(counts):
        codes += pass_codes(rng, 2, p, n, taken)
    codes = np.array(codes, np.uint64)[rng.permutation(len(codes))]
    seqs = proteins(kmers_of(codes), PER_SEQ)
    funcs = [(7 * s + 3) % NF for s in range(len(seqs))]
    lay = Planted(seqs, funcs, NF, len(codes))
    lay.counts = list(counts)
    return lay


# pass 0: fewer than 2048 entries; pass 1: empty; pass 2: two spans, the second partial; pass 3 (the
# last emission group at every emit_group): the largest pass, which sets pf_span and pf_nwg
# (size_local: pf = ceil(W / 16384), pf_span = 4096 * ceil(ceil(W / pf) / 4096), pf_nwg = ceil(W / pf_span)).
# A last span of exactly one entry needs W = k * pf_span + 1 with pf = k + 1 workgroups, which first
# happens at pf = 4: W = 3 * 16384 + 1.  (W = 2 * 16384 + 1 gives three spans of 12,288: layout_s2.)
S_SMALL, S_MID = 1500, 20001


@functools.lru_cache(maxsize=None)
def layout_s1():
    """Pass 3 holds 3 * 16384 + 1 entries: four spans of 16,384, the last holds exactly one."""
    return _layout_s(5101, (S_SMALL, 0, S_MID, 3 * MIN_SPAN + 1))


@functools.lru_cache(maxsize=None)
def layout_s2():
    """Pass 3 holds 2 * 16384 + 1 entries: three spans of 12,288, the last partial."""
    return _layout_s(5104, (S_SMALL, 0, S_MID, 2 * MIN_SPAN + 1))


@functools.lru_cache(maxsize=None)
def layout_s3():
    """Pass 3 holds exactly 3 * 16384 entries: three full spans of 16,384."""
    return _layout_s(5102, (S_SMALL, 0, S_MID, 3 * MIN_SPAN))


LAYOUTS_S = {"s1": layout_s1, "s2": layout_s2, "s3": layout_s3}
# name: (pf_span, pf_nwg, entries of the largest pass's last span)
S_CLAIMS = {"s1": (MIN_SPAN, 4, 1), "s2": (3 * pf.SC_ROUND, 3, 2 * MIN_SPAN + 1 - 6 * pf.SC_ROUND),
            "s3": (MIN_SPAN, 3, MIN_SPAN)}


H_COPIES = 40000
H_OTHERS = 400


@functools.lru_cache(maxsize=None)
def layout_h():
    """H_COPIES copies of one 8-residue protein (a homopolymer whose hash lies in the upper half of
    the passes, so routing moves it), then H_OTHERS distinct windows: the first two spans of the
    heavy key's pass hold that key alone."""
    rng = np.random.default_rng(5103)
    letter = pf.upper_half_letter()
    heavy = bytes([letter]) * 8
    taken = set()
    others = []
    for p in range(PASSES):
        others += pass_codes(rng, 2, p, H_OTHERS // PASSES, taken)
    others = np.array(others, np.uint64)[rng.permutation(len(others))]
    seqs = [heavy] * H_COPIES + proteins(kmers_of(others), 20)
    funcs = [5] * H_COPIES + [(7 * s + 3) % NF for s in range(len(seqs) - H_COPIES)]
    lay = Planted(seqs, funcs, NF, len(others) + 1)
    lay.heavy_pass = pf.homopolymer_hash(letter) >> (KEY_BITS - 2)
    assert int.from_bytes(heavy, "little") not in set(lay.windows.keys[H_COPIES:].tolist())
    return lay


def destinations(W, passes, world=1):
    """Per window of W: its pass and its level-0 destination (the top 6 of the owner and level-1
    bucket bits of the hash)."""
    pb = passes.bit_length() - 1
    g = Geometry(pb, (world - 1).bit_length())
    nbits = g.owner_bits + g.b1_bits
    prefix = g.prefix_of(W.hash)
    d = (prefix & np.uint64((1 << nbits) - 1)) >> np.uint64(nbits - 6)
    return (prefix >> np.uint64(nbits)).astype(np.int64), d.astype(np.int64)


def stage_table(W, passes, q, pf_span, pf_nwg, world=1):
    """The (pf_nwg + 1) x 64 table of pass q: row w, column d = the start of slice d plus the
    entries of the spans before w that go to d."""
    ps, d = destinations(W, passes, world)
    d = d[ps == q]                      # the pass's windows in position order
    assert len(d) <= pf_span * pf_nwg
    cnt = np.zeros((pf_nwg, N0), np.int64)
    for w in range(pf_nwg):
        cnt[w] = np.bincount(d[w * pf_span:(w + 1) * pf_span], minlength=N0)
    start = np.zeros(N0, np.int64)
    start[1:] = np.cumsum(cnt.sum(0))[:-1]
    t = np.zeros((pf_nwg + 1, N0), np.int64)
    t[0] = start
    t[1:] = start + np.cumsum(cnt, 0)
    return t.astype(np.uint64)


def check_invariants(t, total):
    """What holds for every table, whatever the spans: each column is non-decreasing in w, the last
    row is the next slice's start, and the last slice ends at the pass's entry count."""
    t = t.astype(np.int64)
    assert t[0, 0] == 0
    assert np.all(np.diff(t, axis=0) >= 0)
    assert np.array_equal(t[-1, :-1], t[0, 1:])
    assert t[-1, -1] == total


def span_counts(n, pf_span, pf_nwg):
    """Entries of each of the pf_nwg spans of a pass of n entries."""
    return [max(0, min(pf_span, n - w * pf_span)) for w in range(pf_nwg)]
