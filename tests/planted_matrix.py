"""Planted groups for the matrix distance's pair-count kernels -- a plain helper module of the tests.

Everything after k_md_hits in skm_matrix.hip (k_md_slot, the radix sort, k_md_starts / k_md_segstart,
k_md_rowstat / k_md_rowfill, k_md_rows, k_md_rows_seg, the gathers) sees only (k-mer, index) hits.
Over an exact-key DB (KeptKmerDb) that list can be written by hand: a Plan is one matrix-distance
problem, a list of sequences (index, length, the k-mers it hosts).  A sparse sequence hosts its
k-mers STRIDE residues apart inside random residues; a dense one is a block of random residues
every window of which is a DB key (that is how a row gets 65,535 entries).  A k-mer is shared by
exactly the sequences the plan names: Material redraws residues until the planted k-mers are
pairwise distinct and no unplanted window of any sequence is a DB key, and asserts both (random
8-mers do collide at this size -- about 3e5 windows against 20^8 keys give 1.8 expected collisions
-- so a different seed is no answer).

Length filter: all hosts of a k-mer have one length `len` and the record says mean = len, var = 0
(kept: sd = 0.1 len).  The mean is a u16; hosts longer than 65,535 get mean 60,000, which keeps
every length up to 81,918.

A plan carries `claims` (what it is built to be), `hand` (the exact {(id1, id2): count} where it
can be written in closed form); pairs(plan) derives the same from the plan's membership lists
alone, with no matrix-distance routine.  Model restates the kernels' path decisions from the plan:
per row the entries (distinct (k-mer, index) with a member after it in its group, a trailing
duplicate counting as a member, as md_entry does), ncol, wide, passes, sweeps and the partner total
of a sweep; per problem the hits, key_bits and radix rounds.  tests/test_planted_matrix_cpu.py
proves all of it and compares the constants below with those in skm_matrix.hip.

Known limit, not tested: rowub is a u32 sum of partner counts per row and would wrap for a row
whose entries x group tails reach 2^32; no input of test size gets near that.
"""
from __future__ import annotations

import collections
import functools
import os
import re

import numpy as np

import oracle_ref
from planted_hits import AA, FUNC_BASE, HYPO, function_index, window_keys  # noqa: F401  (re-exported)

# mirrored from skm_matrix.hip (source_constants() reads the real ones)
MR_THREADS = 1024   # k_md_rows: entries per sweep
MR_WORDS = 32768    # histogram words: 65,536 u16 columns or 32,768 u32 columns per pass
MR_UNROLL = 4       # partners per thread and step: MR_THREADS * MR_UNROLL per step
SEG_COLS = 1024     # k_md_rows_seg: problems of at most this many indices
SEG_SUB = 16
SEG_RB = 4
RS_TILE = 4096      # radix sort tile
MIRRORED = ("MR_THREADS", "MR_WORDS", "MR_UNROLL", "SEG_COLS", "SEG_SUB", "SEG_RB", "RS_TILE")

STRIDE = 9          # planted k-mers of a sparse sequence start every STRIDE residues
LONG_MEAN = 60000   # the record's mean for hosts longer than a u16
BLOCK = 230         # windows per short dense sequence of a spread row


def source_constants():
    """Every `constexpr int|uint32_t NAME = expression` of skm_matrix.hip that evaluates to an integer."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "signature_kmers_amd", "csrc",
                        "skm_matrix.hip")
    env = {}
    for decl in re.findall(r"constexpr\s+(?:int|uint32_t)\s+([^;]+);", open(path).read()):
        for part in decl.split(","):
            if "=" not in part:
                continue
            name, expr = (x.strip() for x in part.split("=", 1))
            expr = re.sub(r"(\d)u\b", r"\1", expr).replace("/", "//")
            try:
                env[name] = int(eval(expr, {"__builtins__": {}}, dict(env)))  # noqa: S307 (our own source)
            except Exception:
                pass
    return env


def ceil_log2(x):
    b = 0
    while (1 << b) < x:
        b += 1
    return b


def is_hypo(key):
    """A k-mer whose local id is a tuple ("H", ...) carries the hypothetical protein's record."""
    return isinstance(key[1], tuple) and key[1][:1] == ("H",)


class Seq:
    def __init__(self, idx, length, kmers=(), block=None):
        self.idx, self.length, self.kmers, self.block = int(idx), int(length), list(kmers), block


class Plan:
    """One problem.  n_idx: its index count; L: the default length of a sparse sequence; bands: also
    run as row tiles; far: local ids of sparse k-mers planted on the problem's last column(s), which
    a batch also plants in the first sequences of the next problem."""

    def __init__(self, name, n_idx, L=STRIDE, claims=None, hand=None, bands=False, far=()):
        self.name, self.n_idx, self.L = name, int(n_idx), int(L)
        self.claims, self.hand, self.bands, self.far = claims or {}, hand, bands, list(far)
        self.seqs = []

    def key(self, kid):
        return (self.name, kid)

    def add(self, idx, kmers, length=None):
        kmers = list(kmers)
        length = max(self.L, STRIDE * len(kmers)) if length is None else length
        assert 0 <= idx < self.n_idx and (not kmers or STRIDE * (len(kmers) - 1) + 8 <= length), self.name
        self.seqs.append(Seq(idx, length, [self.key(k) for k in kmers]))

    def group(self, kid, idxs, length=None):
        for i in idxs:
            self.add(i, [kid], length)

    def dense(self, idx, block, W):
        assert 0 <= idx < self.n_idx and W >= 1
        self.seqs.append(Seq(idx, W + 7, block=(self.key(block), int(W))))

    def blank(self, idx, length):
        self.seqs.append(Seq(idx, length))


# ---- what a plan says, without any matrix-distance routine ---------------------------------------

def classes(plan):
    """[(members, multiplicity)]: members = the sorted indices of a k-mer's surviving hits (one per
    occurrence, duplicates kept); k-mers with equal member lists are counted together (the windows
    of a dense block all have their block's)."""
    mem = {}
    for s in plan.seqs:
        if s.block is not None:
            mem.setdefault(("__block__",) + s.block, []).append(s.idx)
        else:
            for k in s.kmers:
                if not is_hypo(k):
                    mem.setdefault(k, []).append(s.idx)
    out = collections.Counter()
    for k, m in mem.items():
        out[tuple(sorted(m))] += k[2] if k[0] == "__block__" else 1
    return sorted(out.items())


def pairs(plan):
    """{(id1, id2): count}: every pair of distinct indices of a k-mer's member list counts once."""
    if getattr(plan, "_pairs", None) is None:
        out = {}
        for m, mult in classes(plan):
            d = sorted(set(m))
            for a in range(len(d)):
                for b in range(a + 1, len(d)):
                    out[(d[a], d[b])] = out.get((d[a], d[b]), 0) + mult
        plan._pairs = out
    return plan._pairs


def as_array(d):
    """{(id1, id2): count} -> (n, 3) u32 sorted by (id1, id2), as MatrixDistance.pairs() gives it."""
    if not d:
        return np.zeros((0, 3), np.uint32)
    a = np.array([(k[0], k[1], v) for k, v in d.items()], np.uint32)
    return a[np.lexsort((a[:, 1], a[:, 0]))]


def hits_groups(plan):
    """(surviving hits, distinct hit k-mers) of a plan."""
    cl = classes(plan)
    return sum(len(m) * k for m, k in cl), sum(k for m, k in cl)


class Row:
    pass


class Model:
    """The path decisions of md_group and k_md_rows for one plan; rows [r0, r1) only, as a row tile."""

    def __init__(self, plan, r0=0, r1=None):
        r1 = plan.n_idx if r1 is None else r1
        cl = classes(plan)
        self.hits = sum(len(m) * k for m, k in cl)
        self.groups = sum(k for m, k in cl)
        self.idx_bits = max(1, ceil_log2(max(plan.n_idx, 2)))
        self.lg = max(4, ceil_log2(2 * max(self.hits, 1)))
        self.key_bits = self.lg + self.idx_bits
        self.rounds = -(-self.key_bits // 8) if self.hits else 0
        self.sort_tiles = -(-self.hits // RS_TILE)
        per_row = {}
        for m, k in cl:
            for j in range(len(m) - 1):
                if j and m[j - 1] == m[j]:
                    continue
                if r0 <= m[j] < r1:
                    per_row.setdefault(m[j], []).append((k, np.array(m[j + 1:], np.int64)))
        self.rows = {}
        for r, ents in per_row.items():
            R = Row()
            R.entries = sum(k for k, _ in ents)
            R.ncol = plan.n_idx - r - 1
            R.wide = R.entries > 65535
            R.cpp = MR_WORDS if R.wide else 2 * MR_WORDS
            R.passes = -(-R.ncol // R.cpp)
            R.multi = R.ncol > R.cpp
            R.sweeps = -(-R.entries // MR_THREADS)
            R.rowub = sum(k * len(p) for k, p in ents)
            tot = np.zeros(max(R.passes, 1), np.int64)
            kinds, cols = set(), set()
            for k, p in ents:
                c = p - r - 1  # local columns; a duplicate of the row's own index has column -1
                c = c[c >= 0]
                if R.passes:
                    cnt = np.bincount(c // R.cpp, minlength=R.passes)
                    tot += k * cnt
                    kinds.add(tuple(int(x) for x in np.nonzero(cnt)[0]))
                cols.update(int(x) for x in c)
            R.pass_kinds = kinds
            R.columns = cols
            R.nnz = len(cols) if R.passes else 0
            R.sweep_total = int(tot.max()) if R.entries <= MR_THREADS else None
            R.steps = -(-R.sweep_total // (MR_THREADS * MR_UNROLL)) if R.sweep_total is not None else None
            self.rows[r] = R
        self.total_entries = sum(R.entries for R in self.rows.values())


# ---- the catalogue -------------------------------------------------------------------------------

def _spread(W):
    return [BLOCK] * (W // BLOCK) + ([W % BLOCK] if W % BLOCK else [])


def _all_pairs(ids, count=1):
    ids = sorted(ids)
    return {(ids[a], ids[b]): count for a in range(len(ids)) for b in range(a + 1, len(ids))}


GROUP_NIDX = 65537   # row 0 has exactly 65,536 columns: one pass, `multi` false
GROUP_EDGE = [64, 65, 65472, 65473, 65536]  # row 0's local columns 63 | 64, 65471 | 65472 and the last


def _group_set(G):
    """G indices: 0, then the edge columns' indices from the last one down, then 1, 2, ..."""
    if G <= 3:
        return [0, 64, 65][3 - G:] if G == 3 else [0, 65]
    rest = [i for i in range(1, G) if i not in GROUP_EDGE]
    return sorted([0] + GROUP_EDGE + rest[:G - 1 - len(GROUP_EDGE)])


GROUP_SETS = {G: _group_set(G) for G in (2, 3, 64, 65, 1024, 1025)}
COLPASS_NIDX = 5 + 1 + 2 * 65536 + 9


def catalogue():
    P = []

    def new(*a, **k):
        P.append(Plan(*a, **k))
        return P[-1]

    # -- tiny and degenerate
    p = new("two_share_one", 2, claims=dict(hits=2, groups=1, lg=4, rounds=1, row=0, entries=1), hand={(0, 1): 1})
    p.group("a", [0, 1])
    p = new("alone", 1, claims=dict(hits=3, groups=3, total_entries=0), hand={})
    p.add(0, ["a", "b", "c"])
    p = new("twice_in_one", 3, claims=dict(hits=2, groups=1, row=0, entries=1, nnz=0), hand={})
    p.add(0, ["a", "a"])
    p = new("hypo_shared", 2, claims=dict(hits=0, groups=0, total_entries=0), hand={})
    p.group(("H", 0), [0, 1])
    p = new("short_and_empty", 5, L=18, claims=dict(hits=2, groups=1), hand={(0, 3): 1})
    p.add(0, ["a", ("H", 0)])
    p.blank(1, 5)
    p.blank(2, 0)
    p.add(3, [("H", 0), "a"])
    p.blank(4, 7)
    # -- hit counts: partial waves and tiles of the sort; radix rounds 2, 4 and 5
    for n, nidx, rounds in ((255, 2, 2), (256, 2, 2), (257, 2, 2), (4095, 2, 2), (4096, 2, 2), (4097, 70001, 4),
                            (8193, 262146, 5)):
        a, b, hi = (n + 1) // 2, n // 2, nidx - 1
        p = new("hits_%d" % n, nidx, claims=dict(hits=n, groups=a, rounds=rounds, row=0, entries=b), hand={(0, hi): b})
        p.add(0, range(a), STRIDE * a)
        p.add(hi, range(b), STRIDE * a)
    # -- group sizes, with row 0's nonzero columns on both sides of a compaction thread's words
    for G, ids in GROUP_SETS.items():
        p = new("group_%d" % G, GROUP_NIDX, bands=True, hand=_all_pairs(ids),
                claims=dict(hits=G, groups=1, row=0, entries=1, ncol=65536, passes=1, multi=False, wide=False,
                            sweep_total=G - 1, nnz=G - 1))
        assert len(set(ids)) == G and set(GROUP_EDGE if G > 3 else [65]) <= set(ids)
        p.group("g", ids)
    # -- entries and sweeps
    for E in (1023, 1024, 1025, 2049):
        p = new("entries_%d" % E, 2, hand={(0, 1): E},
                claims=dict(row=0, entries=E, sweeps=-(-E // 1024), wide=False, passes=1))
        p.add(0, range(E))
        p.add(1, range(E))
    for extra, tot in ((4, 4095), (5, 4096), (6, 4097)):
        hand = {(a, b): (1023 if b < 5 else 0) + (1 if b < extra else 0) for a in range(6) for b in range(a + 1, 6)}
        p = new("sweep_%d" % tot, 6, hand={k: v for k, v in hand.items() if v},
                claims=dict(row=0, entries=1024, sweeps=1, sweep_total=tot, steps=-(-tot // 4096)))
        for i in range(6):
            kids = (list(range(1023)) if i < 5 else []) + (["x"] if i < extra else [])
            if kids:
                p.add(i, kids, STRIDE * 1024)
    hand = _all_pairs(range(1025))
    hand[(0, 1)] = 1001
    p = new("one_big_entry", 1025, hand=hand, claims=dict(row=0, entries=1001, sweeps=1, sweep_total=2024))
    p.group("big", range(1025))
    p.add(0, range(1000))
    p.add(1, range(1000))
    # -- the u16 boundary and the wide form
    for W in (65535, 65536):
        cl = dict(hits=3 * W, groups=W, rounds=3, row=0, entries=W, wide=W > 65535, passes=1, count=W)
        p = new("dense3_%d" % W, 3, hand=_all_pairs(range(3), W), claims=cl)
        for i in range(3):
            p.dense(i, "D", W)
        p = new("spread3_%d" % W, 3, hand=_all_pairs(range(3), W), claims=cl)
        for i in range(3):
            for b, w in enumerate(_spread(W)):
                p.dense(i, ("S", b), w)
    # -- column passes: rows 0 and 5, partners at chosen local columns of three passes
    p = new("colpass", COLPASS_NIDX, bands=True, far=[("C", 0), ("C", 5), ("D", 0), ("D", 5)],
            claims=dict(row=5, entries=4, ncol=2 * 65536 + 9, passes=3, multi=True, wide=False,
                        pass_kinds={(0,), (1,), (0, 1, 2), (2,)}))
    for id1 in (0, 5):
        last = COLPASS_NIDX - id1 - 2
        for nm, cols in (("A", [0, 1, 65534, 65535]), ("B", [65536, 65537, 131071]),
                         ("C", [0, 65535, 65536, 131071, 131072, last]), ("D", [131072, last])):
            p.group((nm, id1), [id1] + [id1 + 1 + c for c in cols])
    for nc in (65536, 65537):
        p = new("ncol_%d" % nc, nc + 1, far=["b"], hand={**_all_pairs([0, 1, 65536]), **_all_pairs([0, 65535, nc]),
                                                         **({(0, 65536): 2} if nc == 65536 else {})},
                claims=dict(row=0, entries=2, ncol=nc, passes=-(-nc // 65536), multi=nc > 65536, wide=False))
        p.group("a", [0, 1, 65536])
        p.group("b", [0, 65535, nc])
    S = [0, 1, 32, 33, 32768, 32769]
    hand = _all_pairs(S, BLOCK)
    hand[(0, 1)] = 65536
    hand[(0, 32769)] = BLOCK + 40 + 1
    p = new("wide_2pass", 32770, far=["far"], hand=hand,
            claims=dict(row=0, entries=65536 + 40 + 1, wide=True, ncol=32769, passes=2, multi=True, rounds=5,
                        pass_kinds={(0,), (1,), (0, 1)}))
    for b, w in enumerate(_spread(65536)):
        p.dense(0, ("S", b), w)
        p.dense(1, ("S", b), w)
    for i in S[2:]:
        p.dense(i, ("S", 0), BLOCK)  # row 0's columns 31 | 32, the last of pass 0, the one of pass 1
    p.dense(0, "T", 40)
    p.dense(32769, "T", 40)
    p.group("far", [0, 32769])
    # -- duplicates of a (k-mer, index), inside a sequence and as two sequences under one index
    p = new("dups_small", 12, L=27, claims=dict(row=11, entries=1, ncol=0, passes=0, nnz=0),
            hand={(0, 3): 1, (0, 7): 1, (3, 7): 1, (1, 4): 1, (1, 9): 1, (4, 9): 1, (2, 5): 1, (6, 8): 1, (3, 11): 1})
    p.add(0, ["a", "a"])       # the group's first member, twice inside a sequence
    p.add(3, ["a"])
    p.add(7, ["a"])
    p.add(1, ["b"])
    p.add(4, ["b"])
    p.add(9, ["b"])            # the group's last member, as two sequences
    p.add(9, ["b"])
    p.add(2, ["c", "c", "c"])  # three times
    p.add(5, ["c"])
    p.add(6, ["d"])
    p.add(8, ["d", "d"])       # the only other member
    p.add(3, ["e"])
    p.add(11, ["e"])           # the last index: its row has an entry and no column
    p.add(11, ["e"])
    p.add(10, ["f"])           # a group of one index only, both ways at once
    p.add(10, ["f", "f"])
    n3 = 2 * 65536 + 3         # row 0: passes of 65,536, 65,536 and 2 columns
    F = [0, 1, 65536, 65537, 131072, 131073, 131074]
    hand = _all_pairs(F)
    hand[(0, 65537)] = 2
    hand[(0, 131074)] = 2
    p = new("dups_pass", n3, L=18, far=["f", "h"], hand=hand,
            claims=dict(row=0, entries=3, ncol=n3 - 1, passes=3, multi=True, pass_kinds={(0, 1, 2), (1,), (2,)}))
    p.add(0, ["f"])
    p.add(1, ["f", "f"])        # pass 0's first column
    p.add(65536, ["f"])         # pass 0's last column
    p.add(65536, ["f"])
    p.add(65537, ["f", "f"])    # pass 1's first column
    p.add(131072, ["f"])        # pass 1's last column
    p.add(131072, ["f"])
    p.add(131073, ["f", "f"])   # pass 2's first column
    p.add(131074, ["f"])        # the last column
    p.add(131074, ["f"])
    p.add(0, ["g", "g"])        # the first member twice, its partner in pass 1 only
    p.add(65537, ["g"])
    p.add(0, ["h"])             # the only other member three times, in pass 2
    p.add(131074, ["h", "h"])
    p.add(131074, ["h"])
    # -- for the batch: a problem of exactly SEG_COLS indices, rows around the one-wave sweep
    p = new("prob_1024", SEG_COLS, far=["a", "b", "c"], claims=dict(row=0, entries=2, ncol=1023),
            hand={(0, 1023): 2, (1022, 1023): 1, (0, 1): 1, (1, 1023): 1})
    p.group("a", [0, 1023])
    p.group("b", [1022, 1023])
    p.group("c", [0, 1, 1023])
    p = new("wave_sweep", 8, claims=dict(row=3, entries=129), hand={(0, 4): 63, (1, 5): 64, (2, 6): 65, (3, 7): 129})
    for r, E in enumerate((63, 64, 65, 129)):
        p.add(r, [(r, i) for i in range(E)], STRIDE * 129)
        p.add(r + 4, [(r, i) for i in range(E)], STRIDE * 129)
    p = new("tail", 2, hand={(0, 1): 1})
    p.group("a", [0, 1])
    return P


NAMES = [p.name for p in catalogue()]
BAND_NAMES = [p.name for p in catalogue() if p.bands]


def batch_plans():
    """The catalogue as adjacent problems; every far-column k-mer of a problem is also planted in
    first sequences of the next problem (local index 0: the global index just past the problem's
    end), one sequence of the hosts' length per k-mer.  It pairs with nothing there."""
    P = catalogue()
    assert not P[-1].far
    for p, nxt in zip(P[:-1], P[1:]):
        for k, kid in enumerate(p.far):
            nxt.seqs.insert(k, Seq(0, p.L, [p.key(kid)]))
    return P


# ---- materialise ---------------------------------------------------------------------------------

class Material:
    """Plans made residues and one exact-key DB.
    flat / seq_off / seq_len / seq_idx   all sequences back to back, indices local to their plan
    prob_seq / prob_nidx                 the plans as the problems of a batch
    keys / data                          the DB, keys ascending"""

    def __init__(self, plans, seed=3):
        self.plans = plans
        rng = np.random.default_rng(seed)
        seqs = [s for p in plans for s in p.seqs]
        skeys, blocks, klen = {}, {}, {}
        for s in seqs:
            for k in s.kmers:
                skeys.setdefault(k, len(skeys))
                assert klen.setdefault(k, s.length) == s.length, ("hosts of one k-mer differ in length", k)
            if s.block is not None:
                blocks.setdefault(s.block[0], s.block[1])
                assert blocks[s.block[0]] == s.block[1]
        # the planted k-mers: pairwise distinct, by redrawing the ones that are not
        kres = AA[rng.integers(0, 20, (len(skeys), 8))]
        bres = {b: AA[rng.integers(0, 20, W + 7)] for b, W in blocks.items()}
        bnames = list(bres)
        for _ in range(100):
            parts = [np.ascontiguousarray(kres).view("<u8").ravel()] + [window_keys(bres[b]) for b in bnames]
            bounds = np.cumsum([0] + [len(x) for x in parts])
            allk = np.concatenate(parts)
            o = np.argsort(allk, kind="stable")
            bad = o[1:][allk[o][1:] == allk[o][:-1]]
            if not len(bad):
                break
            for i in bad:
                src = int(np.searchsorted(bounds, i, side="right")) - 1
                if src == 0:
                    kres[i] = AA[rng.integers(0, 20, 8)]
                else:
                    w = int(i - bounds[src])
                    bres[bnames[src - 1]][w:w + 8] = AA[rng.integers(0, 20, 8)]
        assert len(np.unique(allk)) == len(allk), "planted k-mers are not pairwise distinct"
        self.n_planted = len(allk)
        # records
        func = np.zeros(len(allk), np.int64)
        lens_of = np.zeros(len(allk), np.int64)
        for k, i in skeys.items():
            func[i] = HYPO if is_hypo(k) else FUNC_BASE + i % 50000
            lens_of[i] = klen[k]
        for j, b in enumerate(bnames):
            func[bounds[j + 1]:bounds[j + 2]] = FUNC_BASE + 50000 + j % 1000
            lens_of[bounds[j + 1]:bounds[j + 2]] = blocks[b] + 7
        mean = np.where(lens_of <= 0xFFFF, lens_of, LONG_MEAN)
        sl, mu = lens_of.astype(np.float64), mean.astype(np.float64)
        assert not ((sl < mu - sl * 0.1 * 2.0) | (sl > mu + sl * 0.1 * 2.0)).any(), "a host fails the length filter"
        data = np.zeros(len(allk), oracle_ref.STORED_DTYPE)
        data["function_index"], data["mean"] = func, mean
        o = np.argsort(allk)
        self.keys, self.data = allk[o], data[o]
        # the sequences
        self.seq_len = np.array([s.length for s in seqs], np.uint32)
        self.seq_idx = np.array([s.idx for s in seqs], np.uint32)
        lens = self.seq_len.astype(np.int64)
        self.seq_off = np.zeros(len(seqs), np.uint64)
        self.seq_off[1:] = np.cumsum(lens[:-1])
        off = self.seq_off.astype(np.int64)
        total = int(lens.sum())
        flat = AA[rng.integers(0, 20, total)]
        fixed = np.zeros(total, bool)      # residues of planted k-mers
        nw = max(total - 7, 0)
        planted = np.zeros(nw, bool)       # windows that are planted k-mers
        valid = np.zeros(nw, bool)         # windows inside one sequence
        ppos, pk = [], []
        for s, a in zip(seqs, off):
            if s.length >= 8:
                valid[a:a + s.length - 7] = True
            if s.block is not None:
                flat[a:a + s.length] = bres[s.block[0]]
                fixed[a:a + s.length] = True
                planted[a:a + s.length - 7] = True
            elif s.kmers:
                ppos.append(a + STRIDE * np.arange(len(s.kmers)))
                pk.append(np.array([skeys[k] for k in s.kmers]))
        if ppos:
            ppos, pk = np.concatenate(ppos), np.concatenate(pk)
            at = ppos[:, None] + np.arange(8)
            flat[at] = kres[pk]
            fixed[at] = True
            planted[ppos] = True
        # no unplanted window is a DB key: redraw the free residues of those that are
        for _ in range(100):
            wk = window_keys(flat)
            un = np.nonzero(valid & ~planted)[0]
            hit = un[np.isin(wk[un], self.keys)]
            if not len(hit):
                break
            for w in hit:
                free = np.nonzero(~fixed[w:w + 8])[0] + w
                assert len(free), "an unplanted window made of planted residues only"
                flat[free] = AA[rng.integers(0, 20, len(free))]
        self.flat, self._valid, self._planted = flat, valid, planted
        assert self.no_accidental_hits(), "an unplanted window is a DB key"
        self.n_windows = int(valid.sum())
        cnt = np.array([len(p.seqs) for p in plans], np.int64)
        self.prob_seq = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
        self.prob_nidx = np.array([p.n_idx for p in plans], np.uint32)

    def planted_distinct(self):
        return len(np.unique(self.keys)) == len(self.keys) == self.n_planted

    def no_accidental_hits(self):
        """Recomputed from the residues: the windows that are DB keys are exactly the planted ones."""
        wk = window_keys(self.flat)
        return np.array_equal(np.isin(wk, self.keys) & self._valid, self._planted & self._valid)

    def problem(self, p):
        """(residues, seq_off, seq_len, seq_idx, n_idx) of plan p alone."""
        a, e = int(self.prob_seq[p]), int(self.prob_seq[p + 1])
        lens = self.seq_len[a:e]
        if a == e:
            return np.zeros(0, np.uint8), np.zeros(0, np.uint64), lens, self.seq_idx[a:e], self.plans[p].n_idx
        b0 = int(self.seq_off[a])
        b1 = int(self.seq_off[e - 1]) + int(lens[-1])
        return self.flat[b0:b1], self.seq_off[a:e] - np.uint64(b0), lens, self.seq_idx[a:e], self.plans[p].n_idx

    def seqs_of(self, p):
        res, off, lens, _, _ = self.problem(p)
        return [res[int(o):int(o) + int(n)].tobytes() for o, n in zip(off, lens)]

    def oracle(self, p):
        res, off, lens, idx, _ = self.problem(p)
        if not len(lens):
            return np.zeros((0, 3), np.uint32)
        return oracle_ref.matrix_distance_exact(self.keys, self.data, res, off, lens, idx, HYPO)


@functools.lru_cache(maxsize=None)
def single(name):
    """(plan, Material of that plan alone), made once and shared (never modified)."""
    plan = next(p for p in catalogue() if p.name == name)
    return plan, Material([plan], seed=3 + NAMES.index(name))


@functools.lru_cache(maxsize=None)
def batch():
    """Material of batch_plans(), made once and shared."""
    return Material(batch_plans(), seed=77)


@functools.lru_cache(maxsize=None)
def expect_array(name):
    return as_array(pairs(single(name)[0]))


@functools.lru_cache(maxsize=None)
def oracle_array(name):
    return single(name)[1].oracle(0)
