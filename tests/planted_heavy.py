"""Planted inputs for the path the heaviest k-mers take -- a plain helper module of the tests:
k_ovf_plan, k_ovf_split, k_heavy (the bucketed sample order and the Boyer-Moore + radix-sort path),
k_overflow with group_block, and the giant-chain hand-off (skm_build.hip).

It builds on planted.py.  One scenario is one level-1 bucket whose planted keys share the top 11
bits of rem, so whatever level-2 split k_partition chooses they are one overflow sub-bucket: one
entry of k_ovf_plan's list.  What the heavy path needs beyond the group-by's planting:

  - chosen sequence indices: k_heavy's buckets are bk = s * NBK / n_total of a member's global
    sequence index s, and the radix rounds follow the largest best member's index, so a scenario
    plans the index of a protein (Indexer) and assemble_planned() shuffles only the rest;
  - chosen offsets and lengths: a protein is X*lead + 8-mer + X*trail, so the member's offset from
    the end is 8 + trail and its length lead + 8 + trail (proteins beyond 65535 residues for the
    16-bit wraps);
  - several occurrences in one protein: (8-mer + X) repeated, every window valid;
  - filler sequences of one residue (no window) that set n_total.

model() restates the kernels' decisions with the constants mirrored below (test_planted_heavy_cpu.py
asserts the mirrors against the source text and every scenario's claims against the model); every
scenario declares the edges it is there for (`edges`) and what the model must say (`claims`)."""
import os
import re

import numpy as np

from planted import (CAP, HEAVY_MIN, HV_FT, Geometry, Scenario, b2_of, best_mix, hash_of_keys, kmer_of, pack,
                     windows_of)

SPLIT_MIN = CAP + 1       # k_ovf_plan / k_ovf_split: entries of at least this many elements are split
SPLIT_TAB = 4096          # k_ovf_split's LDS key table
SPLIT_MAXH = 256          # heavy keys taken out of one entry
SPLIT_U = 8               # elements per thread per iteration (512 threads: 4096 per iteration)
HV_NBK = 4096             # k_heavy: sequence-index buckets per key, at most
HV_BCAP = 512             # ... members one wave sorts; a fuller bucket sends the key to the radix sort
RB = 9                    # wg_radix_sort_u32: bits per round
OVF_BLOCK_GROUP = 1024    # k_overflow: groups above this size take group_block
SMALLC = 8                # ... groups up to this size take group_thread
OVF_INLINE_CAP = 32       # ... inline chains per entry
OVF_HEAVY = 8192          # option overflow_heavy_min's default: entries of this size take stream 2
MIRRORED = ("HEAVY_MIN", "SPLIT_MIN", "SPLIT_TAB", "SPLIT_MAXH", "SPLIT_U", "HV_FT", "HV_NBK", "HV_BCAP", "RB",
            "OVF_BLOCK_GROUP", "SMALLC", "CAP", "OVF_INLINE_CAP")
BLOCK_RUNS = 2 * CAP      # group_block's run-head capacity (its caller passes 2 * CAP)
NF = 6
NF_WIDE_TABLE = 4200      # the k_overflow build: more functions than group_block has run heads


SPLIT_HASH_MULT = 0x9E3779B1   # split_hash: (rem * this) mod 2^32, the top log2(SPLIT_TAB) = 12 bits
SPLIT_HASH_TEXT = "uint32_t split_hash(uint32_t rem) { return (rem * 0x9E3779B1u) >> (32 - 12); }"


def source_text():
    """The text of skm_build.hip."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "signature_kmers_amd", "csrc",
                           "skm_build.hip")) as f:
        return f.read()


def split_home(geom, h):
    """k_ovf_split's split_hash of a key's rem: its home slot in the SPLIT_TAB key table (restated
    here on its own, not through process_sub's table hash, so that neither can move unnoticed)."""
    rem = geom.rem_of(h) & np.uint64(0x7FFFFFFF)
    return ((rem * np.uint64(SPLIT_HASH_MULT)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - 12)


def probe_crossings(homes):
    """Linear probing of the keys into the SPLIT_TAB table: how many of them end beyond slot
    SPLIT_TAB - 1, wrapped to the table's start (the same count whatever the order of insertion)."""
    assert len(homes) <= SPLIT_TAB
    used, wrapped = set(), 0
    for h in sorted(int(x) for x in homes):
        s = h
        while s & (SPLIT_TAB - 1) in used:
            s += 1
        used.add(s & (SPLIT_TAB - 1))
        wrapped += s >= SPLIT_TAB
    return wrapped


def source_constants():
    """Every `constexpr int|uint32_t NAME = expression` of skm_build.hip that evaluates to an integer."""
    env = {}
    for decl in re.findall(r"constexpr\s+(?:int|uint32_t)\s+([^;]+);", source_text()):
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


# ---------------------------------------------------------------------------------------------
# sequence indices
# ---------------------------------------------------------------------------------------------
class Indexer:
    """Hands out sequence indices of a build of n_total sequences: exact ones, or free ones of a
    range.  The indices below `low` are given out by exact() only."""

    def __init__(self, n_total, seed, low=1024):
        self.n = n_total
        self.free = np.ones(n_total, bool)
        self.held = np.zeros(n_total, bool)
        self.held[:low] = True
        self.rng = np.random.default_rng(seed)

    def hold(self, i):
        self.held[i] = True

    def exact(self, i):
        assert self.free[i], i
        self.free[i] = False
        return int(i)

    def inside(self, lo, hi, k):
        cand = np.nonzero(self.free[lo:hi] & ~self.held[lo:hi])[0] + lo
        assert len(cand) >= k, (lo, hi, k, len(cand))
        pick = np.sort(self.rng.choice(cand, k, replace=False))
        self.free[pick] = False
        return [int(i) for i in pick]

    def bucket(self, bk, nbk):
        """[lo, hi): the sequence indices s with s * nbk // n_total == bk."""
        return -(-bk * self.n // nbk), -(-(bk + 1) * self.n // nbk)


def nbk_of(n):
    nbk = 1
    while nbk < HV_NBK and nbk * 256 < n:
        nbk <<= 1
    return nbk


def M(fn, at=None, lead=None, trail=None, reps=1):
    """One protein of a key: function, planned sequence index, leading / trailing X, occurrences."""
    return (fn, at, lead, trail, reps)


# ---------------------------------------------------------------------------------------------
# scenarios
# ---------------------------------------------------------------------------------------------
class HScenario(Scenario):
    """One level-1 bucket whose keys all lie in one deepest (11-bit) sub-bucket.

    plan[k]: the planned sequence index of protein k (None: any); index[k]: where assemble_planned
    put it.  edges: the edges the scenario is there for (the printed table).  claims: what model()
    must say, {key name: {field: value}} and {"entry": {...}} under the option sets named in
    `under`.  best / avg / mean: hand-written expectations per k-mer."""

    def __init__(self, name, geom, prefix, seed, nf=NF, sub11=0x2D5):
        super().__init__(name, geom, prefix, seed, nf, total=0)
        self.deep = (11, sub11)
        self.plan, self.index = [], None
        self.edges, self.claims, self.names = [], {}, {}
        self.best, self.avg, self.mean = {}, {}, {}

    def _protein(self, kmer, fn, long=False, twice=False):
        super()._protein(kmer, fn, long, twice)
        self.plan.append(None)

    def key(self, name, members, kept, best=None, avg=None, mean=None, where=None):
        """One k-mer; members: M(...) proteins.  kept / best / avg / mean: written by the caller."""
        kmer = kmer_of(self.take(1, self.deep, where)[0])
        funcs = []
        for fn, at, lead, trail, reps in members:
            lead = int(self.rng.integers(0, 60)) if lead is None else lead
            trail = int(self.rng.integers(0, 60)) if trail is None else trail
            self.seqs.append(b"X" * lead + (kmer + b"X") * (reps - 1) + kmer + b"X" * trail)
            self.funcs.append(fn)
            self.plan.append(at)
            funcs += [fn] * reps
        assert kmer not in self.expect and name not in self.names
        self.expect[kmer] = kept
        self.groups.append((kmer, funcs))
        self.names[name] = kmer
        if best is not None:
            self.best[kmer] = best
        if avg is not None:
            self.avg[kmer] = avg
        if mean is not None:
            self.mean[kmer] = mean
        return kmer

    def light(self, n, where=None):
        """n singleton keys (always kept): the light remainder."""
        self.singletons(n, sub=self.deep, where=where)

    def done(self, *edges, **claims):
        self.total = self.n_elements()
        assert self.total > CAP, (self.name, self.total)
        self.b2 = b2_of(self.total)
        sizes = [0] * (1 << self.b2)
        sizes[self.deep[1] >> (11 - self.b2)] = self.total
        self.sub_sizes = tuple(sizes)
        self.overflow_subbuckets, self.overflow_elements = 1, self.total
        self.under = claims.pop("under", {})  # the option set the claims are made under
        self.edges += list(edges)
        self.claims.update(claims)
        return self


def assemble_planned(scenarios, n_total=None, seed=0, filler=b"X"):
    """The build's input of n_total sequences: every protein with a planned index at that index, the
    others shuffled over the free indices by a fixed seed, the rest one-residue fillers (no window,
    function 0).  Sets every scenario's `index`."""
    prots = [(sc, k) for sc in scenarios for k in range(len(sc.seqs))]
    n_total = len(prots) if n_total is None else n_total
    assert len(prots) <= n_total, (len(prots), n_total)
    seqs = [None] * n_total
    funcs = np.zeros(n_total, np.uint16)
    for sc in scenarios:
        sc.index = np.full(len(sc.seqs), -1, np.int64)
    rest = []
    for sc, k in prots:
        at = sc.plan[k]
        if at is None:
            rest.append((sc, k))
        else:
            assert seqs[at] is None, (sc.name, at)
            seqs[at], funcs[at], sc.index[k] = sc.seqs[k], sc.funcs[k], at
    free = np.array([i for i in range(n_total) if seqs[i] is None], np.int64)
    spots = np.random.default_rng(seed).permutation(free)[:len(rest)]
    for (sc, k), at in zip(rest, spots):
        seqs[at], funcs[at], sc.index[k] = sc.seqs[k], sc.funcs[k], at
    for i in range(n_total):
        if seqs[i] is None:
            seqs[i] = filler
    res, off, lens = pack(seqs)
    return res, off, lens, funcs, np.arange(n_total, dtype=np.uint32)


_members = {}


def members_of(sc):
    """Every valid window of the scenario's proteins, from the residues: k-mer (u64), function,
    sequence index, offset from the end (len - i, before the builder's mod 2^16), protein length."""
    if id(sc) not in _members:
        km, fn, sq, of, ln = [], [], [], [], []
        for seq, f, s in zip(sc.seqs, sc.funcs, sc.index):
            w = windows_of(seq)
            raw = np.lib.stride_tricks.sliding_window_view(np.frombuffer(seq, np.uint8), 8)[w]
            km.append(np.ascontiguousarray(raw).view("<u8").ravel())
            fn.append(np.full(len(w), f, np.int64))
            sq.append(np.full(len(w), s, np.int64))
            of.append(len(seq) - w)
            ln.append(np.full(len(w), len(seq), np.int64))
        _members[id(sc)] = (np.concatenate(km).astype(np.uint64), np.concatenate(fn), np.concatenate(sq),
                            np.concatenate(of).astype(np.int64), np.concatenate(ln), sc)
    return _members[id(sc)][:5]


# ---------------------------------------------------------------------------------------------
# the model of the kernels' decisions
# ---------------------------------------------------------------------------------------------
def bucket_class(c):
    """heavy_bucket_out<E>: the items per lane of a bucket of c members."""
    return 1 if c <= 64 else 2 if c <= 128 else 4 if c <= 256 else 8


def radix_rounds(smax):
    bits = 0
    while bits < 32 and (smax >> bits):
        bits += RB
    return bits // RB


def kept_rule(best, n):
    return 5 * best >= 4 * n


def key_stats(fn):
    cnt = np.bincount(fn)
    f = int(np.argmax(cnt))  # the lowest function of the largest count
    return f, int(cnt[f])


def heavy_key_model(fn, sq, n_total, fast, giant_min):
    """k_heavy on one key: its members' functions and sequence indices."""
    n = len(fn)
    f, cb = key_stats(fn)
    k = dict(n=n, best_f=f, cb=cb, kept=kept_rule(cb, n), path="heavy")
    best = fn == f
    k["smax"] = int(sq[best].max())
    k["rounds"] = radix_rounds(k["smax"])
    k["bucketed"] = False
    if fast:
        nbk = nbk_of(n)
        bk = sq * nbk // n_total
        k["nbk"] = nbk
        k["members"] = np.bincount(bk, minlength=nbk)
        k["bests"] = np.bincount(bk[best], minlength=nbk)
        k["fullest"] = int(k["members"].max())
        k["bucketed"] = k["fullest"] <= HV_BCAP
        # (members, best members) of the buckets a wave sorts: those with a best member
        k["sorted_buckets"] = sorted((int(c), int(b)) for c, b in zip(k["members"], k["bests"]) if b)
        k["classes"] = sorted(set(bucket_class(c) for c, _ in k["sorted_buckets"]))
    k["giant"] = bool(k["kept"] and giant_min and cb >= giant_min)
    k["job"] = bool(k["kept"] and not k["giant"])
    return k


def overflow_model(km, fn, inline_min):
    """k_overflow on one entry (the elements it is handed)."""
    n = len(km)
    N = CAP
    while N < n:
        N <<= 1
    nch = (n + CAP - 1) // CAP * CAP
    o = dict(n=n, N=N, nch=nch, pad_chunks=(N - nch) // CAP, keys={})
    sizes, chains, runs = [], [], {}
    for key in np.unique(km):
        f = fn[km == key]
        c = len(f)
        bf, cb = key_stats(f)
        cls = "thread" if c <= SMALLC else "wave" if c <= OVF_BLOCK_GROUP else "block"
        r = len(np.unique(f))
        if cls == "block" and r > BLOCK_RUNS:
            cls = "block_fallback"
        kept = kept_rule(cb, c)
        o["keys"][int(key)] = dict(n=c, best_f=bf, cb=cb, kept=kept, path="overflow", group=cls, runs=r,
                                   job=kept and cb >= 3, giant=False)
        sizes.append(c)
        if kept and cb >= 3:
            chains.append(cb)
    o["sizes"] = sorted(sizes)
    o["chains"] = sorted(chains)
    o["groups"] = len(sizes)
    o["inline"] = min(OVF_INLINE_CAP, sum(1 for c in chains if c >= inline_min))
    return o


def model(sc, n_total, nf, opts, table=False):
    """What the kernels decide for one scenario (one overflow entry) under the option set.  table:
    also where k_ovf_split's key table puts the keys (home_min, home_max, probe_wrapped)."""
    km, fn, sq, of, ln = members_of(sc)
    passes = opts.get("key_range_passes", 1)
    heavy_min = max(opts.get("heavy_min", HEAVY_MIN), 2)
    split_min = max(opts.get("split_min", SPLIT_MIN), CAP + 1)
    fast = nf <= HV_FT and not opts.get("heavy_lsd", 0)
    gcls = opts.get("giant_class", 14 if passes == 1 else 0)
    giant_min = (1 << gcls) if gcls > 0 else 0
    inline_min = opts.get("overflow_inline_min", 0x7FFFFFFF)
    n = len(km)
    keys, cnt = np.unique(km, return_counts=True)
    m = dict(n=n, distinct=len(keys), split=n >= split_min, keys={})
    m["stream"] = 2 if n >= opts.get("overflow_heavy_min", OVF_HEAVY) else 3
    m["npad"] = 1 << max(0, int(n - 1).bit_length())  # k_ovf_plan: the entry's scratch, a power of two >= n
    m["pass"] = sc.prefix >> 12 if passes > 1 else 0
    m["fail"] = m["split"] and len(keys) > SPLIT_TAB
    if table and m["split"] and not m["fail"]:  # the key table's probe chains (split_hash)
        homes = split_home(sc.geom, hash_of_keys(keys))
        m["home_min"], m["home_max"] = int(homes.min()), int(homes.max())
        m["probe_wrapped"] = probe_crossings(homes)
    m["iterations"] = -(-n // (512 * SPLIT_U))
    cand = keys[cnt >= heavy_min] if m["split"] and not m["fail"] else keys[:0]
    m["candidates"] = len(cand)
    if len(cand) > SPLIT_MAXH:
        # which candidates get the SPLIT_MAXH slots is the order of an atomic: the scenario makes
        # them interchangeable in size, so the counts below hold whichever they are
        assert len(set(cnt[cnt >= heavy_min].tolist())) == 1, sc.name
        heavy_elems = SPLIT_MAXH * int(cnt[cnt >= heavy_min][0])
        m["heavy_keys"] = SPLIT_MAXH
        cand = None
    else:
        heavy_elems = int(cnt[np.isin(keys, cand)].sum())
        m["heavy_keys"] = len(cand)
    m["heavy_elements"] = heavy_elems
    m["light_elements"] = n - heavy_elems
    light = n - heavy_elems
    if light == 0:
        m["rest"] = "none"
    elif heavy_elems and light <= CAP and opts.get("ovf_light", 1):
        m["rest"] = "light"
    else:
        m["rest"] = "overflow"
    m["jobs"] = m["samples"] = m["giants"] = m["giant_max"] = m["inline"] = 0
    if cand is None:
        # every candidate is alike (asserted above): kept keys of one function
        one = fn[km == keys[cnt >= heavy_min][0]]
        bf, cb = key_stats(one)
        kept = kept_rule(cb, len(one))
        nk = int(np.count_nonzero(cnt >= heavy_min))
        m["jobs"] += nk * int(kept and cb >= 3)
        m["samples"] += SPLIT_MAXH * cb * int(kept) + (nk - SPLIT_MAXH) * cb * int(kept and m["rest"] == "overflow")
        lightsel = cnt < heavy_min
    else:
        for key in cand:
            sel = km == key
            k = heavy_key_model(fn[sel], sq[sel], n_total, fast, giant_min)
            m["keys"][int(key)] = k
            m["jobs"] += k["job"]
            m["samples"] += k["cb"] * k["job"]
            m["giants"] += k["giant"]
            m["giant_max"] = max(m["giant_max"], k["cb"] * k["giant"])
        lightsel = ~np.isin(keys, cand)
    rest = np.isin(km, keys[lightsel])
    if m["rest"] == "overflow":
        o = overflow_model(km[rest], fn[rest], inline_min)
        m["overflow"] = o
        m["keys"].update(o["keys"])
        m["inline"] = o["inline"]
        m["jobs"] += len(o["chains"]) - o["inline"]
        m["samples"] += sum(o["chains"])
    elif m["rest"] == "light":
        # k_ovf_light: the LDS group-by; its chains are jobs, their lengths stay in tmp
        for key in keys[lightsel]:
            bf, cb = key_stats(fn[km == key])
            m["jobs"] += int(kept_rule(cb, int(np.count_nonzero(km == key))) and cb >= 3)
    return m


def counters_of(scenarios, n_total, nf, opts):
    """The counters a build of these scenarios must report.  The two demands are k_ovf_plan's sums
    over a pass's entries (the largest pass): the scratch elements and the elements of the entries
    that are split.  A build given exactly the first as its work-buffer capacity (option
    work_buffer_elements) fits, so it is not redone; the automatic first guess is made for inputs
    whose overflow is a small share of the windows, which the planted ones are not."""
    ms = [model(sc, n_total, nf, opts) for sc in scenarios]
    light = [m for m in ms if m["rest"] == "light"]
    passes = sorted(set(m["pass"] for m in ms))
    return dict(demand_overflow_scratch=max(sum(m["npad"] for m in ms if m["pass"] == p) for p in passes),
                demand_split=max(sum(m["n"] for m in ms if m["pass"] == p and m["split"]) for p in passes),
                overflow_subbuckets=len(ms), overflow_elements=sum(m["n"] for m in ms),
                overflow_light_subbuckets=len(light), overflow_light_elements=sum(m["light_elements"] for m in light),
                chain_jobs=sum(m["jobs"] for m in ms), chain_samples=sum(m["samples"] for m in ms),
                giant_chains=sum(m["giants"] for m in ms), giant_max=max([m["giant_max"] for m in ms] + [0]),
                redone=0)


# ---------------------------------------------------------------------------------------------
# key builders
# ---------------------------------------------------------------------------------------------
def spread(n, nbest, f, others):
    """n single-occurrence members anywhere: nbest of function f, the minority spread evenly."""
    return [M(fn) for fn in best_mix(n, nbest, f, others)]


def bucket_key(sc, ix, name, n, cb, spec, f, others, kept=True, **kw):
    """A key of n members, cb of function f, with planned sequence buckets: spec {bucket: (members,
    best members)}; the members left over are dealt evenly over the other buckets."""
    nbk = nbk_of(n)
    members = []
    for b, (c, nb) in spec.items():
        idx = ix.inside(*ix.bucket(b, nbk), c)
        members += [M(fn, at=i) for fn, i in zip(best_mix(c, nb, f, others), idx)]
    left = n - sum(c for c, _ in spec.values())
    left_best = cb - sum(nb for _, nb in spec.values())
    other = [b for b in range(nbk) if b not in spec]
    assert (left == 0 and left_best == 0) or other
    if left:
        mix = best_mix(left, left_best, f, others)
        at = 0
        for j, b in enumerate(other):
            c = left // len(other) + (1 if j < left % len(other) else 0)
            idx = ix.inside(*ix.bucket(b, nbk), c)
            members += [M(fn, at=i) for fn, i in zip(mix[at:at + c], idx)]
            at += c
    assert len(members) == n
    return sc.key(name, members, kept, best=f if kept else None, **kw)


# ---------------------------------------------------------------------------------------------
# the main build: the split and k_heavy
# ---------------------------------------------------------------------------------------------
NT_MAIN = 150001       # sequences of the main build: odd, so no bucket boundary is a whole multiple
HEAVY16 = {"heavy_min": 16}
_built = {}


def main_build(pass_bits=0):
    """The scenarios of the split and of k_heavy, one build.  Every remainder is singletons, so
    heavy_min 16 changes nothing but the scenarios made for it; under the default heavy_min their
    16-member keys are light and their entries are k_overflow's.  pass_bits 2: the same scenarios
    planted for four key-range passes, spread over all four."""
    if ("main", pass_bits) in _built:
        return _built[("main", pass_bits)]
    geom = Geometry(pass_bits)
    ix = Indexer(NT_MAIN, 77)
    for b in range(1, 4):  # the boundary scenario's indices
        lo, _ = ix.bucket(b, 4)
        ix.hold(lo - 1)
        ix.hold(lo)
    ix.hold(NT_MAIN - 1)
    scs = []

    def new(name, nf=NF):
        k = len(scs)
        prefix = ((k % (1 << pass_bits)) << 12) | (101 + 37 * k)
        sc = HScenario(name, geom, prefix, 1000 + k, nf, sub11=(0x2D5 + 97 * k) & 0x7FF)
        scs.append(sc)
        return sc

    # ---- the split's entry sizes: nt * SPLIT_U = 4096 elements per iteration, almost all heavy;
    #      the keys' sizes are the NBK doubling points 256 * NBK | + 1 ----
    for total, rem, sizes in ((4096, 1, (1024, 1025, 2046)), (4097, 1, (1024, 1024, 1024, 1024)),
                              (8192, 1, (4096, 2049, 2046)), (8193, 1, (4097, 2048, 2047)),
                              (4096, CAP, (1024, 1024)), (4097, CAP, (1025, 1024)),
                              (8192, CAP, (2048, 2048, 2048)), (8193, CAP, (2049, 2048, 2048))):
        sc = new(f"entry_{total}_rem_{rem}")
        assert sum(sizes) + rem == total
        claims = {}
        for j, n in enumerate(sizes):
            # alternately all of one function, 90 %, exactly 80 % (or the first count above), one short
            nb = (n, 9 * n // 10, -(-4 * n // 5), -(-4 * n // 5) - 1)[(j + total) % 4]
            f = (1, 4, 0, NF - 1)[j]
            sc.key(f"k{j}_{n}", spread(n, nb, f, [(f + 1) % NF, (f + 3) % NF]), kept_rule(nb, n),
                   best=f if kept_rule(nb, n) else None)
            claims[f"k{j}_{n}"] = dict(n=n, nbk=nbk_of(n), cb=nb, bucketed=True)
        sc.light(rem)
        sc.done(f"k_ovf_split: an entry of {total} elements ({-(-total // 4096)} iteration(s) of 4096), "
                f"{len(sizes)} heavy keys and a remainder of {rem}",
                "k_heavy: NBK doubles at n = 256 * NBK | + 1 (" + ", ".join(f"{n}: {nbk_of(n)}" for n in sizes) + ")",
                entry=dict(n=total, iterations=-(-total // 4096), heavy_keys=len(sizes), light_elements=rem,
                           rest="light"), **claims)

    sc = new("all_heavy")
    for j in range(3):
        sc.key(f"k{j}", spread(1024, 1024 - 50 * j, j + 1, [0]), True, best=j + 1)
    sc.done("k_ovf_split: every key of the entry is heavy (the remainder is empty, e.n = 0)",
            entry=dict(n=3072, heavy_keys=3, light_elements=0, rest="none"))

    sc = new("rest_on_stream_2")
    sc.key("a", spread(3000, 2700, 1, [0, 2]), True, best=1)
    sc.key("b", spread(3000, 2400, NF - 1, [0]), True, best=NF - 1)
    sc.light(2500)
    sc.done("k_overflow: a light remainder beyond CAP of an entry of overflow_heavy_min or more (the first launch, "
            "stream 2; distinct_4096's goes through the second, stream 3)",
            entry=dict(n=8500, stream=2, heavy_keys=2, light_elements=2500, rest="overflow"))

    # ---- the key table ----
    for singles in (SPLIT_TAB - 1, SPLIT_TAB):
        sc = new(f"distinct_{singles + 1}", nf=NF)
        sc.key("big", spread(1100, 900, 2, [0, 5]), True, best=2)
        sc.light(singles)
        if singles + 1 == SPLIT_TAB:
            sc.done("k_ovf_split: exactly SPLIT_TAB = 4096 distinct keys: the table is full, every lookup ends, "
                    "the entry is split", entry=dict(distinct=SPLIT_TAB, fail=False, heavy_keys=1, rest="overflow",
                                                     stream=3),
                    big=dict(path="heavy"))
        else:
            sc.done("k_ovf_split: 4097 distinct keys: s_fail, the entry goes to k_overflow unsplit with a key "
                    "above OVF_BLOCK_GROUP inside (group_block after s_fail)",
                    "k_overflow after s_fail: this entry alone (n = 5197, N = 8192: one 1100-member group_block key "
                    "plus singletons).  An entry reaches k_overflow in the same form whether split_min or s_fail kept "
                    "it whole, so the sizes 2049 | 4096 | 4097 | 8193, the SMALLC groups and the 64 | 65 chains run "
                    "under split_min 2^30 only (build overflow)",
                    entry=dict(distinct=SPLIT_TAB + 1, fail=True, heavy_keys=0, rest="overflow"),
                    big=dict(path="overflow", group="block"))

    # ---- heavy_min 16: SPLIT_MAXH and the wrapping probe chains ----
    for nk in (SPLIT_MAXH, SPLIT_MAXH + 1):
        sc = new(f"maxh_{nk}")
        for j in range(nk):
            sc.key(f"k{j}", [M(3, lead=10, trail=20)] * 16, True, best=3, avg=28, mean=38)
        sc.light(100)
        sc.done(f"k_ovf_split (heavy_min 16): {nk} keys of 16 members: " +
                ("all heavy" if nk == SPLIT_MAXH else "the 257th stays light (SPLIT_MAXH)"),
                under=HEAVY16, entry=dict(candidates=nk, heavy_keys=SPLIT_MAXH, light_elements=100 + 16 * (nk - 256),
                                          rest="light"))
    sc = new("probe_wrap")
    wrap = lambda h: split_home(geom, h) >= np.uint64(4000)  # noqa: E731
    for j in range(100):
        sc.key(f"k{j}", spread(16, 16 if j % 3 else 13, j % NF, [(j + 1) % NF]), True, best=j % NF, where=wrap)
    for j in range(540):
        sc.key(f"p{j}", spread(2, 2, j % NF, []), True, where=wrap)
    sc.done("k_ovf_split (heavy_min 16): 640 keys whose split_hash homes are 4000..4095, so the probe chains "
            "wrap past slot 4095; 100 of them heavy", under=HEAVY16,
            entry=dict(distinct=640, heavy_keys=100, light_elements=1080, rest="light"))

    # ---- k_heavy, the bucketed sample order ----
    sc = new("fullest_bucket")
    bucket_key(sc, ix, "full_512", 1024, 900, {0: (512, 480), 1: (256, 256), 2: (192, 100), 3: (64, 64)}, 1, [0, 2])
    bucket_key(sc, ix, "full_513", 1025, 950, {5: (513, 500)}, 4, [3])
    sc.light(200)
    sc.done("k_heavy: bucketed = bm <= HV_BCAP: the fullest sequence bucket holds 512 (bucketed) | 513 (sorted path: "
            "a crowded bucket)", "heavy_bucket_out<8> at 512 members with nb < c",
            full_512=dict(nbk=4, fullest=512, bucketed=True, classes=[1, 4, 8]),
            full_513=dict(nbk=8, fullest=513, bucketed=False))

    sc = new("bucket_classes_a")
    spec, b = {}, 0
    for c in (64, 65, 128, 129):
        for nb in (1, c - 1, c):
            spec[b] = (c, nb)
            b += 1
    spec[12] = (40, 0)     # members, none of them best
    spec[13] = (0, 0)      # no member at all
    cb = 4097 - (63 + 64 + 127 + 128 + 4 + 40)
    bucket_key(sc, ix, "classes", 4097, cb, spec, 2, [5, 0])
    sc.light(300)
    want = sorted((c, nb) for c, nb in spec.values() if nb)
    sc.done("heavy_bucket_out<1|2|4>: buckets of 64 | 65, 128 | 129 members with 1, c - 1 and c best members",
            "k_heavy: a bucket with members and no best member, and an empty bucket",
            classes=dict(nbk=32, bucketed=True, cb=cb, has_buckets=want, empty_best=2))

    sc = new("bucket_classes_b")
    spec, b = {}, 0
    for c in (256, 257):
        for nb in (1, c - 1, c):
            spec[b] = (c, nb)
            b += 1
    spec[6] = (512, 300)
    spec[31] = (512, 512)
    cb = 4097 - (255 + 256 + 2 + 212)
    bucket_key(sc, ix, "classes", 4097, cb, spec, 0, [NF - 1])
    sc.light(300)
    want = sorted((c, nb) for c, nb in spec.values() if nb)
    sc.done("heavy_bucket_out<4|8>: buckets of 256 | 257 members with 1, c - 1 and c best members, and of 512 with "
            "300 and with 512", classes=dict(nbk=32, bucketed=True, cb=cb, has_buckets=want, classes=[1, 4, 8]))

    sc = new("best_at_the_ends")
    # one bucket holds at most HV_BCAP = 512 members and a kept key of >= 1024 has >= 820 best
    # members, so "all in the last bucket" is the last two (and the first two)
    bucket_key(sc, ix, "last", 1100, 900, {7: (450, 450), 6: (450, 450), 0: (100, 0), 3: (100, 0)}, 3, [1])
    bucket_key(sc, ix, "first", 1100, 900, {0: (450, 450), 1: (450, 450), 7: (100, 0), 4: (100, 0)}, 5, [2])
    sc.light(250)
    sc.done("k_heavy: the reversed best-count scan: every best member in the last two buckets | in the first two "
            "(HV_BCAP keeps 80 % of >= 1024 members out of one bucket)", "buckets with no best member",
            last=dict(nbk=8, bucketed=True, best_buckets=[6, 7]), first=dict(nbk=8, bucketed=True, best_buckets=[0, 1]))

    sc = new("bucket_boundary")
    members = []
    for b in range(4):
        lo, hi = ix.bucket(b, 4)
        # (index 0 is no boundary between two buckets: it belongs to radix_rounds' seq_0)
        members += [M(1, at=ix.exact(lo) if b else ix.inside(lo, hi, 1)[0]), M(1, at=ix.exact(hi - 1))]
        members += [M(fn, at=i) for fn, i in zip(best_mix(254, 230, 1, [0]), ix.inside(lo, hi, 254))]
    sc.key("edges", members, True, best=1)
    sc.light(1100)
    sc.done("k_heavy: the bucket index s * NBK / n_total at the last index of every bucket and the first of the next "
            "(n_total = 150001: no boundary is a whole number)",
            edges=dict(nbk=4, bucketed=True, members=[256] * 4, at_boundaries=True))

    sc = new("one_protein_many")
    sc.key("host_600", [M(2, reps=600, at=ix.inside(40000, 50000, 1)[0])] + spread(500, 420, 2, [1]), True, best=2)
    sc.key("host_100", [M(4, reps=100, at=ix.inside(90000, 99000, 1)[0])] + spread(1000, 900, 4, [0, 1]), True, best=4)
    sc.light(150)
    sc.done("k_heavy: one protein hosting the key 600 times (equal items; its bucket is crowded: the sorted path) | "
            "100 times (equal (s + 1, len) items in one wave's sort)",
            host_600=dict(bucketed=False, n=1100), host_100=dict(bucketed=True, n=1100))

    # ---- the two-level upper median, the u16 length sum, the mean ----
    sc = new("median_bins")
    sc.key("hi_edge", [M(2, lead=5, trail=j % 200) for j in range(512)] +
           [M(2, lead=3, trail=592 + j % 50) for j in range(512)], True, best=2, avg=600, mean=44)
    sc.key("lo_edge", [M(3, lead=0, trail=248 + j % 100) for j in range(512)] +
           [M(3, lead=0, trail=398 + j % 20) for j in range(512)], True, best=3, avg=406, mean=39)
    sc.light(100)
    sc.done("k_heavy median: n / 2 lands exactly on the cumulative count of a high-byte bin (an empty bin follows) | "
            "of a low-byte bin (50 empty bins follow)", hi_edge=dict(n=1024, median_on_edge="high"),
            lo_edge=dict(n=1024, median_on_edge="low"))

    sc = new("offset_bytes")
    # 19 proteins hosting the key 28 times, 65535 residues: offsets 65535 - 9 j (high byte 255)
    sc.key("byte_255", [M(4, lead=0, trail=j % 100) for j in range(500)] +
           [M(4, lead=0, trail=65284, reps=28) for _ in range(19)], True, best=4, avg=65292, mean=27)
    # ... 65788 residues: offsets 65788 - 9 j = 2^16 + 252 .. 2^16 + 9, which wrap below the others
    sc.key("wrapped", [M(5, lead=0, trail=992 + j % 100) for j in range(500)] +
           [M(5, lead=0, trail=65537, reps=28) for _ in range(19)], True, best=5, avg=252, mean=3)
    sc.light(100)
    sc.done("k_heavy median: high bytes 0 and 255 (the median in bin 255)",
            "offsets (len - i) mod 2^16 that wrap (the median is a wrapped one); proteins above 65535 in the mean",
            byte_255=dict(n=1032, high_bytes=[0, 255]), wrapped=dict(n=1032, wraps=532))

    sc = new("length_sum")
    sc.key("sum_65535", [M(1, lead=20, trail=36)] * 1023 + [M(1, lead=20, trail=35)], True, best=1, avg=44, mean=63)
    sc.key("sum_65536", [M(1, lead=20, trail=36)] * 1024, True, best=1, avg=44, mean=0)
    sc.key("sum_long", [M(2, lead=40000, trail=30000)] + spread(1050, 850, 2, [0, 3]), True, best=2)
    sc.light(120)
    sc.done("k_heavy: the u16 length sum at exactly 65535 (mean 63) | 65536 (wraps to 0: mean 0)",
            "a best member of more than 65535 residues; the mean's d2u16",
            sum_65535=dict(length_sum=65535), sum_65536=dict(length_sum=65536))

    # ---- the best function ----
    sc = new("best_function")
    sc.key("tie", spread(1024, 512, 0, [NF - 1]), False)
    sc.key("exact_80", spread(1025, 820, NF - 1, [0]), True, best=NF - 1)
    sc.key("short_80", spread(1025, 819, NF - 1, [0]), False)
    # k_ovf_split's scatter orders the members by an atomic cursor, so which member leads a wave is
    # not ours to choose: the minority 20 % is spread evenly over the sequence
    sc.key("minority", spread(1280, 1024, 3, [0]), True, best=3)
    sc.light(90)
    sc.done("k_heavy: a tie between function 0 and nf - 1 (cut)", "exactly 80 % | one short (fast path and "
            "Boyer-Moore across waves under heavy_lsd)", "a 20 % minority of a lower function spread evenly (the "
            "scatter's order is an atomic's: lane 0's function cannot be planted)",
            tie=dict(kept=False, cb=512), exact_80=dict(kept=True, cb=820), short_80=dict(kept=False, cb=819))

    # ---- the sorted path's radix rounds ----
    sc = new("radix_rounds")
    sc.key("seq_0", [M(1, reps=1100, at=ix.exact(0))], True, best=1)
    sc.key("smax_511", [M(2, reps=4, at=ix.exact(i)) for i in range(1, 512, 2)] + spread(76, 0, 2, [0]), True, best=2)
    sc.key("smax_512", [M(3, reps=4, at=ix.exact(i)) for i in range(2, 513, 2)] + spread(77, 0, 3, [1]), True, best=3)
    sc.light(50)
    sc.done("k_heavy sorted path: bits = 0 (every best member in sequence 0: no radix round, the result is sa)",
            "one | two radix rounds: the largest best-member index 511 | 512 (the result in sb | sa)",
            "cb = 1024 | 1100: cb a multiple of 512 and not",
            seq_0=dict(smax=0, rounds=0, bucketed=False), smax_511=dict(smax=511, rounds=1, bucketed=False, cb=1024),
            smax_512=dict(smax=512, rounds=2, bucketed=False, cb=1024))

    # ---- giant chains (giant_class 10) ----
    sc = new("giant_edge")
    sc.key("cb_1023", spread(1100, 1023, 2, [1]), True, best=2)
    sc.key("cb_1024", spread(1100, 1024, 4, [1]), True, best=4)
    sc.light(60)
    sc.done("giant chains (giant_class 10): cb = 2^10 - 1 (a job) | 2^10 (a giant chain)", under={"giant_class": 10},
            cb_1023=dict(cb=1023, giant=False), cb_1024=dict(cb=1024, giant=True))

    arrays = assemble_planned(scs, NT_MAIN, seed=5)
    _built[("main", pass_bits)] = (scs, arrays, NT_MAIN)
    return _built[("main", pass_bits)]


MAIN_OPTS = {
    "default": {},
    "heavy_min_16": dict(HEAVY16),
    "heavy_lsd": {"heavy_lsd": 1},
    "heavy_lsd_16": {"heavy_lsd": 1, "heavy_min": 16},
    "ovf_light_0": {"ovf_light": 0, "heavy_min": 16},
    "giant_10": {"giant_class": 10},
    "unsplit": {"split_min": 1 << 30},
}
PASS4_OPTS = {
    "passes_4": {"key_range_passes": 4},
    "passes_4_16": {"key_range_passes": 4, "heavy_min": 16},
    "passes_4_ovf_light_0": {"key_range_passes": 4, "ovf_light": 0, "heavy_min": 16},
}


# ---------------------------------------------------------------------------------------------
# the k_overflow build: nothing split (split_min 2^30)
# ---------------------------------------------------------------------------------------------
UNSPLIT = {"split_min": 1 << 30}
OVF_OPTS = {"unsplit": dict(UNSPLIT), "unsplit_inline_16": dict(UNSPLIT, overflow_inline_min=16), "default": {}}


def overflow_build():
    if "ovf" in _built:
        return _built["ovf"]
    geom = Geometry()
    scs = []
    nf = NF_WIDE_TABLE

    def new(name):
        k = len(scs)
        sc = HScenario(name, geom, 211 + 53 * k, 2000 + k, nf, sub11=(0x133 + 71 * k) & 0x7FF)
        scs.append(sc)
        return sc

    def fill(sc, total):
        sc.light(total - sc.n_elements())

    sc = new("n_2049")
    sc.key("g8", spread(8, 7, 1, [2]), True, best=1)
    sc.key("g9", spread(9, 8, 2, [0]), True, best=2)
    sc.key("g8_cut", spread(8, 6, 1, [2]), False)
    sc.key("g9_cut", spread(9, 7, 4199, [0]), False)
    sc.key("chain_64", spread(64, 64, 3, []), True, best=3)
    sc.key("chain_65", spread(65, 65, 4, []), True, best=4)
    sc.key("chain_64_of_80", spread(80, 64, 4199, [0]), True, best=4199)
    fill(sc, 2049)
    sc.done("k_overflow: n = 2049 (N = 4096, no padding chunk)", "groups of SMALLC 8 | 9 (group_thread | group_wave)",
            "chains of 64 | 65 samples (lengths written per thread | by the workgroup)", under=UNSPLIT,
            entry=dict(n=2049, rest="overflow"), overflow=dict(N=4096, nch=4096, pad_chunks=0),
            g8=dict(group="thread"), g9=dict(group="wave"), chain_64=dict(cb=64), chain_65=dict(cb=65))

    sc = new("n_4096")
    sc.key("g1024", spread(1024, 900, 5, [1, 0]), True, best=5)
    sc.key("g1025", spread(1025, 900, 7, [1, 4199]), True, best=7)
    fill(sc, 4096)
    sc.done("k_overflow: n = 4096 (N = nch = 4096)", "groups of OVF_BLOCK_GROUP 1024 | 1025 (group_wave | group_block)",
            under=UNSPLIT, entry=dict(n=4096), overflow=dict(N=4096, nch=4096, pad_chunks=0),
            g1024=dict(group="wave"), g1025=dict(group="block", runs=3))

    sc = new("n_4097")
    sc.key("g1025_cut", spread(1025, 819, 0, [4199]), False)
    sc.key("g1500", spread(1500, 1200, 4199, [0, 17]), True, best=4199)
    fill(sc, 4097)
    sc.done("k_overflow: n = 4097 (N = 8192, nch = 6144: one all-padding chunk)", under=UNSPLIT,
            entry=dict(n=4097), overflow=dict(N=8192, nch=6144, pad_chunks=1))

    sc = new("n_8193")
    sc.key("g3000", spread(3000, 2400, 9, [8, 10]), True, best=9)
    sc.key("g2000_tie", spread(2000, 1000, 0, [4199]), False)
    fill(sc, 8193)
    sc.done("k_overflow: n = 8193 (N = 16384, nch = 10240: three all-padding chunks; stream 2)", under=UNSPLIT,
            entry=dict(n=8193, stream=2), overflow=dict(N=16384, nch=10240, pad_chunks=3))

    # group_block's run heads: 2 * CAP = 4096 fit.  The group is one run of the best function plus
    # singleton-function runs; each is kept at >= 80 %
    for singles, big in ((4095, 16400), (4096, 16400), (4097, 16404)):
        sc = new(f"runs_{singles + 1}")
        assert kept_rule(big, big + singles)
        funcs = [100] * big + [f for f in range(4200) if f != 100][:singles]
        sc.rng.shuffle(funcs)
        sc.key("runs", [M(int(f)) for f in funcs], True, best=100)
        sc.light(30)
        sc.done(f"group_block: a kept group of {singles + 1} function runs (" +
                ("the run heads just fit" if singles + 1 <= BLOCK_RUNS else
                 "more than 2 * CAP: returns false, group_wave on the first wave") + ")", under=UNSPLIT,
                runs=dict(runs=singles + 1, group="block" if singles + 1 <= BLOCK_RUNS else "block_fallback",
                          kept=True, cb=big))

    sc = new("chains_520")
    for j in range(520):
        sc.key(f"c{j}", spread(65, 65, j % nf, []), True, best=j % nf)
    # no other group: the first round of 512 groups is 512 long chains whatever the key order
    sc.done("k_overflow: 520 groups with 65-sample chains in one entry (two emit rounds, the first with 512 long "
            "chains: every slot of s_big)", "overflow_inline_min 16: 32 of the chains run inline, the rest are jobs",
            under=UNSPLIT, entry=dict(n=520 * 65), overflow=dict(groups=520, chains=[65] * 520))
    arrays = assemble_planned(scs, None, seed=6)
    _built["ovf"] = (scs, arrays, len(arrays[2]))
    return _built["ovf"]


# ---------------------------------------------------------------------------------------------
# the wide build: three radix rounds need a best member at sequence index 2^18
# ---------------------------------------------------------------------------------------------
NT_WIDE = (1 << 18) + 1
WIDE_OPTS = {"heavy_lsd": {"heavy_lsd": 1}, "default": {}}


def wide_build():
    if "wide" in _built:
        return _built["wide"]
    ix = Indexer(NT_WIDE, 78, low=0)
    sc = HScenario("radix_wide", Geometry(), 1500, 3000)
    for name, top, f in (("smax_2p18_m1", (1 << 18) - 1, 1), ("smax_2p18", 1 << 18, 2)):
        ix.exact(top)
        idx = ix.inside(0, (1 << 18) - 1, 1099)
        funcs = best_mix(1099, 999, f, [0, 5])
        sc.key(name, [M(f, at=top)] + [M(fn, at=i) for fn, i in zip(funcs, idx)], True, best=f)
    sc.light(100)
    sc.done("k_heavy sorted path: two | three radix rounds: the largest best-member index 2^18 - 1 | 2^18 (the "
            "result in sa | sb); cb = 1000, no multiple of 512", under={"heavy_lsd": 1},
            smax_2p18_m1=dict(smax=(1 << 18) - 1, rounds=2, cb=1000), smax_2p18=dict(smax=1 << 18, rounds=3, cb=1000))
    arrays = assemble_planned([sc], NT_WIDE, seed=7)
    _built["wide"] = ([sc], arrays, NT_WIDE)
    return _built["wide"]


# ---------------------------------------------------------------------------------------------
# the plan build: more than 1024 overflow entries
# ---------------------------------------------------------------------------------------------
PLAN_SPLIT = CAP + 21
PLAN_OPTS = {"split_min_mid": {"split_min": PLAN_SPLIT}, "default": {}, "unsplit": dict(UNSPLIT)}
PLAN_SMALL = 1030


def plan_build():
    """1030 entries of CAP + 1 .. CAP + 40 elements beside entries of 4095 | 4096 | 4097 and 8191 |
    8192 | 8193.  An entry is one key in two proteins (the key repeated), kept: a wrong bin, npad or
    scratch offset of k_ovf_plan makes two entries share scratch or drops one."""
    if "plan" in _built:
        return _built["plan"]
    geom = Geometry()
    scs = []
    sizes = [CAP + 1 + j % 40 for j in range(PLAN_SMALL)] + [4095, 4096, 4097, 8191, 8192, 8193]
    for k, n in enumerate(sizes):
        sc = HScenario(f"entry_{k}_{n}", geom, 2 + 3 * k, 4000 + k, sub11=(0x077 + 13 * k) & 0x7FF)
        f = k % NF
        sc.key("only", [M(f, reps=n // 2), M(f, reps=n - n // 2)], True, best=f)
        sc.done(entry=dict(n=n))
        scs.append(sc)
    scs[0].edges = ["k_ovf_plan: 1036 entries (a thread of the scratch-offset scan owns two), sizes CAP + 1 .. CAP + 40 "
                    "on both sides of split_min CAP + 21",
                    "k_ovf_plan: entries of 4095 | 4096 | 4097 and 8191 | 8192 | 8193: both sides of a power of two "
                    "(bins, npad, scratch offsets) and of overflow_heavy_min 8192 (stream 3 | stream 2: PLAN_NHEAVY)",
                    "k_overflow with nothing split (split_min 2^30): both launches take entries"]
    arrays = assemble_planned(scs, None, seed=8)
    _built["plan"] = (scs, arrays, len(arrays[2]))
    return _built["plan"]


BUILDS = {
    "main": (main_build, MAIN_OPTS),
    "main_passes4": (lambda: main_build(2), PASS4_OPTS),
    "overflow": (overflow_build, OVF_OPTS),
    "wide": (wide_build, WIDE_OPTS),
    "plan": (plan_build, PLAN_OPTS),
}
