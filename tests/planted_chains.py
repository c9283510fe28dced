"""Planted inputs for the deferred statistics scheduler -- a plain helper module of the tests:
k_job_count / k_job_scan / k_job_scatter (the class sort), k_chains (one lane per chain),
k_long_plan / k_long_stash / k_long_snap (the run arena of key-range passes), flush_long_chains (the
lane | wave-pair split of a batch) and k_giant_order / k_chain_dyn (skm_build.hip).

It builds on planted.py and planted_heavy.py.  One occurrence is one protein, X*lead + 8-mer +
X*trail, so a key's chain length (the members of its best function) and its samples (their protein
lengths, in reverse sequence order) are chosen exactly; a key is planted in a chosen key-range pass
and level-1 bucket, and the kind of bucket chooses where the group-by leaves its samples:

  recs   a bucket of at most CAP elements (the direct path),
  tmp    a bucket above CAP whose level-2 sub-buckets hold at most CAP each (k_partition),
  big    a group of more than 64 members (k_big_groups),
  lens   a sub-bucket above CAP (its keys share the top 11 bits of rem): k_overflow's, or with
         heavy_min 64 k_heavy's, whose chains of >= 2^giant_class samples are the giant ones.

The group-by writes a deferred record with median = var = 0 and the order of a job list is an
atomic's, so every planted chain has a nonzero u16 median and a nonzero u16 variance, and no two
chains of one pass have the same (median, var): a chain that no kernel ran, or one that ran on a
neighbour's samples, differs from its expectation whatever the order was.  The lengths are drawn
after the input's sequence order is fixed, until both hold.

facts() recounts everything from the input arrays alone (windows, hashes, buckets, sub-buckets,
groups, visit order); expected() runs pyref's recurrences over every chain's samples; model()
restates the scheduler's decisions for an option set with the constants mirrored below
(check_source() asserts them against the source text).

Not reachable through the options: k_long_plan's "the samples fit but the job slots do not" branch.
long_jobs_cap is at least 4096 + valid windows >> class, and every long job has >= 2^class samples
of the pass's windows, so the job slots never run out before the samples do."""
import numpy as np

import planted_heavy as ph
import pyref
from planted import CAP, _DIGIT, Geometry, Scenario, b2_of, best_mix, hash_of_keys, kmer_of, pack

JOB_CLASSES = 32       # k_job_*: length classes, floor(log2 n)
JOB_WG = 256           # ... threads of a workgroup
JOB_NWG = 256          # ... workgroups: one contiguous chunk of the job list each
LONG_GRID = 2048       # k_long_stash / k_chain_long: workgroups, one job at a time
GORD_MAX = 4096        # k_giant_order: the first this many giant jobs are sorted
CHAIN_B = 16           # chain_run: samples per block
DEFER_MIN = 3          # a best-function run of at least this many members is deferred
BIG_MIN = 65           # groups of this many members are k_big_groups'
LONG_JOBS_MIN = 4096   # alloc_caps: the long-job list holds at least this many
TAIL_SLOT = 16         # flush_long_chains: the batch after the last pass
PLAN_WG = 1024         # k_long_plan: jobs per scan round
MIRRORED = ("JOB_CLASSES", "JOB_WG", "JOB_NWG", "LONG_GRID", "GORD_MAX")
NF = 6

SOURCE_LINES = (
    "constexpr uint32_t B = 16;",
    "if (cbest >= 3) {",
    "if (r.cbest >= 3) {",
    "__global__ __launch_bounds__(1024) void k_long_plan(",
    "const uint32_t nb = std::min<uint32_t>(P >= 2 ? std::min<uint32_t>(P, (uint32_t)std::max(1, "
    "b->tune.chain_batches)) : 1u, 16u);",
    "const uint32_t per = std::max<uint32_t>(1u, P / nb);",
    "if (nb > 1 && (pass + 1) % per == 0 && pass + 1 < P) {",
    "flush_long_chains(b, (int)((pass + 1) / per - 1));",
    "if (b->pass_bits) flush_long_chains(b, 16);",
    "const bool few = (1 << b->pass_bits) < 8;",
    "const int lmax = slot < 16 && !few ? b->tune.lane_long : std::min(b->tune.lane_long, b->tune.lane_tail);",
    "if (jb.n < min_n) continue;",
    "if (max_n && n >= max_n) continue;",
    "b->world * (b->valid_total >> cls) + 4096);",
    "for (uint32_t cc = long_class; cc < JOB_CLASSES; ++cc) nl += tot[cc];",
    "const uint32_t nj = (uint32_t)min((unsigned long long)GORD_MAX, *njobs);",
    "int main_long_class = 14;",
    "int ovf_long_class = 14;",
    "int chain_batches = 2;",
    "int lane_long = 1 << 20;",
    "int lane_tail = 1 << 16;",
)


def check_source():
    """The mirrored constants and the restated host arithmetic against the text of skm_build.hip."""
    src, text = ph.source_constants(), ph.source_text()
    for name in MIRRORED:
        assert src[name] == globals()[name], name
    for line in SOURCE_LINES:
        assert line in text, line


def ref_d2u16(xs):
    """A chain's record fields: pyref's P^2 median and running variance, truncated as d2u16 does."""
    med, var = pyref.ref_chain(xs)
    return pyref.d2u16(med), pyref.d2u16(var)


# ---------------------------------------------------------------------------------------------
# planting
# ---------------------------------------------------------------------------------------------
class ChainBuild:
    """The planted input of one build at 2^pass_bits key-range passes.  span: (largest base length,
    largest width) of a chain's drawn lengths."""

    def __init__(self, name, pass_bits, seed, span=(200, 300)):
        self.name, self.pass_bits, self.seed, self.span = name, pass_bits, seed, span
        self.geom = Geometry(pass_bits)
        self.rng = np.random.default_rng(seed)
        self.scs, self.decl, self.edges = [], [], []
        self.arrays = None

    def bucket(self, pas, name):
        """A new level-1 bucket of pass `pas`."""
        k = len(self.scs)
        assert k < 4096 and 0 <= pas < (1 << self.pass_bits)
        sc = Scenario(f"p{pas}_{name}_{k}", self.geom, (pas << 12) | ((37 + 211 * k) % 4096), self.seed * 1000 + k, NF,
                      total=0)
        sc.pas, sc.planted = pas, 0
        self.scs.append(sc)
        return sc

    def chain(self, sc, n, sub=None, other=0):
        """One key: n members of its best function and `other` of another (kept: at least 80 %)."""
        assert 5 * n >= 4 * (n + other)
        f = len(self.decl) % NF
        self.decl.append((sc, sc.take(1, sub)[0], n, other, f))
        sc.planted += n + other

    def singles(self, sc, k, sub=None):
        for code in sc.take(k, sub):
            self.decl.append((sc, code, 1, 0, int(self.rng.integers(0, NF))))
        sc.planted += k

    # -- placements ----------------------------------------------------------------------------
    def direct(self, pas, lengths, name="recs"):
        """Chains in buckets of at most CAP elements (samples from recs; above 64 members: big)."""
        sc = None
        for n in lengths:
            if sc is None or sc.planted + n > CAP:
                sc = self.bucket(pas, name)
            self.chain(sc, n)

    def partitioned(self, pas, lengths, total):
        """Chains dealt over the four level-2 sub-buckets of one bucket of `total` elements, CAP <
        total <= 3072 (b2 = 2; samples from tmp); the rest is singletons."""
        assert CAP < total <= 3072 and b2_of(total) == 2 and sum(lengths) <= total
        sc = self.bucket(pas, "tmp")
        for j, n in enumerate(lengths):
            self.chain(sc, n, sub=(2, j % 4))
        left = total - sc.planted
        for v in range(4):
            self.singles(sc, left // 4 + (1 if v < left % 4 else 0), sub=(2, v))

    def entry(self, pas, chains, singles=0, name="lens"):
        """One overflow sub-bucket: chains as (n, other); every key shares the top 11 bits of rem."""
        sc = self.bucket(pas, name)
        deep = (11, (0x2D5 + 97 * len(self.scs)) & 0x7FF)
        for n, other in chains:
            self.chain(sc, n, sub=deep, other=other)
        self.singles(sc, singles, sub=deep)
        assert sc.planted > CAP, (sc.name, sc.planted)
        return sc

    # -- the input -----------------------------------------------------------------------------
    def _draw(self, n):
        lo = int(self.rng.integers(8, self.span[0]))
        w = int(self.rng.integers(6, self.span[1]))
        return lo + self.rng.integers(0, w + 1, n)

    def finish(self, n_total=None):
        """Fix the sequence order, then draw every chain's lengths (nonzero u16 median and variance,
        a (median, var) pair of its own within the pass) and write the proteins."""
        total = sum(n + o for _, _, n, o, _ in self.decl)
        n_total = total if n_total is None else n_total
        spots = self.rng.permutation(n_total)[:total]
        seqs = [b"X"] * n_total
        funcs = np.zeros(n_total, np.uint16)
        seen = {}
        at = 0
        for sc, code, n, other, f in self.decl:
            m = n + other
            where = spots[at:at + m]
            at += m
            fl = best_mix(m, n, f, [(f + 1) % NF]) if other else [f] * m
            best = np.array([x == f for x in fl])
            length = np.zeros(m, np.int64)
            length[~best] = self.rng.integers(8, 120, m - n)
            if n >= DEFER_MIN:
                visit = np.argsort(-where[best])  # reverse sequence order
                used = seen.setdefault(sc.pas, set())
                while True:
                    xs = self._draw(n)
                    mv = ref_d2u16(xs)
                    if mv[0] and mv[1] and mv not in used:
                        break
                used.add(mv)
                tmp = np.zeros(n, np.int64)
                tmp[visit] = xs
                length[best] = tmp
            else:
                length[best] = self.rng.integers(8, 68, n)
            kmer = kmer_of(code)
            for j in range(m):
                lead = int(self.rng.integers(0, length[j] - 7))
                seqs[where[j]] = b"X" * lead + kmer + b"X" * (int(length[j]) - 8 - lead)
                funcs[where[j]] = fl[j]
        res, off, lens = pack(seqs)
        self.arrays = (res, off, lens, funcs, np.arange(n_total, dtype=np.uint32))
        return self


# ---------------------------------------------------------------------------------------------
# the recount: everything below comes from the input arrays
# ---------------------------------------------------------------------------------------------
class Facts:
    """Per key (ascending): key, pas, bucket (prefix), n members, best function, cb, kept, the entry
    it lies in (-1: none; else the entry's index in `entries`), source, and its best-function run's
    protein lengths in visit order (samples[k])."""


def facts(arrays, pass_bits, order=None, classify=True):
    """order: the sequence order the group-by sees (world > 1: rank by rank); default the input's.
    classify: also the buckets, sub-buckets and entries of the one-rank geometry."""
    res, off, lens, funcs, _ = arrays
    off = off.astype(np.int64)
    ok = _DIGIT[res] < np.uint64(40)
    run = np.zeros(len(res) + 1, np.int64)
    run[1:] = np.cumsum(ok)
    start = np.nonzero(run[8:] - run[:-8] == 8)[0]
    s = np.searchsorted(off, start, "right") - 1
    inside = start + 8 <= off[s] + lens[s].astype(np.int64)
    start, s = start[inside], s[inside]
    km = np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(res, 8)[start]).view("<u8").ravel()
    rank = s if order is None else np.argsort(order)[s]  # position in the visit order's sequence
    fn = funcs[s].astype(np.int64)
    keys, inv, cnt = np.unique(km, return_inverse=True, return_counts=True)
    nk = len(keys)
    nf = int(fn.max()) + 1
    table = np.zeros((nk, nf), np.int64)
    np.add.at(table, (inv, fn), 1)
    F = Facts()
    F.windows = len(km)
    F.keys, F.n = keys, cnt
    F.best_f = table.argmax(axis=1)  # the lowest function of the largest count
    F.cb = table.max(axis=1)
    F.kept = 5 * F.cb >= 4 * F.n
    geom = Geometry(pass_bits)
    h = hash_of_keys(keys)
    F.bucket = geom.prefix_of(h).astype(np.int64)
    F.pas = F.bucket >> 12
    # the visit order: a key's members by descending sequence position, the best function's only
    o = np.lexsort((-rank, inv))
    isbest = fn[o] == F.best_f[inv[o]]
    F.samples = np.split(lens[s[o]][isbest].astype(np.int64), np.cumsum(F.cb)[:-1])
    # buckets, level-2 sub-buckets, overflow entries
    F.source = np.full(nk, "recs", object)
    F.entry = np.full(nk, -1, np.int64)
    F.entries = []  # (pas, key indices)
    for b in np.unique(F.bucket) if classify else ():
        sel = np.nonzero(F.bucket == b)[0]
        total = int(F.n[sel].sum())
        if total <= CAP:
            continue
        b2 = b2_of(total)
        sub = geom.sub_of(h[sel], b2).astype(np.int64)
        for v in np.unique(sub):
            ks = sel[sub == v]
            if int(F.n[ks].sum()) > CAP:
                # one entry must stay one whatever the split: its keys share the top 11 bits of rem
                assert len(np.unique(geom.sub_of(h[ks], 11))) == 1
                F.entry[ks] = len(F.entries)
                F.entries.append((int(F.pas[ks[0]]), ks))
                F.source[ks] = "lens"
            else:
                F.source[ks] = "tmp"
    F.source[(F.n >= BIG_MIN) & (F.entry < 0)] = "big"
    return F


_expected = {}


def expected(F):
    """{key index: (u16 median, u16 var)} of every key with a deferred chain, from pyref."""
    if id(F) not in _expected:
        idx = np.nonzero(F.kept & (F.cb >= DEFER_MIN))[0]
        _expected[id(F)] = ({int(k): ref_d2u16(F.samples[k]) for k in idx}, F)
    return _expected[id(F)][0]


# ---------------------------------------------------------------------------------------------
# the model of the scheduler's decisions
# ---------------------------------------------------------------------------------------------
def job_class(n):
    return int(n | 1).bit_length() - 1


def batch_of_pass(P, chain_batches):
    """run_once: the snapshot slot the stashed chains of every pass leave in, and the flushes as
    (after pass, slot); the tail batch (slot 16) follows the last pass."""
    nb = min(min(P, max(1, chain_batches)) if P >= 2 else 1, 16)
    per = max(1, P // nb)
    flushes = [(p, (p + 1) // per - 1) for p in range(P) if nb > 1 and (p + 1) % per == 0 and p + 1 < P]
    slot = []
    for p in range(P):
        later = [s for after, s in flushes if after >= p]
        slot.append(later[0] if later else TAIL_SLOT)
    return slot, flushes


def lane_threshold(P, slot, opts):
    """flush_long_chains: stashed chains below this many samples run one lane each, the others on a
    wave pair (0: all on wave pairs)."""
    lane_long, lane_tail = opts.get("lane_long", 1 << 20), opts.get("lane_tail", 1 << 16)
    return max(0, lane_long if slot < TAIL_SLOT and P >= 8 else min(lane_long, lane_tail))


def chunk_sizes(nj):
    """job_chunk: the jobs of each of the JOB_NWG workgroups."""
    chunk = -(-nj // JOB_NWG)
    return [min(nj, min(nj, w * chunk) + chunk) - min(nj, w * chunk) for w in range(JOB_NWG)]


def entry_model(F, ks, opts, giant_min):
    """One overflow sub-bucket: (jobs as key indices, giants, counted samples, scratch, split)."""
    n = int(F.n[ks].sum())
    split_min = max(opts.get("split_min", ph.SPLIT_MIN), CAP + 1)
    heavy_min = max(opts.get("heavy_min", ph.HEAVY_MIN), 2)
    npad = 1 << max(0, (n - 1).bit_length())
    jobs, giants, samples = [], [], 0
    split = n >= split_min
    heavy = ks[F.n[ks] >= heavy_min] if split else ks[:0]
    assert len(ks) <= ph.SPLIT_TAB and len(heavy) <= ph.SPLIT_MAXH
    for k in heavy:  # k_heavy
        if not F.kept[k]:
            continue
        if giant_min and F.cb[k] >= giant_min:
            giants.append(int(k))
        else:
            jobs.append(int(k))
            samples += int(F.cb[k])
    light = np.setdiff1d(ks, heavy)
    nlight = int(F.n[light].sum())
    # a light remainder of at most CAP beside heavy keys is k_ovf_light's: not planted here
    assert nlight == 0 or len(heavy) == 0 or nlight > CAP or not opts.get("ovf_light", 1)
    for k in light:  # k_overflow
        if F.kept[k] and F.cb[k] >= DEFER_MIN:
            jobs.append(int(k))
            samples += int(F.cb[k])
    return jobs, giants, samples, npad, n if split else 0


def model(F, opts):
    """What the scheduler decides under the option set: per pass and chain set the jobs, the class
    histogram, nlong, the stash offsets' total, the batch and its lane threshold; the giant jobs;
    and the counters the build must report."""
    P = opts.get("key_range_passes", 1)
    long_class = {"main": opts.get("main_long_class", 14), "ovf": opts.get("overflow_long_class", 14)}
    gcls = opts.get("giant_class", 14 if P == 1 else 0)
    giant_min = (1 << gcls) if gcls > 0 else 0
    assert opts.get("overflow_inline_min", 1 << 31) > int(F.cb.max())  # no inline chains here
    slot, flushes = batch_of_pass(P, opts.get("chain_batches", 2))
    jobs = {(p, s): [] for p in range(P) for s in ("main", "ovf")}
    deferred = F.kept & (F.cb >= DEFER_MIN) & (F.entry < 0)
    for k in np.nonzero(deferred)[0]:
        jobs[(int(F.pas[k]), "main")].append(int(k))
    giants = {p: [] for p in range(P)}
    scratch, splits, counted = [0] * P, [0] * P, 0
    for p, ks in F.entries:
        j, g, smp, npad, nsplit = entry_model(F, ks, opts, giant_min)
        jobs[(p, "ovf")] += j
        giants[p] += g
        counted += smp
        scratch[p] += npad
        splits[p] += nsplit
    m = dict(P=P, slot=slot, flushes=flushes, sets={}, giants=giants, stashed={})
    total = ljobs = 0
    batches = {}
    for (p, s), ks in jobs.items():
        ns = [int(F.cb[k]) for k in ks]
        hist = [0] * JOB_CLASSES
        for n in ns:
            hist[job_class(n)] += 1
        L = long_class[s]
        long_ks = [k for k in ks if job_class(int(F.cb[k])) >= L] if P > 1 else []
        nlong_sorted = sum(hist[L:])
        stash = sum(int(F.cb[k]) for k in long_ks)
        m["sets"][(p, s)] = dict(nj=len(ks), hist=hist, nlong=nlong_sorted, stash=stash, chunks=chunk_sizes(len(ks)),
                                 lane_blocks=-(-(len(ks) - nlong_sorted) // 64),
                                 last_block=(len(ks) - nlong_sorted) % 64, rounds=-(-nlong_sorted // PLAN_WG),
                                 lengths=sorted(ns), keys=ks)
        total += stash
        ljobs += len(long_ks)
        thr = lane_threshold(P, slot[p], opts)
        for k in long_ks:
            n = int(F.cb[k])
            m["stashed"][k] = dict(slot=slot[p], threshold=thr, kernel="lane" if n < thr else "pair", n=n,
                                   source=F.source[k], set=s, pas=p)
            batches.setdefault(slot[p], []).append(k)
    m["batches"] = {s: len(batches.get(s, [])) for s in [x for _, x in flushes] + [TAIL_SLOT]} if P > 1 else {}
    allg = [int(F.cb[k]) for p in giants for k in giants[p]]
    m["arena_total"], m["long_jobs"] = total, ljobs
    m["scratch"], m["split"] = max(scratch), max(splits)
    m["counters"] = dict(chain_jobs=sum(len(v) for v in jobs.values()), chain_samples=counted, long_samples=total,
                         demand_long_samples=total, demand_long_jobs=ljobs, giant_chains=len(allg),
                         giant_max=max(allg + [0]), redone=0, passes=P)
    return m


def work_buffer(m):
    """The work_buffer_elements under which nothing is redone: the overflow scratch, the split path
    and the run arena are all sized by it."""
    return max(m["scratch"], m["split"], m["arena_total"], 1)


# ---------------------------------------------------------------------------------------------
# the builds
# ---------------------------------------------------------------------------------------------
T_LONG, T_TAIL = 40, 20   # lane_long | lane_tail of the small builds
T_EDGES = [T_TAIL - 1, T_TAIL, T_TAIL + 1, T_LONG - 1, T_LONG, T_LONG + 1]
BLOCK_EDGES = [3, 15, 16, 17, 31, 32, 33, 47, 48, 49]   # chain_run's blocks of 16
SMALL = dict(main_long_class=2, overflow_long_class=2, lane_long=T_LONG, lane_tail=T_TAIL, split_min=1 << 30,
             poison_jobs=1)
_built = {}


def cycle(values, k):
    return [values[j % len(values)] for j in range(k)]


def main_build():
    """16 passes.  Main-set jobs per pass: 0, 1, 255, 256, 257, 513, ...; long jobs (class 2: four
    samples) 0, 1, 0, ..., 1023, 1024, 1025, 2049; the four sample sources; both sets stashing in
    pass 10; the lane thresholds' edges in pass 3 (an early batch) and pass 15 (the tail batch)."""
    if "main" in _built:
        return _built["main"]
    b = ChainBuild("main", 4, 41)
    b.singles(b.bucket(0, "none"), 5)                                  # 0 jobs
    b.direct(1, [4])                                                   # 1 job, long: nlong == nj == 1
    b.direct(2, [3] * 255)                                             # 255 jobs of one class
    p3 = BLOCK_EDGES + T_EDGES + [3, 4, 5, 63, 64, 65]
    b.direct(3, p3 + cycle([3, 4, 5, 6], 256 - len(p3)))               # 256 jobs
    b.partitioned(4, cycle([3, 4, 5, 6, 21, 7], 257), 2600)            # 257 jobs, samples in tmp
    b.direct(5, cycle([3, 4, 5], 513))                                 # 513 jobs
    b.direct(6, cycle([4, 5], 1023) + [3] * 10)                        # nlong 1023
    b.direct(7, [4] * 1024)                                            # nlong 1024 == nj
    b.direct(8, cycle([4, 5, 7], 1025) + [3] * 70)                     # nlong 1025: a second scan round
    b.direct(9, [4] * 2049 + [3])                                      # nlong 2049 > LONG_GRID
    b.direct(10, [3, 5, 9, 17, 33, 64, 130, 260, 520])                 # classes 1..9 (big groups above 64)
    b.direct(10, [1030])                                               # class 10
    b.entry(10, [(2100, 0), (4100, 0), (6, 1), (12, 3), (3, 0)], singles=100)   # classes 11, 12: k_overflow
    b.entry(11, [(3000, 0)] + [(n, 0) for n in cycle(list(range(3, 16)), 63)], singles=120)
    b.direct(12, cycle(list(range(4, 31)), 40) + [2048])               # a big group of CAP members
    b.singles(b.bucket(13, "none"), 7)                                 # 0 jobs after passes with some
    b.direct(14, [3] * 65)                                             # 65 per-lane jobs: a last block of 1
    b.direct(15, T_EDGES + BLOCK_EDGES + [4, 3, 3])
    b.edges = [
        ("a", "k_chains: chains of 3, 15, 16, 17, 31, 32, 33, 47, 48 and 49 samples in one block (pass 15 under "
              "class 6: its 19 jobs; pass 3: the first of four); 63 short chains and one of 3000 in one block (pass "
              "11, overflow set, class 13); last blocks of 1 (pass 14) and 63 (pass 2); per-lane ranges that start at "
              "nlong = 1023, 1025, 2049; chain_grid 1 and lane_grid 1 (option set grid_1) beside the defaults"),
        ("b", "class boundary: chains of 2^L - 1, 2^L, 2^L + 1 samples for L = 2 (3, 4, 5) and L = 6 (63, 64, 65: the "
              "last a big group, pass 3); a pass of one class (pass 2: 255 chains of 3); a pass with a job in every "
              "class 1..12 (pass 10)"),
        ("c", "job_chunk over 256 workgroups: main-set job counts 0, 1, 255, 256, 257 and 513 (passes 0..5)"),
        ("d", "k_long_plan / k_long_stash: nlong 0, 1, 1023, 1024, 1025 and 2049 (passes 0, 1, 6..9); nlong == nj "
              "(passes 1, 7); both sets stash in pass 10 (the compare-and-swap from two streams); long chains from "
              "recs, tmp (pass 4), big (passes 3, 10, 12) and lens (passes 10, 11)"),
        ("e", "batches: chain_batches 1, 2, 3 and 16 at 16 passes; with 16 the batches of passes 0, 2, 13 and 14 are "
              "empty (lo == hi) before and after non-empty ones; chain_streams 4 and lane_streams 4"),
        ("f", "lane | wave-pair split: stashed chains of T' - 1, T', T' + 1, T - 1, T, T + 1 samples (T = 40, T' = "
              "20) in pass 3 (an early batch) and pass 15 (the tail batch); lane_long 0"),
    ]
    _built["main"] = b.finish()
    return b


MAIN = dict(SMALL, key_range_passes=16)
MAIN_OPTS = {
    "base": dict(MAIN),
    "batches_1": dict(MAIN, chain_batches=1),
    "batches_3": dict(MAIN, chain_batches=3),
    "batches_16_streams_4": dict(MAIN, chain_batches=16, chain_streams=4, lane_streams=4),
    "grid_1": dict(MAIN, chain_grid=1, lane_grid=1),
    "class_6": dict(MAIN, main_long_class=6, overflow_long_class=6, lane_long=600, lane_tail=100),
    "class_13": dict(MAIN, main_long_class=13, overflow_long_class=13),
    "lane_long_0": dict(MAIN, lane_long=0),
    "tail_async_0": dict(MAIN, tail_async=0),
}


def arena_build():
    """4 passes, no overflow sub-bucket (the overflow scratch and the split path ask for nothing):
    the run arena to the element, and the lane thresholds where every batch takes the smaller."""
    if "arena" in _built:
        return _built["arena"]
    b = ChainBuild("arena", 2, 42)
    b.direct(0, T_EDGES + [4, 3])
    b.singles(b.bucket(1, "none"), 9)
    b.direct(2, cycle([4, 5, 6, 9], 300) + [3] * 5)
    b.direct(3, T_EDGES + [5, 70, 3])
    b.edges = [
        ("f", "4 passes: every batch takes min(lane_long, lane_tail); the thresholds' edges in pass 0 (batch 0) and "
              "pass 3 (the tail batch)"),
        ("g", "work_buffer_elements = the stashed samples exactly: redone 0, long_samples == demand == total; one "
              "less: the reservation of pass 3 (not the first) fails, redone 1, under poison_jobs 1"),
    ]
    _built["arena"] = b.finish()
    return b


ARENA = dict(SMALL, key_range_passes=4)


def passes64_build():
    """64 passes with chain_batches 16: a flush after every fourth pass, most of them empty."""
    if "p64" in _built:
        return _built["p64"]
    b = ChainBuild("passes_64", 6, 43)
    for pas, lengths in ((0, [4, 3]), (3, T_EDGES + [5]), (4, [7, 3, 3]), (20, [64, 9]), (62, [6]),
                         (63, T_EDGES + [4])):
        b.direct(pas, lengths)
    b.edges = [("e", "chain_batches 16 at 64 passes: four passes a batch, flushes after passes 3, 7, ..., 59; chains "
                     "in passes 0, 3, 4, 20, 62 and 63 only")]
    _built["p64"] = b.finish()
    return b


P64 = dict(SMALL, key_range_passes=64, chain_batches=16)


def passes2_build():
    if "p2" in _built:
        return _built["p2"]
    b = ChainBuild("passes_2", 1, 44)
    b.direct(0, T_EDGES + [4, 3, 130])
    b.direct(1, T_EDGES + [5, 3])
    b.edges = [("e", "two passes: the first pass's chains are flushed after it (slot 0), the second's are the tail")]
    _built["p2"] = b.finish()
    return b


P2 = dict(SMALL, key_range_passes=2)

GIANT = dict(main_long_class=2, overflow_long_class=2, lane_long=T_LONG, lane_tail=T_TAIL, poison_jobs=1, giant_class=6,
             heavy_min=64)


def giant_entries(b, pas, ngiant):
    """Split entries of at most 256 heavy keys of 64 members, ngiant of them giant chains (64, now
    and then 70 or 100 samples: equal lengths for k_giant_order's tie rule and a longest one); the
    last entry ends with 32 heavy keys whose best function has 60 members (k_heavy's jobs)."""
    left = ngiant
    while left > 0:
        k = min(left, ph.SPLIT_MAXH) if left > ph.SPLIT_MAXH - 33 else left
        keys = [((70 if j % 50 == 7 else 100 if j == 11 else 64), 0) for j in range(k)]
        left -= k
        if left == 0:
            assert k + 33 <= ph.SPLIT_MAXH
            keys += [(60, 4)] * 33
        b.entry(pas, keys, name="heavy")


def giant_build():
    """4 passes with giant_class 6, heavy_min 64: 1, 2, 3 and 1025 giant chains a pass."""
    if "giant" in _built:
        return _built["giant"]
    b = ChainBuild("giant", 2, 45, span=(120, 120))
    for pas, k in enumerate((1, 2, 3, GORD_MAX // 4 + 1)):
        giant_entries(b, pas, k)
    b.edges = [("h", "k_giant_order / k_chain_dyn: 1, 2, 3 and 1025 giant chains a pass (k_giant_order returns below "
                     "two), equal lengths among them; k_heavy's jobs of 60 samples are stashed from its lens")]
    _built["giant"] = b.finish()
    return b


def giant_4097_build():
    """GORD_MAX + 1 giant chains in one pass: the first 4096 are reordered, the last stays."""
    if "giant_4097" in _built:
        return _built["giant_4097"]
    b = ChainBuild("giant_4097", 1, 46, span=(120, 120))
    giant_entries(b, 0, GORD_MAX + 1)
    b.singles(b.bucket(1, "none"), 5)
    b.edges = [("h", "k_giant_order: GORD_MAX + 1 = 4097 giant chains in one pass")]
    _built["giant_4097"] = b.finish()
    return b


BUILDS = {
    "main": (main_build, MAIN_OPTS),
    "arena": (arena_build, {"base": dict(ARENA), "lane_long_0": dict(ARENA, lane_long=0)}),
    "passes_64": (passes64_build, {"batches_16": dict(P64)}),
    "passes_2": (passes2_build, {"base": dict(P2)}),
    "giant": (giant_build, {"giant_6": dict(GIANT, key_range_passes=4)}),
    "giant_4097": (giant_4097_build, {"giant_6": dict(GIANT, key_range_passes=2)}),
}
