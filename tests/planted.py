"""Planted inputs for the group-by kernels -- a plain helper module of the tests.

mix43 (the 43-bit hash of a k-mer's base-40 code, skm_common.h, restated here) is a bijection on
43 bits, so it can be inverted: a k-mer can be made to land in a chosen level-1 bucket, a chosen
level-2 sub-bucket and a chosen home slot of the LDS hash table.  Every occurrence gets a protein
of its own, X*a + 8-mer + X*b (exactly one valid window; length and offset vary), so every bucket,
sub-bucket and group has exactly the size its scenario states.

The element's bit layout (set_geometry and k_bucket_process in skm_build.hip), from the top of the
43-bit hash: pass bits (log2 of the key-range passes), owner bits (log2 of the world size), b1_bits
of level-1 bucket, then `rem`.  The level-2 sub-bucket of a partitioned bucket is the top b2 bits of
rem, b2 from the bucket's total; the home slot of the LDS table is a multiplicative hash of rem.

A Scenario owns one level-1 bucket (one prefix): different scenarios are walked by different
workgroups, so one build holds many of them and its result is compared scenario by scenario."""
import numpy as np

CAP = 2048            # elements of one LDS batch (process_sub)
TAB_BITS = 12         # the LDS hash table has 2 * CAP slots
SUB_TARGET = 768      # k_partition: target elements per level-2 sub-bucket
MAX_B2 = 11
HEAVY_MIN = 1024      # occurrences that make a key of an overflow sub-bucket heavy (k_ovf_split)
HV_FT = 4096          # k_heavy: the largest n_functions that takes the LDS function table
SLOT_MULT = 0x9E3779B1
KEY_BITS = 43
KEY_MASK = (1 << KEY_BITS) - 1
MIX_M1, MIX_M2, MIX_SHIFT = 0x3C6EF372FE9, 0x5851F42D4C9, 22
NCODES = 40 ** 8
LETTERS = b"ACDEFGHIKLMNPQRSTVWY" + b"acdefghiklmnpqrstvwy"
LONG_A, LONG_B = 40000, 30000  # a protein of more than 65535 residues: X*LONG_A + 8-mer + X*LONG_B


def _inv_odd(m):
    x = m
    for _ in range(6):
        x = (x * (2 - m * x)) & ((1 << 64) - 1)
    return x & KEY_MASK


MIX_I1, MIX_I2 = _inv_odd(MIX_M1), _inv_odd(MIX_M2)


def mix43(k):
    k = np.asarray(k, np.uint64)
    x = (k * np.uint64(MIX_M1)) & np.uint64(KEY_MASK)
    x = x ^ (x >> np.uint64(MIX_SHIFT))
    x = (x * np.uint64(MIX_M2)) & np.uint64(KEY_MASK)
    return x ^ (x >> np.uint64(MIX_SHIFT))


def unmix43(x):
    x = np.asarray(x, np.uint64)
    x = x ^ (x >> np.uint64(MIX_SHIFT))
    x = (x * np.uint64(MIX_I2)) & np.uint64(KEY_MASK)
    x = x ^ (x >> np.uint64(MIX_SHIFT))
    return (x * np.uint64(MIX_I1)) & np.uint64(KEY_MASK)


def pack(seqs):
    lens = np.array([len(s) for s in seqs], np.uint32)
    off = np.zeros(len(seqs), np.uint64)
    off[1:] = np.cumsum(lens[:-1])
    return np.frombuffer(b"".join(seqs), np.uint8), off, lens


def assert_same(got, ref):
    np.testing.assert_array_equal(got.keys, ref["keys"])
    for f in ("avg_from_end", "function_index", "mean", "median", "var"):
        bad = np.nonzero(got.data[f] != ref["data"][f])[0]
        assert len(bad) == 0, (f, len(bad), got.data[bad[:5]], ref["data"][bad[:5]],
                               [int(k).to_bytes(8, "little") for k in got.keys[bad[:5]]])
    np.testing.assert_array_equal(got.distinct_functions, ref["distinct_functions"])
    np.testing.assert_array_equal(got.seqs_with_func, ref["seqs_with_func"])
    assert got.n_seqs_with_signature == ref["n_seqs_with_signature"]
    assert got.distinct_signatures == ref["distinct_signatures"]


def kmer_of(code):
    code = int(code)
    out = bytearray(8)
    for j in range(7, -1, -1):
        code, d = divmod(code, 40)
        out[j] = LETTERS[d]
    return bytes(out)


_DIGIT = np.full(256, 255, np.uint64)
_DIGIT[np.frombuffer(LETTERS, np.uint8)] = np.arange(40, dtype=np.uint64)


def code_of_keys(keys):
    """The base-40 codes of k-mers given as little-endian u64 (the builder's keys): byte j of the
    key is residue j, the first residue the most significant digit."""
    keys = np.ascontiguousarray(keys, np.uint64)
    code = np.zeros(len(keys), np.uint64)
    for j in range(8):
        d = _DIGIT[((keys >> np.uint64(8 * j)) & np.uint64(0xFF)).astype(np.int64)]
        assert np.all(d < np.uint64(40))
        code = code * np.uint64(40) + d
    return code


def hash_of_keys(keys):
    return mix43(code_of_keys(keys))


_codes = {}


def bucket_codes():
    """The valid codes of one sub-bucket: same top 23 hash bits as the code of b"MKVLAAGI"."""
    if "c" not in _codes:
        first = 0
        for ch in b"MKVLAAGI":
            first = first * 40 + LETTERS.index(ch)
        top = int(mix43(np.array([first], np.uint64))[0]) >> 20
        c = unmix43((np.uint64(top) << np.uint64(20)) | np.arange(1 << 20, dtype=np.uint64))
        assert np.all(mix43(c) >> np.uint64(20) == np.uint64(top))
        c = c[c < np.uint64(NCODES)]
        c = c[c != np.uint64(first)]
        np.random.default_rng(1234).shuffle(c)
        _codes["c"] = (first, c)
    return _codes["c"]


class Planter:
    """Occurrences of k-mers of the one sub-bucket, one protein each."""

    def __init__(self, seed, nf=6):
        self.rng = np.random.default_rng(seed)
        self.nf = nf
        self.heavy_code, self.codes = bucket_codes()
        self.next = 0
        self.seqs, self.funcs, self.light = [], [], []

    def code(self):
        self.next += 1
        return self.codes[self.next - 1]

    def plant(self, code, funcs, light, long_at=None):
        kmer = kmer_of(code)
        for j, fn in enumerate(funcs):
            a, b = int(self.rng.integers(0, 60)), int(self.rng.integers(0, 60))
            if long_at is not None and j == long_at:
                a, b = LONG_A, LONG_B  # a protein of more than 65535 residues
            self.seqs.append(b"X" * a + kmer + b"X" * b)
            self.funcs.append(fn)
            self.light.append(light)
        return kmer

    def heavy(self, n, funcs=None, code=None):
        return self.plant(self.heavy_code if code is None else code, funcs or [1] * n, False)

    def group(self, funcs, long_at=None):
        return self.plant(self.code(), list(funcs), True, long_at)

    def singletons(self, n):
        for _ in range(n):
            self.group([int(self.rng.integers(0, self.nf))])

    def arrays(self, order="shuffled"):
        """order: the light members' sequences first, last, or shuffled among the heavy ones."""
        n = len(self.seqs)
        light = np.array(self.light, bool)
        perm = self.rng.permutation(n)
        if order == "first":
            perm = np.concatenate([perm[light[perm]], perm[~light[perm]]])
        elif order == "last":
            perm = np.concatenate([perm[~light[perm]], perm[light[perm]]])
        res, off, lens = pack([self.seqs[k] for k in perm])
        return res, off, lens, np.array(self.funcs, np.uint16)[perm], np.arange(n, dtype=np.uint32)


# ---------------------------------------------------------------------------------------------
# the element's bit layout
# ---------------------------------------------------------------------------------------------
class Geometry:
    """Where a 43-bit hash goes: `prefix` (pass, owner, level-1 bucket) selects the workgroup,
    `rem` is what that workgroup groups by."""

    def __init__(self, pass_bits=0, owner_bits=0):
        self.pass_bits, self.owner_bits = pass_bits, owner_bits
        self.b1_bits = (13 if owner_bits >= 2 else 12) - owner_bits
        self.prefix_bits = pass_bits + owner_bits + self.b1_bits
        self.rem_bits = KEY_BITS - self.prefix_bits

    def prefix_of(self, h):
        return np.asarray(h, np.uint64) >> np.uint64(self.rem_bits)

    def rem_of(self, h):
        return np.asarray(h, np.uint64) & np.uint64((1 << self.rem_bits) - 1)

    def sub_of(self, h, b2):
        """The level-2 sub-bucket: the top b2 bits of rem."""
        return self.rem_of(h) >> np.uint64(self.rem_bits - b2)

    def slot_of(self, h):
        """The home slot of the LDS hash table (process_sub)."""
        return ((self.rem_of(h) * np.uint64(SLOT_MULT)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - TAB_BITS)


def b2_of(n):
    """k_partition's choice: the smallest b2 with (n >> b2) <= SUB_TARGET, at most MAX_B2."""
    b2 = 0
    while b2 < MAX_B2 and (n >> b2) > SUB_TARGET:
        b2 += 1
    return b2


def codes(prefix_bits, prefix, n, rng, where=None):
    """n distinct valid base-40 codes (< 40^8) whose 43-bit hash has the given top prefix_bits:
    walks the low hash bits from a random start and inverts mix43.  where: a filter on the hashes
    (array -> bool array)."""
    low_bits = KEY_BITS - prefix_bits
    size = 1 << low_bits
    assert 0 <= prefix < (1 << prefix_bits)
    span = min(size, 1 << 16)
    pos = int(rng.integers(0, size))
    out, have, walked = [], 0, 0
    while have < n:
        assert walked < size, "not enough codes under this prefix and filter"
        low = (np.uint64(pos) + np.arange(span, dtype=np.uint64)) & np.uint64(size - 1)
        h = (np.uint64(prefix) << np.uint64(low_bits)) | low
        c = unmix43(h)
        ok = c < np.uint64(NCODES)
        if where is not None:
            ok &= where(h)
        out.append(c[ok])
        have += int(np.count_nonzero(ok))
        pos = (pos + span) & (size - 1)
        walked += span
    return np.concatenate(out)[:n]


# ---------------------------------------------------------------------------------------------
# scenarios
# ---------------------------------------------------------------------------------------------
class Scenario:
    """One level-1 bucket with planted groups.

    name, geom, prefix: the bucket.  seqs / funcs: its proteins.  expect: {kmer: kept?}, written by
    hand with every group.  sub_sizes: the declared sizes of its level-2 sub-buckets in sub-bucket
    order (None: the bucket is declared by its total alone), b2 the declared split.  big_groups /
    big_kept / overflow_subbuckets / overflow_elements: its declared contribution to the counters."""

    def __init__(self, name, geom, prefix, seed, nf, total, sub_sizes=None, b2=None):
        self.name, self.geom, self.prefix, self.nf = name, geom, prefix, nf
        self.rng = np.random.default_rng(seed)
        self.total, self.sub_sizes, self.b2 = total, sub_sizes, b2
        if sub_sizes is not None:
            assert b2 is not None and len(sub_sizes) == 1 << b2 and sum(sub_sizes) == total
            assert b2 == b2_of(total), (name, "declared b2 is not the kernel's choice", b2, b2_of(total))
        self.seqs, self.funcs = [], []
        self.expect = {}
        self.groups = []  # (kmer, member functions) of every key, singletons included
        self.big_groups = self.big_kept = 0
        self.overflow_subbuckets = self.overflow_elements = 0
        self.has_long = self.has_twice = False
        self._used = set()
        self._pool = {}

    # -- codes -------------------------------------------------------------------------------
    def _fresh(self, c):
        out = []
        for v in c:
            v = int(v)
            if v not in self._used:
                self._used.add(v)
                out.append(v)
        return out

    def take(self, n, sub=None, where=None):
        """n unused codes of this bucket; sub: of that level-2 sub-bucket (needs b2), or (bits,
        value) for the top `bits` bits of rem; where: a filter on the hash."""
        pb, px = self.geom.prefix_bits, self.prefix
        if sub is not None:
            bits, val = sub if isinstance(sub, tuple) else (self.b2, sub)
            pb, px = pb + bits, (px << bits) | val
        if where is not None:
            got = []
            while len(got) < n:
                got += self._fresh(codes(pb, px, n - len(got), self.rng, where))
            return got
        pool = self._pool.setdefault(sub, [])
        while len(pool) < n:
            pool += self._fresh(codes(pb, px, max(n - len(pool), 512), self.rng))
        self._pool[sub] = pool[n:]
        return pool[:n]

    # -- proteins ----------------------------------------------------------------------------
    def _protein(self, kmer, fn, long=False, twice=False):
        a, b = int(self.rng.integers(0, 60)), int(self.rng.integers(0, 60))
        if long:
            a, b = LONG_A, LONG_B
            self.has_long = True
        if twice:
            self.has_twice = True
        self.seqs.append(b"X" * a + kmer + (b"X" + kmer if twice else b"") + b"X" * b)
        self.funcs.append(fn)

    def group(self, funcs, kept, sub=None, where=None, long_at=None, twice_at=None, code=None):
        """One k-mer with len(funcs) occurrences, occurrence j in a protein of function funcs[j].
        kept: the expectation, written by the caller.  long_at: that occurrence's protein has more
        than 65535 residues.  twice_at: occurrences twice_at and twice_at + 1 (same function) are
        one protein, 8-mer + X + 8-mer."""
        funcs = list(funcs)
        if code is None:
            code = self.take(1, sub, where)[0]
        kmer = kmer_of(code)
        j = 0
        while j < len(funcs):
            tw = twice_at is not None and j == twice_at
            if tw:
                assert funcs[j] == funcs[j + 1]
            self._protein(kmer, funcs[j], long=(long_at is not None and j == long_at), twice=tw)
            j += 2 if tw else 1
        assert kmer not in self.expect
        self.expect[kmer] = kept
        self.groups.append((kmer, funcs))
        return kmer

    def singletons(self, n, sub=None, where=None):
        """n keys of one occurrence each (always kept), random functions."""
        for code in self.take(n, sub, where):
            self.group([int(self.rng.integers(0, self.nf))], True, code=code)

    def n_elements(self):
        return sum(len(f) for _, f in self.groups)


def best_mix(c, nbest, f, others):
    """c member functions in an interleaved order: nbest of function f, the rest cycling through
    `others`, spread evenly among them."""
    out, k, acc = [], 0, 0
    for _ in range(c):
        acc += c - nbest
        if acc >= c and others:
            acc -= c
            out.append(others[k % len(others)])
            k += 1
        else:
            out.append(f)
    assert len(out) == c and out.count(f) == nbest and f not in others, (c, nbest, out.count(f))
    return out


def assemble(scenarios, seed):
    """The build's input: every scenario's proteins, their order shuffled by a fixed seed."""
    seqs = [s for sc in scenarios for s in sc.seqs]
    funcs = np.array([f for sc in scenarios for f in sc.funcs], np.uint16)
    perm = np.random.default_rng(seed).permutation(len(seqs))
    res, off, lens = pack([seqs[k] for k in perm])
    return res, off, lens, funcs[perm], np.arange(len(seqs), dtype=np.uint32)


def windows_of(seq):
    """The offsets of the valid windows of a planted protein (residues other than the 40 letters
    break a window), restated without the oracle."""
    ok = _DIGIT[np.frombuffer(seq, np.uint8)] < np.uint64(40)
    run = np.zeros(len(seq) + 1, np.int64)
    run[1:] = np.cumsum(ok)
    return np.nonzero(run[8:] - run[:-8] == 8)[0]


def scenario_hashes(sc):
    """(hash, function) of every valid window of the scenario's proteins, from the residues."""
    hs, fs = [], []
    for seq, fn in zip(sc.seqs, sc.funcs):
        for i in windows_of(seq):
            w = int.from_bytes(seq[i:i + 8], "little")
            hs.append(w)
            fs.append(fn)
    return hash_of_keys(np.array(hs, np.uint64)), np.array(fs, np.int64), np.array(hs, np.uint64)


def assert_scenarios(got_keys, got_data, ref, scenarios):
    """Bit-exact comparison scenario by scenario (the keys whose hash has the scenario's prefix),
    then the hand-written expectations: a failure names the scenario, the field and the k-mers."""
    geom = scenarios[0].geom
    gp = geom.prefix_of(hash_of_keys(got_keys))
    rp = geom.prefix_of(hash_of_keys(ref["keys"]))
    for sc in scenarios:
        gk, gd = got_keys[gp == np.uint64(sc.prefix)], got_data[gp == np.uint64(sc.prefix)]
        rk, rd = ref["keys"][rp == np.uint64(sc.prefix)], ref["data"][rp == np.uint64(sc.prefix)]
        missing = np.setdiff1d(rk, gk)
        extra = np.setdiff1d(gk, rk)
        assert len(missing) == 0 and len(extra) == 0, (
            sc.name, "kept set", "missing", [int(k).to_bytes(8, "little") for k in missing[:5]], len(missing),
            "extra", [int(k).to_bytes(8, "little") for k in extra[:5]], len(extra))
        assert np.array_equal(gk, rk), (sc.name, "key order")
        for f in ("avg_from_end", "function_index", "mean", "median", "var"):
            bad = np.nonzero(gd[f] != rd[f])[0]
            assert len(bad) == 0, (sc.name, f, len(bad), gd[bad[:5]], rd[bad[:5]],
                                   [int(k).to_bytes(8, "little") for k in gk[bad[:5]]])
        kept = set(int(k) for k in gk)
        wrong = [k for k, is_kept in sc.expect.items() if (int.from_bytes(k, "little") in kept) != is_kept]
        assert not wrong, (sc.name, "expectation", wrong[:5], len(wrong))
        assert len(gk) == sum(sc.expect.values()), (sc.name, "kept count")


def counter_sums(scenarios):
    return {f: sum(getattr(sc, f) for sc in scenarios)
            for f in ("big_groups", "big_kept", "overflow_subbuckets", "overflow_elements")}
