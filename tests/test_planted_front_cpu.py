"""The planted front-end layouts are what test_gpu_front_edges.py claims (no GPU), from the packed
arrays and the restated geometry alone: every declared row, tile and chunk offset holds a window,
all 16 x 24 invalid-byte cases are present and yield exactly the windows a plain per-position check
allows, the declared empty rows and passes are empty under mix43, the full-tile islands give 16
same-pass windows to every lane of a tile, and the oracle keeps every distinct window."""
import numpy as np
import pytest

import oracle_ref
import planted_front as pf
from planted import KEY_BITS, LETTERS, code_of_keys, mix43

LAYOUTS = {"g": pf.layout_g, "e64": pf.layout_e64, "e4": pf.layout_e4, "one": pf.layout_one, "none": pf.layout_none,
           **{f"tail{m}": (lambda m=m: pf.layout_tail(m)) for m in pf.TAIL_MODS}}
_ref = {}


def oracle(name):
    if name not in _ref:
        lay = LAYOUTS[name]()
        _ref[name] = oracle_ref.build(*lay.arrays, lay.nf)
    return _ref[name]


def test_geometry_of_layout_g():
    L = pf.layout_g()
    W = L.windows
    assert W.rp == L.rp == pf.G_RP == int(np.sum(L.arrays[2][L.arrays[3] != pf.UNDEF].astype(np.int64) + 1))
    sel_wg, span = pf.sel_geometry(W.rp)
    assert sel_wg == pf.SEL_WG and span == L.span
    assert 2 * pf.TILE + pf.CHUNK <= span < 3 * pf.TILE      # a third tile, and a short one
    assert span % pf.TILE == pf.CHUNK                        # the last tile is one lane's chunk
    assert (sel_wg - 1) * span >= W.rp > (sel_wg - 2) * span   # the last row starts past rp
    assert W.rp % pf.CHUNK == 7
    lens = L.arrays[2]
    assert 15 <= np.count_nonzero(lens > 400_000) <= 20 and lens.max() == pf.MAX_LEN
    print("layout g: rp", W.rp, "span", span, "sequences", len(lens), "windows", W.n, "positions", W.positions)


def test_declared_offsets_hold_windows():
    L = pf.layout_g()
    W, c, span = L.windows, L.claims, L.span
    named = set()
    for name, p in c["must"].items():
        assert W.has(p), name
        named.add((p // span, p % span))
    for r in (0, 1, pf.G_EDGE_ROWS[1], c["last_row"]):       # row 0, row 1, a middle row, the last non-empty row
        assert any(row == r for row, _ in named), r
    for at in (0, pf.TILE - 1, pf.TILE, span - 1):
        assert sum(1 for _, o in named if o == at) >= 3, at
    assert int(W.pos[-1]) // span == c["last_row"]
    for p in c["isolated"]:
        assert W.has(p) and not W.has(p - 1) and not W.has(p + 1), p
    for p, n in c["dense"]:
        assert W.count_in(p, p + n) == n, p
    # the window at span - 1 has its residues in the next row, the one at TILE - 1 in the next tile
    p, n = c["dense_stretch"]
    assert W.count_in(p, p + n) == n - 7 and not W.has(p - 1) and not W.has(p + n - 7)
    a = L.row(pf.G_DENSE_ROW, pf.TILE)                       # a full tile of distinct keys
    tile = slice(np.searchsorted(W.pos, a), np.searchsorted(W.pos, a + pf.TILE))
    assert tile.stop - tile.start == pf.TILE
    for P in pf.PASSES:
        assert len(np.unique(W.hash[tile] >> np.uint64(KEY_BITS - P.bit_length() + 1))) == P


def plain_windows(b):
    """The windows of an island between two X: offset t is a window iff its 8 bytes are letters."""
    return [t for t in range(len(b) - 7) if all(x in LETTERS for x in b[t:t + 8])]


def test_alignment_sweep():
    L = pf.layout_g()
    W = L.windows
    cases, used = set(), set()
    for q, a, j, b in L.claims["sweep"]:
        assert q % pf.CHUNK == a and len(b) == pf.LANE_BYTES
        assert W.buf[q - 1] == ord("X") and W.buf[q + len(b)] == ord("X")
        assert bytes(W.buf[q:q + len(b)]) == b
        want = plain_windows(b)
        got = [int(p) - q for p in W.pos[np.searchsorted(W.pos, q - 8):np.searchsorted(W.pos, q + len(b) + 8)]]
        assert got == want, (a, j)
        # the build's oracle on the island alone keeps exactly these windows (all singletons)
        one = (np.frombuffer(b, np.uint8), np.zeros(1, np.uint64), np.array([len(b)], np.uint32),
               np.zeros(1, np.uint16), np.zeros(1, np.uint32))
        assert sorted(int(k) for k in oracle_ref.build(*one, 1)["keys"]) == \
            sorted(int.from_bytes(b[t:t + 8], "little") for t in want), (a, j)
        # oracle_ref.kmer_windows restates the annotate side's iterator (for_each_kmer<8>), whose rule
        # is another one: only X and * break a window, and the window that ends right before one is
        # dropped too.  It agrees with the build's rule on the islands without such a byte.
        annot = [int(t) for t in oracle_ref.kmer_windows(b)]
        if isinstance(j, int) and b[j] in b"X*":
            assert annot == [t for t in want if t + 8 != j], (a, j)
        else:
            assert annot == list(range(17)), (a, j)
        if isinstance(j, int):
            assert not pf.VALID[b[j]] and want == [t for t in range(17) if not t <= j <= t + 7]
            cases.add((a, j))
            used.add(b[j])
        else:
            assert want == list(range(17))
            if j == "lower":
                assert b.islower()
    assert cases == {(a, j) for a in range(pf.CHUNK) for j in range(pf.LANE_BYTES)}
    assert used == set(pf.INVALID_BYTES)
    assert sum(1 for _, _, j, _ in L.claims["sweep"] if j is None) == pf.CHUNK
    assert sum(1 for _, _, j, _ in L.claims["sweep"] if j == "lower") == pf.CHUNK


def test_empty_rows():
    L = pf.layout_g()
    W, span = L.windows, L.span
    for r0, r1 in L.claims["empty_rows"]:
        assert r1 - r0 >= 5 and W.count_in(r0 * span, r1 * span) == 0, (r0, r1)
    assert W.rp - int(W.pos[-1]) >= 3 * span
    assert int(W.pos[np.searchsorted(W.pos, 3 * span)]) - 3 * span >= 3 * span   # after rows 0 .. 2
    occupied = np.unique(W.pos // span)
    assert len(occupied) < 200                               # most of the 8192 rows are empty
    assert np.count_nonzero(np.diff(occupied) > 5) >= 6      # runs of at least 5 empty rows, several times


def test_full_tiles():
    L = pf.layout_g()
    W, span = L.windows, L.span
    for row, tile in L.claims["full_tiles"]:
        a = L.row(row, tile * pf.TILE)
        s = slice(np.searchsorted(W.pos, a), np.searchsorted(W.pos, a + pf.TILE))
        assert np.array_equal(W.pos[s], np.arange(a, a + pf.TILE))
        assert len(np.unique(W.hash[s])) == 1                # one pass: 16 windows in every lane's count field
        assert np.array_equal(np.bincount((W.pos[s] - a) // pf.CHUNK), np.full(64, pf.CHUNK))
    (ka, pa, na, _), (ku, pu, nu, _) = L.homo
    assert ka == b"A" * 8 and pa % span == 0 and na == pf.TILE + 2 * pf.CHUNK and pf.homopolymer_hash(b"A"[0]) == 0
    assert pu % span == 0 and nu == 2 * span and W.count_in(pu, pu + nu) == nu
    hu = pf.homopolymer_hash(ku[0])
    for P in pf.PASSES:
        assert hu >> (KEY_BITS - P.bit_length() + 1) >= P // 2
    # the short last tile of a full row: one lane's 16 windows
    assert W.count_in(pu + 2 * pf.TILE, pu + span) == pf.CHUNK == span - 2 * pf.TILE


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_pass_counts(name):
    L = LAYOUTS[name]()
    W = L.windows
    h = mix43(code_of_keys(W.keys))
    for P in pf.PASSES:
        want = np.bincount((h >> np.uint64(KEY_BITS - P.bit_length() + 1)).astype(np.int64), minlength=P)
        assert np.array_equal(L.pass_counts[P], want) and want.sum() == W.n
    assert W.positions == sum(max(int(n) - 7, 0) for n, f in zip(L.arrays[2], L.arrays[3]) if f != pf.UNDEF)


def test_empty_passes():
    for L in (pf.layout_e64(), pf.layout_e4()):
        W, c = L.windows, L.claims
        P = c["passes"]
        assert L.span == pf.CHUNK
        assert [int(p) for p in np.nonzero(L.pass_counts[P])[0]] == c["natural"]
        assert int(W.pos[0]) == c["leading"] == 3 * L.span and W.rp - int(W.pos[-1]) >= 3 * L.span
        last = W.pos // L.span == c["last_row"]
        assert np.count_nonzero(last) == 2 and int(W.pos[-1]) // L.span == c["last_row"]
        in_last = (W.hash >> np.uint64(KEY_BITS - P.bit_length() + 1)) == np.uint64(c["last_pass"])
        if len(c["natural"]) > 1:
            assert np.array_equal(in_last, last)             # that pass's only windows: the last occupied row
        assert np.all(np.diff(W.pos) >= 9) and len(np.unique(W.seq)) == 5
    W = pf.layout_e64().windows
    assert int(W.hash.min()) == 0 and b"A" * 8 == int(W.keys[np.argmin(W.hash)]).to_bytes(8, "little")
    top = pf.largest_valid_hash()
    assert int(W.hash.max()) == top and top >> (KEY_BITS - 18) == (1 << 18) - 1   # last pass, last bucket
    assert all(int(pf.unmix43(np.array([h], np.uint64))[0]) >= pf.NCODES for h in range(top + 1, 1 << KEY_BITS))
    assert pf.layout_one().windows.n == 1 and pf.layout_none().windows.n == 0
    assert pf.layout_none().windows.positions > 0


def test_small_sequences_and_undefined():
    L = pf.layout_g()
    W, c = L.windows, L.claims
    _, off, lens, funcs, _ = L.arrays
    for name, mod in (("run1", 0), ("run2", pf.BLOCK - 3)):
        start, (s8, p8) = c[name]
        assert start % pf.BLOCK == mod
        k = int(np.searchsorted(W.pos, p8))
        assert W.pos[k] == p8 and W.seq[k] == s8 and W.i[k] == 0 and lens[s8] == 8
        assert W.count_in(start, p8) == 0
        run = [s for s in range(s8) if funcs[s] != pf.UNDEF and W.pstart[np.searchsorted(W.kept, s)] >= start]
        assert len(run) >= 100 and all(lens[s] < 8 for s in run) and any(lens[s] == 0 for s in run)
        assert any(funcs[s] == pf.UNDEF and lens[s] >= 8 for s in range(run[0], s8))
    # dozens of sequences share the 64-byte block ahead of run 1's window
    p8 = c["run1"][1][1]
    assert p8 % pf.BLOCK == 40 and np.count_nonzero(W.buf[p8 - p8 % pf.BLOCK:p8] == 0) == 30
    eights = c["eights"]
    assert len(eights) == 64 and all(p == eights[0][1] + 9 * k for k, (_, p) in enumerate(eights))
    k0 = int(np.searchsorted(W.pos, eights[0][1]))
    assert np.array_equal(W.pos[k0:k0 + 64], [p for _, p in eights])
    assert np.array_equal(W.seq[k0:k0 + 64], [s for s, _ in eights]) and not W.i[k0:k0 + 64].any()
    # sequences with the undefined function: interleaved, some with valid windows, none in the result
    und = [s for s in range(len(lens)) if funcs[s] == pf.UNDEF]
    assert len(und) >= 20 and 0 < und[0] and und[-1] < len(lens) - 1
    res = L.arrays[0]
    hidden = 0
    for s in und:
        b = bytes(res[int(off[s]):int(off[s]) + int(lens[s])])
        ks = [int.from_bytes(b[t:t + 8], "little") for t in plain_windows(b)]
        hidden += len(ks)
        assert not np.isin(np.array(ks, np.uint64), W.keys).any()
        assert not np.isin(np.array(ks, np.uint64), oracle("g")["keys"]).any()
    assert hidden > 500
    assert len(set(int(f) for f in funcs)) > 100             # functions vary per sequence


def test_longest_protein_and_cross():
    L = pf.layout_g()
    W, c = L.windows, L.claims
    big, start = c["big"]
    assert L.arrays[2][big] == pf.MAX_LEN == 1_048_575
    mine = W.i[W.seq == big]
    assert set(pf.G_BIG_I) <= set(int(i) for i in mine) and int(mine.max()) == pf.MAX_LEN - 8 == 1_048_567
    assert int(mine.max()).bit_length() == pf.ELEM_I_BITS and (int(mine.max()) >> 19) == 1
    x = c["cross"]
    assert W.buf[x] == 0
    near = W.pos[np.searchsorted(W.pos, x - 40):np.searchsorted(W.pos, x + 40)]
    assert [int(p) for p in near] == list(range(x - 15, x - 7)) + list(range(x + 1, x + 9))
    assert len(set(int(s) for s in W.seq[np.searchsorted(W.pos, x - 40):np.searchsorted(W.pos, x + 40)])) == 2


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_oracle_keeps_every_distinct_window(name):
    L = LAYOUTS[name]()
    W = L.windows
    ref = oracle(name)
    _, _, lens, funcs, _ = L.arrays
    assert len(ref["keys"]) == L.distinct == len(np.unique(W.keys)) == ref["distinct_signatures"]
    assert ref["n_seqs_with_signature"] == len(np.unique(W.seq))
    if W.n == 0:
        return
    at = np.searchsorted(ref["keys"], W.keys)
    assert np.array_equal(ref["keys"][at], W.keys)
    homo = np.isin(W.keys, np.array([int.from_bytes(h[0], "little") for h in L.homo], np.uint64))
    d = ref["data"][at[~homo]]
    # a singleton's record names its sequence's function and its offset from the end
    assert np.array_equal(d["function_index"], funcs[W.seq[~homo]])
    assert np.array_equal(d["avg_from_end"], ((lens[W.seq[~homo]].astype(np.int64) - W.i[~homo]) & 0xFFFF))
    # the homopolymers by hand: n windows of one key in one sequence, all of its function, so kept;
    # avg_from_end is the upper median of (len - i) mod 2^16
    for kmer, p, n, s in L.homo:
        row = ref["data"][np.searchsorted(ref["keys"], np.uint64(int.from_bytes(kmer, "little")))]
        i0 = p - int(W.pstart[np.searchsorted(W.kept, s)])
        offs = np.sort((int(lens[s]) - (i0 + np.arange(n))) & 0xFFFF)
        assert row["function_index"] == funcs[s] and row["avg_from_end"] == offs[n // 2], kmer
        assert np.count_nonzero(W.keys == np.uint64(int.from_bytes(kmer, "little"))) == n


@pytest.mark.parametrize("mod", pf.TAIL_MODS)
def test_tails(mod):
    L = pf.layout_tail(mod)
    W = L.windows
    assert W.rp % pf.CHUNK == mod and int(L.arrays[2].sum()) < pf.BLOCK
    assert int(W.pos[-1]) + 8 == W.rp - 1                    # the last window ends on the last residue
    assert W.n == 4 and W.seq[-1] == 1
