"""Pure-Python restatement of the build and call-side window rules -- TEST INFRASTRUCTURE.

A second, independently written checker for SMALL inputs (dict grouping + Python loops), used to
cross-check the C++ oracle (oracle/skm_oracle.cpp) on randomized tiny cases.  It follows the same
reference lines:
  build_py        signature_build.tcc:121-181 (windows), :184-213 (group visit), :219-293 (cut/stats)
  P2              Boost.Accumulators p_square_quantile, p = 0.5
  call_windows    for_each_kmer, kmer_data.h:76-102
  hitset_calls    process_aa_seq and HitSet::process, call_functions.tcc:259-338, :35-103
Parity with the reference itself is unpinned: the reference ships no fixtures.
"""
from __future__ import annotations

import struct

OK_PROT = set(b"ACDEFGHIKLMNPQRSTVWYacdefghiklmnpqrstvwy")  # signature_build.h:102-103


def d2u16(d: float) -> int:
    """(unsigned short) of a double as gcc/x86-64 emits it: cvttsd2si to int32, keep 16 bits."""
    if not (-2147483649.0 < d < 2147483648.0):
        return 0
    return int(d) & 0xFFFF  # int() truncates toward zero like cvttsd2si


class P2:
    """p_square_quantile with p = 0.5: heights, actual and desired marker positions."""

    def __init__(self):
        self.h = [0.0] * 5
        self.n = [1.0, 2.0, 3.0, 4.0, 5.0]
        self.d = [1.0, 2.0, 3.0, 4.0, 5.0]
        self.cnt = 0

    def add(self, x: int):
        self.cnt += 1
        x = float(x)
        if self.cnt <= 5:
            self.h[self.cnt - 1] = x
            if self.cnt == 5:
                self.h.sort()
            return
        h, n, d = self.h, self.n, self.d
        if x < h[0]:
            h[0] = x
            cell = 1
        elif x >= h[4]:
            h[4] = x
            cell = 4
        else:
            cell = next(k for k in range(5) if h[k] > x)  # upper_bound
        for k in range(cell, 5):
            n[k] += 1.0
        for k, inc in enumerate((0.0, 0.25, 0.5, 0.75, 1.0)):
            d[k] += inc
        for i in (1, 2, 3):
            di = d[i] - n[i]
            dp = n[i + 1] - n[i]
            dm = n[i - 1] - n[i]
            hp = (h[i + 1] - h[i]) / dp
            hm = (h[i - 1] - h[i]) / dm
            if (di >= 1.0 and dp > 1.0) or (di <= -1.0 and dm < -1.0):
                s = 1 if di > 0 else -1
                hh = h[i] + s / (dp - dm) * ((s - dm) * hp + (dp - s) * hm)
                if h[i - 1] < hh < h[i + 1]:
                    h[i] = hh
                elif di > 0:
                    h[i] = h[i] + hp
                else:
                    h[i] = h[i] - hm
                n[i] += s

    def result(self) -> float:
        return self.h[2]


def group_stats(lengths_in_visit_order):
    """accumulator_set<unsigned short, stats<mean, median, variance>> over the visit sequence."""
    cnt, s, var = 0, 0, 0.0
    p2 = P2()
    for x in lengths_in_visit_order:
        cnt += 1
        s = (s + x) & 0xFFFF
        p2.add(x)
        if cnt > 1:
            m = s / cnt
            t = x - m
            var = var * (cnt - 1) / cnt + t * t / (cnt - 1)
    mean = s / cnt
    return d2u16(mean), d2u16(p2.result()), d2u16(var)


def ref_chain(xs):
    """One deferred chain over the samples in visit order: (P^2 median, running variance with the
    u16-wrapping sum), raw doubles."""
    p2 = P2()
    cnt, s, var = 0, 0, 0.0
    for x in xs:
        x = int(x)
        cnt += 1
        s = (s + x) & 0xFFFF
        p2.add(x)
        if cnt > 1:
            m = s / cnt
            t = x - m
            var = var * (cnt - 1) / cnt + t * t / (cnt - 1)
    return p2.result(), var


def f32(x: float) -> float:
    return struct.unpack("<f", struct.pack("<f", x))[0]


def build_py(seqs, funcs, seq_ids, n_functions):
    """seqs: list of bytes; funcs: FunctionIndex per sequence (0xFFFF = skipped).
    Returns (dict key->(avg_from_end, func, mean, median, var), distinct_functions,
    seqs_with_func, n_seqs_with_signature)."""
    groups = {}
    seqs_with_func = [0] * n_functions
    for s, (seq, fn) in enumerate(zip(seqs, funcs)):
        if fn == 0xFFFF:
            continue
        seqs_with_func[fn] += 1
        for i in range(len(seq) - 7):
            w = seq[i:i + 8]
            if all(c in OK_PROT for c in w):
                key = int.from_bytes(w, "little")
                groups.setdefault(key, []).append((s, i))
    out = {}
    distinct = [0] * n_functions
    sig_seqs = set()
    for key, occ in groups.items():
        visit = occ[::-1]  # TBB 2020 multimap: reverse insertion order
        fc = {}
        for s, _ in visit:
            fc[funcs[s]] = fc.get(funcs[s], 0) + 1
        best_f, best_c = None, -1
        for fn in sorted(fc):
            if fc[fn] > best_c:
                best_f, best_c = fn, fc[fn]
        count = len(visit)
        if f32(float(best_c)) < f32(f32(float(count)) * f32(0.8)):
            continue
        lens = [len(seqs[s]) for s, _ in visit if funcs[s] == best_f]
        mean, med, var = group_stats(lens)
        offs = sorted((len(seqs[s]) - i) & 0xFFFF for s, i in visit)
        for s, _ in visit:
            sig_seqs.add(seq_ids[s])
        distinct[best_f] += 1
        out[key] = (offs[len(offs) // 2], best_f, mean, med, var)
    return out, distinct, seqs_with_func, len(sig_seqs)


def call_windows(seq: bytes):
    """for_each_kmer<8> (kmer_data.h:76-102): yields (offset, key) of the windows the call path
    looks up.  Only 'X' and '*' are ambiguous, and a window is also skipped when the ambiguous
    character sits immediately after it (next_ambig <= ptr + 8)."""
    n = len(seq)
    out = []
    p = 0
    while p + 8 <= n:
        nxt = next((q for q in range(p, n) if seq[q] in b"X*"), n)
        if nxt <= p + 8 and nxt < n:
            p = nxt + 1
            continue
        out.append((p, int.from_bytes(seq[p:p + 8], "little")))
        p += 1
    return out


def matrix_distance(seqs, seq_idx, fetch, hypo_index):
    """kmers-matrix-distance (kmers-matrix-distance.cc:123-196): every window of for_each_kmer whose
    record (fetch(key) -> (avg, func, mean, median, var) or None) is not hypothetical and whose
    sequence length lies within mean -/+ 2 sd (sd = sqrt(var), or 0.1 * seqlen when var == 0) adds
    the sequence's index to the k-mer's set; every pair id1 < id2 of a set counts once.
    Returns {(id1, id2): count}."""
    import math
    sets = {}
    for s, seq in enumerate(seqs):
        seqlen = float(len(seq))
        for _, key in call_windows(seq):
            kd = fetch(key)
            if kd is None or kd[1] == hypo_index:
                continue
            mean = float(kd[2])
            sd = seqlen * 0.1 if kd[4] == 0 else math.sqrt(float(kd[4]))
            if seqlen < mean - sd * 2.0 or seqlen > mean + sd * 2.0:
                continue
            sets.setdefault(key, set()).add(int(seq_idx[s]))
    dist = {}
    for ids in sets.values():
        v = sorted(ids)
        for a in range(len(v)):
            for b in range(a + 1, len(v)):
                dist[(v[a], v[b])] = dist.get((v[a], v[b]), 0) + 1
    return dist


def _bm_mean(vals, mean_mode):
    """boost::math::statistics::mean over float32 values in hit order: the four-lane form of
    Boost >= 1.76 (mean_mode 0) or the single running mean (mean_mode 1), every step rounded to
    float32."""
    import numpy as np
    F = np.float32
    n = len(vals)
    if mean_mode == 1:
        mu, i = F(0), F(1)
        for x in vals:
            mu = mu + (x - mu) / i
            i = i + F(1)
        return mu
    end = n - n % 4
    mu = [F(0), F(0), F(0), F(0)]
    i = F(1)
    for it in range(0, end, 4):
        inv = F(1) / i
        for j in range(4):
            mu[j] = mu[j] + (vals[it + j] - mu[j]) * inv
        i = i + F(1)
    num1 = F(end) / F(4)
    num2 = num1 + F(n % 4)
    for it in range(end, n):  # the tail runs on lane 3
        mu[3] = mu[3] + (vals[it] - mu[3]) / i
        i = i + F(1)
    return (num1 * (mu[0] + mu[1] + mu[2]) + num2 * mu[3]) / F(n)


def hitset_calls(length, hits, min_hits, max_gap, ignore_hypo, hypo_index, mean_mode):
    """process_aa_seq and HitSet::process (call_functions.tcc:259-338, :35-103) over one sequence of
    `length` residues whose DB hits are `hits`: (window position, function_index, mean) in window
    order.  Returns the calls as (start, end, count, function_index, median as unsigned, MAD as
    numpy.float32).

    The statistics are Boost.Math's on std::vector<float>: the mean as _bm_mean, the median and the
    MAD as order statistics of the sorted values and of |float(x) - median| (the corrected MAD,
    mad_mode 0; the older one depends on libstdc++'s nth_element permutation and is left to the C++
    oracle), mad == 0 -> 30, the cut-offs mean -/+ 2 mad in double.  min_hits >= 2: with one hit
    the reference's process() reads end[1] before the beginning of its vector."""
    import numpy as np
    F = np.float32
    assert min_hits >= 2
    calls = []
    held = []      # the HitSet: (pos, function_index, mean)
    cur = 0xFFFF   # UndefinedFunction
    seqlen = float(length)

    def process():
        nonlocal cur, held
        mine = [h for h in held if h[1] == cur]
        vals = [F(h[2]) for h in mine]
        n = len(vals)
        mean = _bm_mean(vals, mean_mode)
        srt = np.sort(np.array(vals, F))
        median = srt[(n - 1) // 2] if n & 1 else (srt[n // 2 - 1] + srt[n // 2]) / F(2)
        dev = np.sort(np.abs(srt - median))
        mad = dev[(n - 1) // 2] if n & 1 else (dev[n // 2 - 1] + dev[n // 2]) / F(2)
        if mad == 0:
            mad = F(30)
        cutoff_b = float(mean) - 2.0 * float(mad)
        cutoff_t = float(mean) + 2.0 * float(mad)
        if n >= min_hits and not (seqlen < cutoff_b or seqlen > cutoff_t):
            calls.append((held[0][0], mine[-1][0] + 7, n, cur, int(median), F(mad)))
        if held[-2][1] != cur and held[-2][1] == held[-1][1]:
            cur = held[-2][1]
            held = held[-2:]
        else:
            held = []

    for pos, func, mean in hits:
        if ignore_hypo and func == hypo_index:
            continue
        if held and held[-1][0] + max_gap < pos:
            if len(held) >= min_hits:
                process()
            else:
                held = []
        if not held:
            cur = func
        held.append((pos, func, mean))
        if len(held) > 1 and cur != func and held[-2][1] == held[-1][1]:
            process()
    if len(held) >= min_hits:
        process()
    return calls
