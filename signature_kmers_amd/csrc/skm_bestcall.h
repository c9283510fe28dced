// skm_bestcall.h -- find_best_call (call_functions.tcc:347-659) for one sequence, on ids instead of
// strings, for host and device.  The kernel (skm_bestcall.hip k_best_calls) and the host batch
// (skm_best_calls_host) both call best_call_one; skm_find_best_call (skm_host.cpp) is the string
// form it is checked against (tests/test_best_call_cpu.py), and tests/native/bestcall_check.cpp
// compiles BestTop against std::partial_sort itself.
//
// What the strings are reduced to beforehand (skm_fidx, one entry per function index plus one for
// every index fname() maps to ""):
//   rank   dense rank of the name under std::string order ("" = 0): `if (f2 > f1) swap`
//   whole  string-pool id of the whole name
//   parts  pool ids of skm_str::split(name, " / "), same pool: the std::map<std::string, char>
//          lookups of the fusion keys become lookups by id
// A name of more than SKM_BEST_MAX_PARTS parts has nparts = SKM_BEST_COMPLEX and no part ids.
#pragma once
#include <cstdint>

#include "../../include/skm.h"
#include "skm_select.h"

namespace skm {

constexpr uint32_t SKM_BEST_COMPLEX = 0xFFFFFFFFu;
constexpr uint16_t SKM_BEST_DEFERRED = 0x8000;  // flags bit, internal: cleared before a caller sees it

struct BestFunc {  // 44 bytes
    uint32_t rank, whole, nparts;
    uint32_t parts[SKM_BEST_MAX_PARTS];
};
struct BestTables {
    const BestFunc* ent;  // [nfunc + 1]; ent[nfunc] is the name ""
    uint32_t nfunc;
};

// fname(): UndefinedFunction and every index past the table are the name ""
SKM_HD inline const BestFunc& best_func(const BestTables& t, uint32_t fi) {
    return t.ent[(fi == SKM_UNDEFINED_FUNCTION || fi >= t.nfunc) ? t.nfunc : fi];
}

// std::partial_sort(vec.begin(), vec.begin() + 2, vec.end(), a.second > b.second) of libstdc++
// (__heap_select + __sort_heap, bits/stl_algo.h) over (function, sum) pairs fed in vec order,
// keeping what the reference reads afterwards: vec[0], vec[1] and whatever is left in vec[2].
// A pop_heap of __heap_select writes the old top to the position being examined and nowhere
// else, so vec[2] is final once the third element has been seen.
struct BestPair {
    uint16_t fi;
    int32_t sum;
};
struct BestTop {
    BestPair h[2];  // the two-element heap under `gt` once n >= 2
    BestPair third;
    uint32_t n = 0;
    struct Gt {
        SKM_HD bool operator()(BestPair a, BestPair b) const { return a.sum > b.sum; }
    };
    SKM_HD void push(BestPair x) {
        const Gt gt;
        if (n < 2) {
            h[n] = x;
            if (n == 1) stl_adjust_heap(h, 0, 2, h[0], gt);  // make_heap(first, first + 2)
        } else {
            BestPair left = x;
            if (gt(x, h[0])) {  // pop_heap(first, middle, i)
                left = h[0];
                stl_adjust_heap(h, 0, 2, x, gt);
            }
            if (n == 2) third = left;
        }
        ++n;
    }
    // vec[0], vec[1] after sort_heap(first, first + 2): one pop_heap, which swaps the two
    SKM_HD BestPair v0() const { return n >= 2 ? h[1] : h[0]; }
    SKM_HD BestPair v1() const { return h[0]; }
    SKM_HD BestPair v2() const { return third; }
};

// regex_match of "^W?A[A|W]*W[B|W]*BW?" as fusion_pattern (skm_host.cpp) runs it: a set of states
// 0 start, 1 before A, 2 in [A|W]*, 3 in [B|W]*, 4 after B, 5 after the last W; bit s = state s.
SKM_HD inline uint32_t best_nfa_step(uint32_t cur, char c) {
    uint32_t nxt = 0;
    if ((cur & 1u) && c == 'W') nxt |= 2u;
    if ((cur & 2u) && c == 'A') nxt |= 4u;
    if (cur & 4u) {
        if (c == 'A' || c == 'W') nxt |= 4u;
        if (c == 'W') nxt |= 8u;
    }
    if (cur & 8u) {
        if (c == 'B' || c == 'W') nxt |= 8u;
        if (c == 'B') nxt |= 16u;
    }
    if ((cur & 16u) && c == 'W') nxt |= 32u;
    return nxt;
}

// One sequence: calls[0, n) in call order, work[0, n) scratch for the collapsed and merged lists
// (both built in place: each write position is at or before every later read).  Returns false
// with SKM_BEST_DEFERRED in out->flags when the sequence is left to skm_find_best_call: more than
// SKM_BEST_MAX_CALLS calls, or a call that names a complex function.  Nothing else defers.
SKM_HD inline bool best_call_one(const skm_kmer_call* calls, uint64_t n, skm_kmer_call* work, const BestTables& tb,
                                 skm_best_call* out) {
    skm_best_call r;
    r.fi = SKM_UNDEFINED_FUNCTION;
    r.fi_a = r.fi_b = SKM_UNDEFINED_FUNCTION;
    r.flags = 0;
    r.score = r.offset = 0.0f;
    if (n == 0) {
        *out = r;
        return true;
    }
    if (n > SKM_BEST_MAX_CALLS) {
        r.flags = SKM_BEST_DEFERRED;
        *out = r;
        return false;
    }
    // 1. collapse runs of the same function (end and count accumulate)
    uint32_t nc = 0;
    for (uint32_t i = 0; i < (uint32_t)n; ++i) {
        const skm_kmer_call c = calls[i];
        if (best_func(tb, c.function_index).nparts == SKM_BEST_COMPLEX) {
            r.flags = SKM_BEST_DEFERRED;
            *out = r;
            return false;
        }
        if (nc && work[nc - 1].function_index == c.function_index) {
            work[nc - 1].end = c.end;
            work[nc - 1].count += c.count;
        } else {
            work[nc++] = c;
        }
    }
    // 2. F1 F2 F1 with F2.count < 5 and F1 + F1 >= 10: drop F2, merge the F1s
    uint32_t nm = 0;
    for (uint32_t i = 0; i < nc;) {
        skm_kmer_call cur = work[i];
        uint32_t j = i + 1;
        while (j + 1 < nc && cur.function_index == work[j + 1].function_index && work[j].count < 5 &&
               cur.count + work[j + 1].count >= 10) {
            cur.end = work[j + 1].end;
            cur.count += work[j + 1].count;
            j += 2;
        }
        work[nm++] = cur;
        i = j;
    }
    // 3. fusion calls.  Part keys are handed out 'A', 'B', ... in order of first appearance and
    // fusion keys 'W', 'X', ...; the pattern needs every key of exp to be A, B or W (with at most
    // SKM_BEST_MAX_PARTS parts per name no part key reaches 'W' and no key reaches '|' before
    // another key has already failed the match), so the tables are followed up to the first other
    // key only: at most one fusion string and 2 + 2 * SKM_BEST_MAX_PARTS part keys.
    if (nm > 1) {
        constexpr uint32_t KCAP = 2 + 2 * SKM_BEST_MAX_PARTS;
        uint32_t kid[KCAP];
        uint32_t nk = 0;
        uint64_t fusion0 = 0;  // the key string that got 'W': one byte (key index + 1) per part
        uint32_t acc_n[3] = {0, 0, 0};
        float acc_sum[3] = {0.0f, 0.0f, 0.0f};  // accumulator_set<float, mean> of A, B, W
        uint16_t w_fi = SKM_UNDEFINED_FUNCTION;
        uint32_t st = 3u;  // state 0 and, past the optional W, state 1
        bool ok = true;
        int32_t sum_scores = 0;
        for (uint32_t i = 0; i < nm; ++i) sum_scores += work[i].count;
        for (uint32_t i = 0; i < nm && ok; ++i) {
            const skm_kmer_call c = work[i];
            const BestFunc& f = best_func(tb, c.function_index);
            auto key_of = [&](uint32_t id, bool insert) -> uint32_t {
                for (uint32_t k = 0; k < nk; ++k)
                    if (kid[k] == id) return k;
                if (!insert || nk == KCAP) return KCAP;
                kid[nk] = id;
                return nk++;
            };
            uint64_t fk = 0;
            for (uint32_t p = 0; p < f.nparts; ++p) {
                const uint32_t k = key_of(f.parts[p], true);
                if (k == KCAP) ok = false;
                fk = fk << 8 | (k + 1);
            }
            int slot;  // 0 A, 1 B, 2 W
            if (f.nparts > 1) {
                if (!fusion0) fusion0 = fk;
                if (fk != fusion0) ok = false;  // a second fusion string: 'X'
                slot = 2;
            } else {
                const uint32_t k = key_of(f.whole, false);  // operator[] on a missing name gives '\0'
                if (k > 1) ok = false;
                slot = (int)k;
            }
            if (!ok) break;
            st = best_nfa_step(st, slot == 0 ? 'A' : slot == 1 ? 'B' : 'W');
            if (!st) ok = false;
            acc_n[slot] += 1;
            acc_sum[slot] += (float)c.protein_length_median;
            if (slot == 2) w_fi = c.function_index;
        }
        if (ok && (st & 48u)) {
            const float a_mean = acc_sum[0] / (float)acc_n[0], b_mean = acc_sum[1] / (float)acc_n[1];
            const float w_mean = acc_sum[2] / (float)acc_n[2];
            const float diff = (a_mean + b_mean) - w_mean;
            const float frac_dif = (diff < 0.0f ? -diff : diff) / w_mean;
            if ((double)frac_dif < 0.1) {
                r.fi = w_fi;
                r.score = (float)sum_scores;
                *out = r;
                return true;
            }
        }
    }
    // 4. per-function sums in ascending function index, top two by partial_sort
    BestTop top;
    for (int32_t prev = -1;;) {
        int32_t next = 0x10000;
        for (uint32_t i = 0; i < nm; ++i) {
            const int32_t f = work[i].function_index;
            if (f > prev && f < next) next = f;
        }
        if (next == 0x10000) break;
        BestPair x;
        x.fi = (uint16_t)next;
        x.sum = 0;
        for (uint32_t i = 0; i < nm; ++i)
            if (work[i].function_index == next) x.sum += work[i].count;
        top.push(x);
        prev = next;
    }
    const BestPair v0 = top.v0(), v1 = top.v1();
    r.offset = top.n == 1 ? (float)v0.sum : (float)(v0.sum - v1.sum);
    if (r.offset >= 5.0f) {
        r.fi = v0.fi;
        r.score = (float)v0.sum;
    } else if (top.n >= 2) {
        uint16_t f1 = v0.fi, f2 = v1.fi;
        if (best_func(tb, f2).rank > best_func(tb, f1).rank) {
            const uint16_t t = f1;
            f1 = f2;
            f2 = t;
        }
        bool pair = top.n == 2;
        if (!pair) {
            const float pair_offset = (float)(v1.sum - top.v2().sum);
            if (pair_offset > 2.0f) {
                pair = true;
                r.offset = pair_offset;
            }
        }
        if (pair) {
            r.flags = SKM_BEST_PAIR;
            r.fi_a = f1;
            r.fi_b = f2;
            r.score = (float)v0.sum;
        }
    }
    *out = r;
    return true;
}

}  // namespace skm
