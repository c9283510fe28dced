// skm_recallplan.h -- the batch cut rule of skm_build_recall (the recall pass over a build's
// resident sequences, kmers-build-signatures.cc:266-349).  Host only, no HIP: the library
// (skm_build.hip), the host entry point skm_recall_plan and tests/native/recallplan_check.cpp share
// this one definition.
//
// The resident sequences lie packed: sequence s at pstart(s) = sum over t < s of (len[t] + 1), one
// 0 byte after each.  A batch is a run of whole sequences whose packed bytes (len + 1 each) do not
// exceed batch_residues; a sequence that alone exceeds it is a batch of its own.  The cuts are
// greedy from the range's first sequence, so they depend on the range as well as on the lengths.
// A batch's view of the residue buffer starts at base = pstart(its first sequence) & ~15 -- the
// lookup kernel loads aligned 16-byte units and indexes its hits by residue position -- and ends
// after its last sequence's separator.
#pragma once
#include <cstdint>
#include <vector>

namespace skm {

// 2^29 packed bytes: about 7 B of query scratch per residue (4 B hits, 2 B per window, the
// per-sequence tables), so under 4 GB a batch.  A plan from that arithmetic, not a measured optimum.
constexpr uint64_t RECALL_DEFAULT_BATCH = 1ull << 29;
// a batch's positions and sequences stay 32-bit counts: larger values are taken as this one
constexpr uint64_t RECALL_MAX_BATCH = 1ull << 31;

struct RecallBatch {
    uint64_t first, n;     // sequences [first, first + n)
    uint64_t base;         // pstart(first) & ~15: where the batch's view of the residues starts
    uint64_t pstart, end;  // pstart(first); pstart(first + n - 1) + len + 1
    uint64_t windows;      // sum of (len >= 8 ? len - 7 : 0)
};

// the range [first, first + n) of n_total sequences, n == 0 meaning "to the end"; false if it does
// not lie inside them
inline bool recall_range(uint64_t n_total, uint64_t first, uint64_t& n) {
    if (first > n_total) return false;
    if (n == 0) n = n_total - first;
    return n <= n_total - first;
}

// len_at(s) = length of sequence s, 0 <= s < n_total.  Returns false for a range outside them.
template <class LenAt>
inline bool recall_plan(LenAt len_at, uint64_t n_total, uint64_t batch_residues, uint64_t first, uint64_t n,
                        std::vector<RecallBatch>& out) {
    out.clear();
    if (!recall_range(n_total, first, n)) return false;
    uint64_t B = batch_residues ? batch_residues : RECALL_DEFAULT_BATCH;
    if (B > RECALL_MAX_BATCH) B = RECALL_MAX_BATCH;
    uint64_t p = 0;
    for (uint64_t s = 0; s < first; ++s) p += (uint64_t)len_at(s) + 1;
    const uint64_t stop = first + n;
    for (uint64_t s = first; s < stop;) {
        RecallBatch b{s, 0, p & ~15ull, p, p, 0};
        uint64_t bytes = 0;
        while (s < stop) {
            const uint64_t len = len_at(s), add = len + 1;
            if (b.n && bytes + add > B) break;
            bytes += add;
            b.windows += len >= 8 ? len - 7 : 0;
            ++b.n;
            ++s;
            if (bytes >= B) break;
        }
        p += bytes;
        b.end = p;
        out.push_back(b);
    }
    return true;
}

}  // namespace skm
