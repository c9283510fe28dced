// The recall pass's batch cut rule (csrc/skm_recallplan.h) over random length vectors against a
// naive loop that decides sequence by sequence.  The lengths live in a heap block of exactly n
// entries, so a build with -fsanitize=address,undefined reports any read past the range.
#include <cstdint>
#include <cstdio>
#include <memory>
#include <random>
#include <vector>

#include "skm_recallplan.h"

int main() {
    std::mt19937_64 rng(12345);
    uint64_t cases = 0, batches = 0, bad = 0;
    for (int it = 0; it < 4000; ++it) {
        const uint64_t n = rng() % 40;
        std::unique_ptr<uint32_t[]> len(new uint32_t[n ? n : 1]);
        for (uint64_t s = 0; s < n; ++s) {
            const uint64_t k = rng() % 8;
            len[s] = k == 0 ? 0 : k == 1 ? (uint32_t)(rng() % 2000) : (uint32_t)(rng() % 40);
        }
        const uint64_t pick[] = {0, 1, 2, 15, 16, 17, 41, 100, 4096, 1ull << 29, 1ull << 40};
        const uint64_t B = pick[rng() % (sizeof(pick) / sizeof(pick[0]))];
        const uint64_t first = rng() % (n + 1);
        uint64_t cnt = rng() % 3 == 0 ? 0 : rng() % (n - first + 1);
        std::vector<skm::RecallBatch> plan;
        const uint32_t* lp = len.get();
        const bool ok = skm::recall_plan([lp](uint64_t s) { return lp[s]; }, n, B, first, cnt, plan);
        ++cases;
        if (!ok) {
            ++bad;
            continue;
        }
        // the naive rule: walk the sequences, close the batch when the next one does not fit
        const uint64_t lim = B == 0 ? (1ull << 29) : (B > (1ull << 31) ? (1ull << 31) : B);
        const uint64_t stop = cnt ? first + cnt : n;
        uint64_t p = 0;
        for (uint64_t s = 0; s < first; ++s) p += (uint64_t)len[s] + 1;
        std::vector<skm::RecallBatch> want;
        uint64_t bytes = 0;
        for (uint64_t s = first; s < stop; ++s) {
            const uint64_t add = (uint64_t)len[s] + 1;
            if (want.empty() || bytes + add > lim) {
                want.push_back(skm::RecallBatch{s, 0, p & ~15ull, p, p, 0});
                bytes = 0;
            }
            skm::RecallBatch& b = want.back();
            bytes += add;
            p += add;
            ++b.n;
            b.end = p;
            b.windows += len[s] >= 8 ? len[s] - 7 : 0;
        }
        batches += plan.size();
        if (plan.size() != want.size()) {
            ++bad;
            continue;
        }
        for (size_t i = 0; i < plan.size(); ++i) {
            const skm::RecallBatch &a = plan[i], &w = want[i];
            if (a.first != w.first || a.n != w.n || a.base != w.base || a.pstart != w.pstart || a.end != w.end ||
                a.windows != w.windows)
                ++bad;
        }
    }
    // ranges outside the sequences are refused
    std::vector<skm::RecallBatch> plan;
    const uint32_t three[3] = {5, 6, 7};
    auto at = [&](uint64_t s) { return three[s]; };
    if (skm::recall_plan(at, 3, 0, 4, 0, plan)) ++bad;
    if (skm::recall_plan(at, 3, 0, 1, 3, plan)) ++bad;
    if (!skm::recall_plan(at, 3, 0, 3, 0, plan) || !plan.empty()) ++bad;
    std::printf("cases %llu batches %llu bad %llu\n", (unsigned long long)cases, (unsigned long long)batches,
                (unsigned long long)bad);
    return bad ? 1 : 0;
}
