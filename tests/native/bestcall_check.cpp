// bestcall_check.cpp -- csrc/skm_bestcall.h's BestTop (the streamed restatement of
// std::partial_sort(first, first + 2, last) and of what it leaves at first + 2) against
// std::partial_sort itself, on tie-heavy vectors of 1-12 (function, sum) pairs in ascending
// function index, as find_best_call builds them from its std::map.  Also one pass of best_call_one
// over random call lists, so that a sanitizer build walks the whole core.
//   bestcall_check [n_vectors]   -> "vectors N bad 0", exit status 0 when nothing differs
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <utility>
#include <vector>

#include "skm_bestcall.h"

int main(int argc, char** argv) {
    const long nvec = argc > 1 ? std::atol(argv[1]) : 1000000;
    std::mt19937_64 rng(12345);
    long bad = 0;
    for (long it = 0; it < nvec; ++it) {
        const int n = 1 + (int)(rng() % 12);
        const int spread = 1 + (int)(rng() % 4);  // 1-4 distinct sums: ties everywhere
        const int base = (int)(rng() % 30);
        std::vector<std::pair<uint16_t, int>> vec;
        uint16_t fi = (uint16_t)(rng() % 5);
        for (int k = 0; k < n; ++k) {
            vec.emplace_back(fi, base + (int)(rng() % spread));
            fi = (uint16_t)(fi + 1 + rng() % 3);
        }
        skm::BestTop top;
        for (const auto& p : vec) top.push(skm::BestPair{p.first, p.second});
        if (vec.size() > 1)
            std::partial_sort(vec.begin(), vec.begin() + 2, vec.end(),
                              [](const std::pair<uint16_t, int>& a, const std::pair<uint16_t, int>& b) {
                                  return a.second > b.second;
                              });
        auto same = [](skm::BestPair a, const std::pair<uint16_t, int>& b) { return a.fi == b.first && a.sum == b.second; };
        bool ok = top.n == vec.size() && same(top.v0(), vec[0]);
        if (vec.size() > 1) ok = ok && same(top.v1(), vec[1]);
        if (vec.size() > 2) ok = ok && same(top.v2(), vec[2]);
        if (!ok && bad++ < 5) std::printf("differs at vector %ld (n = %d)\n", it, n);
    }
    // the whole core once over random lists (names: 0 and 1 single, 2 = "0 / 1", 3 = nine parts)
    std::vector<skm::BestFunc> ent(5);
    for (uint32_t f = 0; f < 5; ++f) {
        ent[f].rank = f == 4 ? 0 : f + 1;
        ent[f].whole = f;
        ent[f].nparts = 1;
        ent[f].parts[0] = f;
    }
    ent[2].nparts = 2;
    ent[2].parts[0] = 0;
    ent[2].parts[1] = 1;
    ent[3].nparts = skm::SKM_BEST_COMPLEX;
    const skm::BestTables tb{ent.data(), 4};
    unsigned long long sum = 0, deferred = 0;
    for (long it = 0; it < nvec / 10; ++it) {
        const uint64_t n = rng() % 70;
        std::vector<skm_kmer_call> calls(n), work(n);
        for (auto& c : calls) {
            c = skm_kmer_call{};
            c.function_index = (uint16_t)(rng() % 40 ? rng() % 3 : rng() % 6);
            c.count = 1 + (int)(rng() % 9);
            c.protein_length_median = 100 + (uint32_t)(rng() % 900);
        }
        skm_best_call r;
        if (!skm::best_call_one(calls.data(), n, work.data(), tb, &r)) ++deferred;
        sum += r.fi + (unsigned long long)r.score;
    }
    std::printf("vectors %ld bad %ld (core checksum %llu, deferred %llu)\n", nvec, bad, sum, deferred);
    return bad ? 1 : 0;
}
