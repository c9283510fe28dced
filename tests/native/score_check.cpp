// Prints md_score_text (front/skm_mdbatch.h: the score column of kmers-matrix-distance-folder /
// -merge) for "count len1 len2" triples given as arguments, one result per line.
#include <cstdio>
#include <cstdlib>

#include "front/skm_mdbatch.h"

int main(int argc, char** argv) {
    for (int i = 1; i + 2 < argc; i += 3) {
        const unsigned long c = std::strtoul(argv[i], nullptr, 10);
        const unsigned long long a = std::strtoull(argv[i + 1], nullptr, 10), b = std::strtoull(argv[i + 2], nullptr, 10);
        std::printf("%s\n", skmf::md_score_text((uint32_t)c, (size_t)a, (size_t)b).c_str());
    }
    return 0;
}
