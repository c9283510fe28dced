// The final.kmers line formatter (csrc/skm_finalkmers.h) against snprintf, for every u16 in each
// column.  Every line is written into a heap block of exactly fk_line_len bytes, so a build with
// -fsanitize=address,undefined reports any byte written past the length the formatter announced.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>

#include "skm_finalkmers.h"

int main() {
    uint64_t lines = 0, bad = 0, bytes = 0;
    const unsigned char kb[8] = {'a', 'C', 0x80, 0xFF, 0, '\t', '\n', 'Y'};
    uint64_t key;
    std::memcpy(&key, kb, 8);  // (little-endian hosts: byte 0 first, as the key holds a k-mer)
    auto check = [&](uint32_t avg, uint32_t fi) {
        char want[64];
        std::memcpy(want, kb, 8);
        const int w = 8 + std::snprintf(want + 8, sizeof(want) - 8, "\t%u\t%u\t\n", avg, fi);
        const uint32_t len = skm::fk_line_len(avg, fi);
        std::unique_ptr<uint8_t[]> got(new uint8_t[len]);
        const uint32_t wrote = skm::fk_write_line(got.get(), key, avg, fi);
        ++lines;
        bytes += len;
        if (len != (uint32_t)w || wrote != len || std::memcmp(got.get(), want, len) != 0 || len < skm::FK_MIN_LINE ||
            len > skm::FK_MAX_LINE)
            ++bad;
    };
    for (uint32_t v = 0; v < 65536; ++v) {
        check(v, (v * 2654435761u) >> 16);
        check((v * 40503u) & 0xFFFFu, v);
    }
    for (uint32_t a : {0u, 9u, 10u, 99u, 100u, 999u, 1000u, 9999u, 10000u, 65535u})
        for (uint32_t f : {0u, 9u, 10u, 99u, 100u, 999u, 1000u, 9999u, 10000u, 65535u}) check(a, f);
    std::printf("lines %llu bytes %llu bad %llu\n", (unsigned long long)lines, (unsigned long long)bytes,
                (unsigned long long)bad);
    return bad ? 1 : 0;
}
