// skm_finalkmers.h -- one line of final.kmers (kmers-build-signatures.cc:212-216), the same code on
// the host and in the device formatter (skm_output.hip: k_fk_len, k_fk_emit):
//
//   KMER '\t' avg_from_end '\t' function_index '\t' '\n'
//
// KMER is the 8 key bytes as the little-endian u64 holds them, byte 0 first, copied and never
// validated; the two u16 print as decimals without leading zeros (0 prints as "0").  A line is
// 12 + ndig(avg_from_end) + ndig(function_index) bytes: 14 .. 22.  Integer-only, no tables, no
// local arrays (the device copy must not touch scratch memory).  Plain C++: a host program may
// include this header without HIP.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SKM_FK_HD __host__ __device__ __forceinline__
#else
#define SKM_FK_HD inline
#endif

namespace skm {

constexpr uint32_t FK_MIN_LINE = 14, FK_MAX_LINE = 22;

SKM_FK_HD uint32_t fk_ndig(uint32_t v) {  // decimal digits of a u16
    return v < 10u ? 1u : v < 100u ? 2u : v < 1000u ? 3u : v < 10000u ? 4u : 5u;
}

SKM_FK_HD uint32_t fk_line_len(uint32_t avg_from_end, uint32_t function_index) {
    return 12u + fk_ndig(avg_from_end) + fk_ndig(function_index);
}

SKM_FK_HD uint32_t fk_put_dec(uint8_t* p, uint32_t v) {  // the digits written
    const uint32_t nd = fk_ndig(v);
    for (uint32_t i = nd; i-- > 0;) {
        p[i] = (uint8_t)('0' + v % 10u);
        v /= 10u;
    }
    return nd;
}

// writes fk_line_len(avg_from_end, function_index) bytes at p and returns that length
SKM_FK_HD uint32_t fk_write_line(uint8_t* p, uint64_t key, uint32_t avg_from_end, uint32_t function_index) {
    for (int j = 0; j < 8; ++j) p[j] = (uint8_t)(key >> (8 * j));
    p[8] = '\t';
    uint32_t o = 9;
    o += fk_put_dec(p + o, avg_from_end);
    p[o++] = '\t';
    o += fk_put_dec(p + o, function_index);
    p[o++] = '\t';
    p[o++] = '\n';
    return o;
}

}  // namespace skm
