// skm_fasta.hip -- FastaParser on the device (fasta_parser.h:38-144, fasta_parser.cc:17-36, as
// parse_fasta_impl in front/skm_front.cpp restates it): the raw bytes of a set of files in, the
// packed residues, QMeta and window offsets of a resident annotate query out (what
// FunctionCaller::process_fasta_stream, call_functions.tcc:217-255, hands to process_aa_seq).
//
// The parser is a byte transducer, so it is an associative scan over transition maps.  "This record
// is kept" (its id is not empty) is folded into the automaton, which gives nine states and no
// look-ahead; a map is 9 x 4 bits in one u64.  Every thread owns one 16-byte load; maps are scanned
// in the wave by shuffles, in the workgroup through LDS, and across workgroup tiles by a launch of
// its own -- no workgroup ever waits for another one inside a launch:
//   k_fasta_maps      per tile: the composition of its bytes' maps
//   k_fasta_map_scan  one workgroup: every tile's entry state
//   k_fasta_count     per tile: kept residues and kept records (entry states now known)
//   k_fasta_sum_scan  one workgroup: exclusive sums of the two counts, and the totals
//   k_fasta_emit      per tile: residues and separators staged in LDS and stored as one contiguous
//                     range; per record its packed start and the position of its '>'; per file its
//                     first record
//   k_fasta_meta      per record: QMeta, seq_len, windows (then Scanner for the window offsets)
// A file start resets the state to START (a constant map), which is all a file boundary means to
// the residues; a record is counted where its id gets its first byte (ID0 -> ID), so a record end
// (the next '>' or the end of the file, parse_complete()) needs no event of its own: record s ends
// where record s + 1 starts in the packed buffer.
#include "skm_fasta.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace skm {

namespace {

// states; *K = of a kept record, *D = of a record with an empty id (dropped with its residues)
enum : uint32_t { F_START, F_ID0, F_ID, F_DEFK, F_DEFD, F_DATAK, F_DATAD, F_IODK, F_IODD, F_NSTATE };

constexpr uint64_t fmap(uint64_t s0, uint64_t s1, uint64_t s2, uint64_t s3, uint64_t s4, uint64_t s5, uint64_t s6,
                        uint64_t s7, uint64_t s8) {
    return s0 | s1 << 4 | s2 << 8 | s3 << 12 | s4 << 16 | s5 << 20 | s6 << 24 | s7 << 28 | s8 << 32;
}
// next state per byte class, indexed START ID0 ID DEFK DEFD DATAK DATAD IODK IODD.  A byte the host
// parser reports as an error changes no state.
constexpr uint64_t M_IDENT = fmap(F_START, F_ID0, F_ID, F_DEFK, F_DEFD, F_DATAK, F_DATAD, F_IODK, F_IODD);  // '\r'
constexpr uint64_t M_GT = fmap(F_ID0, F_ID, F_ID, F_DEFK, F_DEFD, F_DATAK, F_DATAD, F_ID0, F_ID0);
constexpr uint64_t M_BLANK = fmap(F_START, F_DEFD, F_DEFK, F_DEFK, F_DEFD, F_DATAK, F_DATAD, F_IODK, F_IODD);
constexpr uint64_t M_NL = fmap(F_START, F_DATAD, F_DATAK, F_DATAK, F_DATAD, F_IODK, F_IODD, F_IODK, F_IODD);
constexpr uint64_t M_ALPHA = fmap(F_START, F_ID, F_ID, F_DEFK, F_DEFD, F_DATAK, F_DATAD, F_DATAK, F_DATAD);
constexpr uint64_t M_OTHER = fmap(F_START, F_ID, F_ID, F_DEFK, F_DEFD, F_DATAK, F_DATAD, F_IODK, F_IODD);  // '*' too
constexpr uint64_t M_RESET = 0;  // a file start: every state to START

__device__ __forceinline__ bool is_alpha(uint32_t c) { return ((c | 0x20u) - 'a') < 26u; }  // false for c >= 0x80

__device__ __forceinline__ uint64_t byte_map(uint32_t c) {
    return c == '\r' ? M_IDENT
           : c == '>' ? M_GT
           : c == '\n' ? M_NL
           : (c == ' ' || c == '\t') ? M_BLANK
           : is_alpha(c) ? M_ALPHA
                         : M_OTHER;
}
__device__ __forceinline__ uint32_t map_apply(uint64_t m, uint32_t s) { return (uint32_t)(m >> (4 * s)) & 15u; }
// a, then b
__device__ __forceinline__ uint64_t map_compose(uint64_t a, uint64_t b) {
    uint64_t r = 0;
#pragma unroll
    for (uint32_t s = 0; s < F_NSTATE; ++s) r |= (uint64_t)map_apply(b, map_apply(a, s)) << (4 * s);
    return r;
}
__device__ __forceinline__ uint32_t byte_of(const uint4& v, int j) {
    const uint32_t w = j < 4 ? v.x : j < 8 ? v.y : j < 12 ? v.z : v.w;
    return (w >> (8 * (j & 3))) & 255u;
}

// first f in [lo, hi) with file_off[f] >= x (hi when there is none)
__device__ __forceinline__ uint64_t first_file_at(const uint64_t* __restrict__ file_off, uint64_t lo, uint64_t hi,
                                                  uint64_t x) {
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (file_off[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The files that start inside the workgroup's tile [t0, t0 + FA_TILE) and before n: [s_f[0], s_f[1]),
// found once per tile (most tiles hold no file start).  Returns the calling thread's first file
// starting at or after its byte b, and that file's start in nxt (~0 when there is none).
__device__ __forceinline__ uint64_t thread_first_file(const uint64_t* __restrict__ file_off, uint64_t n_files, uint64_t n,
                                                      uint64_t t0, uint64_t b, uint64_t* s_f, uint64_t& fhi,
                                                      uint64_t& nxt) {
    if (threadIdx.x == 0) {
        s_f[0] = first_file_at(file_off, 0, n_files, t0);
        s_f[1] = first_file_at(file_off, s_f[0], n_files, t0 + FA_TILE < n ? t0 + FA_TILE : n);
    }
    __syncthreads();
    const uint64_t flo = s_f[0];
    fhi = s_f[1];
    uint64_t f = fhi;
    nxt = ~0ull;
    if (flo < fhi) {
        f = first_file_at(file_off, flo, fhi, b);
        if (f < fhi) nxt = file_off[f];
    }
    return f;
}

// the composition of the maps of a thread's 16 bytes [b, b + 16)
__device__ __forceinline__ uint64_t thread_map(const uint4& v, uint64_t b, const uint64_t* __restrict__ file_off,
                                               uint64_t f, uint64_t fhi, uint64_t nxt) {
    uint64_t m = M_IDENT;
#pragma unroll
    for (int j = 0; j < (int)FA_BYTES; ++j) {
        if (b + j == nxt) {
            m = M_RESET;
            do {  // empty files start here too
                ++f;
                nxt = f < fhi ? file_off[f] : ~0ull;
            } while (nxt == b + j);
        }
        m = map_compose(m, byte_map(byte_of(v, j)));
    }
    return m;
}

// Workgroup scan of the threads' maps (FA_THREADS threads): returns the composition of the maps of
// the threads before the caller; s_w[FA_THREADS / 64] holds the tile's whole map after it.
__device__ __forceinline__ uint64_t block_excl_map(uint64_t m, uint64_t* s_w) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t x = m;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t y = __shfl_up(x, d, 64);
        if (lane >= d) x = map_compose(y, x);
    }
    if (lane == 63) s_w[wave] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t acc = M_IDENT;
        for (int w = 0; w < (int)FA_THREADS / 64; ++w) {
            const uint64_t t = s_w[w];
            s_w[w] = acc;
            acc = map_compose(acc, t);
        }
        s_w[FA_THREADS / 64] = acc;
    }
    __syncthreads();
    uint64_t e = __shfl_up(x, 1, 64);
    if (lane == 0) e = M_IDENT;
    return map_compose(s_w[wave], e);
}

__global__ __launch_bounds__(FA_THREADS) void k_fasta_maps(const uint8_t* __restrict__ raw, uint64_t n,
                                                           const uint64_t* __restrict__ file_off, uint64_t n_files,
                                                           uint64_t* __restrict__ tile_map) {
    __shared__ uint64_t s_f[2], s_w[FA_THREADS / 64 + 1];
    const uint64_t t0 = (uint64_t)blockIdx.x * FA_TILE, b = t0 + (uint64_t)threadIdx.x * FA_BYTES;
    const uint4 v = *reinterpret_cast<const uint4*>(raw + b);
    uint64_t fhi, nxt;
    const uint64_t f = thread_first_file(file_off, n_files, n, t0, b, s_f, fhi, nxt);
    (void)block_excl_map(thread_map(v, b, file_off, f, fhi, nxt), s_w);
    if (threadIdx.x == 0) tile_map[blockIdx.x] = s_w[FA_THREADS / 64];
}

// one workgroup of 1024: tile_map[t] := the state the parser is in before tile t's first byte
__global__ __launch_bounds__(1024) void k_fasta_map_scan(uint64_t* __restrict__ tile_map, uint64_t nt) {
    __shared__ uint64_t s_w[17];
    uint32_t carry = F_START;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint64_t c0 = 0; c0 < nt; c0 += 1024) {
        const uint64_t i = c0 + threadIdx.x;
        uint64_t x = i < nt ? tile_map[i] : M_IDENT;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t y = __shfl_up(x, d, 64);
            if (lane >= d) x = map_compose(y, x);
        }
        if (lane == 63) s_w[wave] = x;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint64_t acc = M_IDENT;
            for (int w = 0; w < 16; ++w) {
                const uint64_t t = s_w[w];
                s_w[w] = acc;
                acc = map_compose(acc, t);
            }
            s_w[16] = acc;
        }
        __syncthreads();
        uint64_t e = __shfl_up(x, 1, 64);
        if (lane == 0) e = M_IDENT;
        if (i < nt) tile_map[i] = map_apply(map_compose(s_w[wave], e), carry);
        carry = map_apply(s_w[16], carry);
        __syncthreads();
    }
}

// one byte of the transducer: c in state s -> the next state; res = c is a kept residue, start = a
// kept record starts here (its id gets its first byte)
__device__ __forceinline__ uint32_t fasta_step(uint32_t s, uint32_t c, bool& res, bool& start) {
    const bool al = is_alpha(c);
    res = (s == F_DATAK && (al || c == '*')) || (s == F_IODK && al);
    const uint32_t t = map_apply(byte_map(c), s);
    start = s == F_ID0 && t == F_ID;
    return t;
}

__global__ __launch_bounds__(FA_THREADS) void k_fasta_count(const uint8_t* __restrict__ raw, uint64_t n,
                                                            const uint64_t* __restrict__ file_off, uint64_t n_files,
                                                            const uint64_t* __restrict__ tile_state,
                                                            uint64_t* __restrict__ tile_cnt) {
    __shared__ uint64_t s_f[2], s_w[FA_THREADS / 64 + 1];
    __shared__ uint32_t s_c[FA_THREADS / 64];
    const uint64_t t0 = (uint64_t)blockIdx.x * FA_TILE, b = t0 + (uint64_t)threadIdx.x * FA_BYTES;
    const uint4 v = *reinterpret_cast<const uint4*>(raw + b);
    uint64_t fhi, nxt;
    uint64_t f = thread_first_file(file_off, n_files, n, t0, b, s_f, fhi, nxt);
    const uint64_t e = block_excl_map(thread_map(v, b, file_off, f, fhi, nxt), s_w);
    uint32_t s = map_apply(e, (uint32_t)tile_state[blockIdx.x]);
    uint32_t cnt = 0;  // residues | records << 16 (a tile holds at most FA_TILE of either)
#pragma unroll
    for (int j = 0; j < (int)FA_BYTES; ++j) {
        if (b + j == nxt) {
            s = F_START;
            do {
                ++f;
                nxt = f < fhi ? file_off[f] : ~0ull;
            } while (nxt == b + j);
        }
        bool res, start;
        s = fasta_step(s, byte_of(v, j), res, start);
        cnt += (res ? 1u : 0u) + (start ? 0x10000u : 0u);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_down(cnt, d, 64);
    if ((threadIdx.x & 63) == 0) s_c[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < (int)FA_THREADS / 64; ++w) t += s_c[w];
        tile_cnt[2 * (uint64_t)blockIdx.x] = t & 0xFFFFu;
        tile_cnt[2 * (uint64_t)blockIdx.x + 1] = t >> 16;
    }
}

// one workgroup of 1024: cnt[2t], cnt[2t + 1] := their exclusive sums over the tiles; the totals
// go to cnt[2 nt], cnt[2 nt + 1]
__global__ __launch_bounds__(1024) void k_fasta_sum_scan(uint64_t* __restrict__ cnt, uint64_t nt) {
    __shared__ uint64_t s_a[17], s_b[17];
    uint64_t ca = 0, cb = 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint64_t c0 = 0; c0 < nt; c0 += 1024) {
        const uint64_t i = c0 + threadIdx.x;
        const uint64_t va = i < nt ? cnt[2 * i] : 0, vb = i < nt ? cnt[2 * i + 1] : 0;
        uint64_t xa = va, xb = vb;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t ya = __shfl_up(xa, d, 64), yb = __shfl_up(xb, d, 64);
            if (lane >= d) {
                xa += ya;
                xb += yb;
            }
        }
        if (lane == 63) {
            s_a[wave] = xa;
            s_b[wave] = xb;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint64_t aa = 0, ab = 0;
            for (int w = 0; w < 16; ++w) {
                const uint64_t ta = s_a[w], tb = s_b[w];
                s_a[w] = aa;
                s_b[w] = ab;
                aa += ta;
                ab += tb;
            }
            s_a[16] = aa;
            s_b[16] = ab;
        }
        __syncthreads();
        if (i < nt) {
            cnt[2 * i] = ca + s_a[wave] + xa - va;
            cnt[2 * i + 1] = cb + s_b[wave] + xb - vb;
        }
        ca += s_a[16];
        cb += s_b[16];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        cnt[2 * nt] = ca;
        cnt[2 * nt + 1] = cb;
    }
}

// With R(p), S(p) = the kept residues and kept record starts before byte p, a residue at p goes to
// res[R(p) + S(p) - 1] and a record start at p (record s = S(p), pstart[s] = R(p) + S(p)) puts the 0
// that ends record s - 1 at the same expression: every event takes the next output byte, so a
// tile's output is one contiguous range, staged in LDS and stored coalesced.  (The first record
// start of all has no record to end: position -1, not stored.  The 0 after the last record is the
// host's tail memset.)
__global__ __launch_bounds__(FA_THREADS) void k_fasta_emit(const uint8_t* __restrict__ raw, uint64_t n,
                                                           const uint64_t* __restrict__ file_off, uint64_t n_files,
                                                           const uint64_t* __restrict__ tile_state,
                                                           const uint64_t* __restrict__ tile_cnt, uint8_t* __restrict__ res,
                                                           uint64_t* __restrict__ pstart, uint64_t* __restrict__ hdr_pos,
                                                           uint64_t* __restrict__ file_rec, uint64_t n_recs, uint64_t rp) {
    __shared__ uint64_t s_f[2], s_w[FA_THREADS / 64 + 1];
    __shared__ uint32_t s_c[FA_THREADS / 64 + 1];
    __shared__ uint8_t s_out[FA_TILE];
    const uint64_t t0 = (uint64_t)blockIdx.x * FA_TILE, b = t0 + (uint64_t)threadIdx.x * FA_BYTES;
    const uint4 v = *reinterpret_cast<const uint4*>(raw + b);
    uint64_t fhi, nxt;
    const uint64_t f0 = thread_first_file(file_off, n_files, n, t0, b, s_f, fhi, nxt);
    const uint64_t nxt0 = nxt;
    const uint64_t e = block_excl_map(thread_map(v, b, file_off, f0, fhi, nxt), s_w);
    const uint32_t s0 = map_apply(e, (uint32_t)tile_state[blockIdx.x]);
    // the thread's counts, then their exclusive sums over the workgroup
    uint32_t cnt = 0;
    {
        uint32_t s = s0;
        uint64_t f = f0;
        nxt = nxt0;
#pragma unroll
        for (int j = 0; j < (int)FA_BYTES; ++j) {
            if (b + j == nxt) {
                s = F_START;
                do {
                    ++f;
                    nxt = f < fhi ? file_off[f] : ~0ull;
                } while (nxt == b + j);
            }
            bool r, st;
            s = fasta_step(s, byte_of(v, j), r, st);
            cnt += (r ? 1u : 0u) + (st ? 0x10000u : 0u);
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t x = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    if (lane == 63) s_c[wave] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t acc = 0;
        for (int w = 0; w < (int)FA_THREADS / 64; ++w) {
            const uint32_t t = s_c[w];
            s_c[w] = acc;
            acc += t;
        }
        s_c[FA_THREADS / 64] = acc;
    }
    __syncthreads();
    const uint32_t ex = s_c[wave] + x - cnt, tot = s_c[FA_THREADS / 64];
    const uint64_t R0 = tile_cnt[2 * (uint64_t)blockIdx.x], S0 = tile_cnt[2 * (uint64_t)blockIdx.x + 1];
    uint64_t R = R0 + (ex & 0xFFFFu), S = S0 + (ex >> 16);
    uint32_t k = (ex & 0xFFFFu) + (ex >> 16);  // the thread's first event in the tile's output
    {
        uint32_t s = s0;
        uint64_t f = f0;
        nxt = nxt0;
#pragma unroll
        for (int j = 0; j < (int)FA_BYTES; ++j) {
            const uint64_t p = b + j;
            if (p == nxt) {
                s = F_START;
                do {
                    file_rec[f] = S;
                    ++f;
                    nxt = f < fhi ? file_off[f] : ~0ull;
                } while (nxt == p);
            }
            const uint32_t c = byte_of(v, j);
            bool r, st;
            s = fasta_step(s, c, r, st);
            // (the bounds below hold by construction -- this pass counts what k_fasta_count counted;
            // they are checked all the same, so that no mistake can write outside a buffer)
            if (r) {
                if (k < FA_TILE) s_out[k] = (uint8_t)c;
                ++k;
                ++R;
            }
            if (st) {
                if (k < FA_TILE) s_out[k] = 0;
                ++k;
                if (S < n_recs) {
                    pstart[S] = R + S;
                    uint64_t q = p - 1;  // the '>' that opened the record: only '\r' can lie between
                    while (q > 0 && raw[q] == '\r') --q;
                    hdr_pos[S] = q;
                }
                ++S;
            }
        }
    }
    __syncthreads();
    const uint32_t nev = min((tot & 0xFFFFu) + (tot >> 16), FA_TILE);
    const uint64_t o0 = R0 + S0;  // output position + 1 of the tile's first event
    for (uint32_t i = threadIdx.x; i < nev; i += FA_THREADS)
        if (o0 + i && o0 + i < rp) res[o0 + i - 1] = s_out[i];
}

// per kept record: QMeta, its length and its windows; *err |= 1 when a record is too long for u32
__global__ void k_fasta_meta(const uint64_t* __restrict__ pstart, uint64_t n_recs, uint64_t rp, QMeta* __restrict__ meta,
                             uint32_t* __restrict__ seq_len, uint32_t* __restrict__ nwin, uint64_t* __restrict__ err) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_recs) return;
    const uint64_t a = pstart[s], len = (s + 1 < n_recs ? pstart[s + 1] : rp) - a - 1;
    if (len > 0xFFFFFFFEull) *err = 1;
    QMeta m;
    m.pstart = a;
    m.len = (uint32_t)len;
    m.pad = 0;
    meta[s] = m;
    seq_len[s] = (uint32_t)len;
    nwin[s] = len >= 8 ? (uint32_t)len - 7 : 0;
}

// ------------------------------------------------------------------------------------------
// The selecting parse (fasta_parse_select): the build's input is a selection of each file's records
// (signature_build.tcc:93-158), rec_func[r] != 0xFFFF of parser record r.  The record current at byte
// p is S(p) - 1, known from the all-record scan above, so the selection needs one more counting pass
// and one more sum scan:
//   k_fasta_sel_count  per tile: selected residues and selected record starts
//   k_fasta_sum_scan   their exclusive sums and totals
//   k_fasta_sel_emit   k_fasta_emit with R and S counted over selected events only (the output), and
//                      over all events for the table (file_rec, hdr_pos, the all-record packed starts
//                      the lengths come from)
//   k_fasta_sel_len    per parser record: its length
// ------------------------------------------------------------------------------------------

// the thread's 16 bytes from state s: on_file(f) for every file that starts at one of them,
// on_byte(p, c, res, start) for every byte (fasta_step's events)
template <class FileFn, class ByteFn>
__device__ __forceinline__ void thread_walk(const uint4& v, uint64_t b, uint32_t s, const uint64_t* __restrict__ file_off,
                                            uint64_t f, uint64_t fhi, uint64_t nxt, FileFn on_file, ByteFn on_byte) {
#pragma unroll
    for (int j = 0; j < (int)FA_BYTES; ++j) {
        const uint64_t p = b + j;
        if (p == nxt) {
            s = F_START;
            do {
                on_file(f);
                ++f;
                nxt = f < fhi ? file_off[f] : ~0ull;
            } while (nxt == p);
        }
        const uint32_t c = byte_of(v, j);
        bool r, st;
        s = fasta_step(s, c, r, st);
        on_byte(p, c, r, st);
    }
}

// Workgroup exclusive sum of a packed pair of counts (low | high << 16, each at most FA_TILE over
// the workgroup); tot = the workgroup's sum.  s_c holds FA_THREADS / 64 + 1 words.
__device__ __forceinline__ uint32_t block_excl_pair(uint32_t cnt, uint32_t* s_c, uint32_t& tot) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t x = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    __syncthreads();  // s_c may still be read from an earlier call
    if (lane == 63) s_c[wave] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t acc = 0;
        for (int w = 0; w < (int)FA_THREADS / 64; ++w) {
            const uint32_t t = s_c[w];
            s_c[w] = acc;
            acc += t;
        }
        s_c[FA_THREADS / 64] = acc;
    }
    __syncthreads();
    tot = s_c[FA_THREADS / 64];
    return s_c[wave] + x - cnt;
}

__device__ __forceinline__ bool rec_selected(const uint16_t* __restrict__ rec_func, uint64_t n_recs, uint64_t r) {
    return r < n_recs && rec_func[r] != 0xFFFFu;
}

// the thread's selected residues | selected record starts << 16, S = the record starts before its
// first byte
__device__ __forceinline__ uint32_t thread_sel_counts(const uint4& v, uint64_t b, uint32_t s0,
                                                      const uint64_t* __restrict__ file_off, uint64_t f0, uint64_t fhi,
                                                      uint64_t nxt0, const uint16_t* __restrict__ rec_func, uint64_t n_recs,
                                                      uint64_t S) {
    bool cur = S > 0 && rec_selected(rec_func, n_recs, S - 1);
    uint32_t sel = 0;
    thread_walk(v, b, s0, file_off, f0, fhi, nxt0, [](uint64_t) {},
                [&](uint64_t, uint32_t, bool r, bool st) {
                    if (r && cur) ++sel;
                    if (st) {
                        cur = rec_selected(rec_func, n_recs, S);
                        if (cur) sel += 0x10000u;
                        ++S;
                    }
                });
    return sel;
}

__global__ __launch_bounds__(FA_THREADS) void k_fasta_sel_count(const uint8_t* __restrict__ raw, uint64_t n,
                                                                const uint64_t* __restrict__ file_off, uint64_t n_files,
                                                                const uint64_t* __restrict__ tile_state,
                                                                const uint64_t* __restrict__ tile_cnt,
                                                                const uint16_t* __restrict__ rec_func, uint64_t n_recs,
                                                                uint64_t* __restrict__ tile_sel) {
    __shared__ uint64_t s_f[2], s_w[FA_THREADS / 64 + 1];
    __shared__ uint32_t s_c[FA_THREADS / 64 + 1];
    const uint64_t t0 = (uint64_t)blockIdx.x * FA_TILE, b = t0 + (uint64_t)threadIdx.x * FA_BYTES;
    const uint4 v = *reinterpret_cast<const uint4*>(raw + b);
    uint64_t fhi, nxt;
    const uint64_t f0 = thread_first_file(file_off, n_files, n, t0, b, s_f, fhi, nxt);
    const uint64_t nxt0 = nxt;
    const uint64_t e = block_excl_map(thread_map(v, b, file_off, f0, fhi, nxt), s_w);
    const uint32_t s0 = map_apply(e, (uint32_t)tile_state[blockIdx.x]);
    uint32_t cnt = 0;
    thread_walk(v, b, s0, file_off, f0, fhi, nxt0, [](uint64_t) {},
                [&](uint64_t, uint32_t, bool r, bool st) { cnt += (r ? 1u : 0u) + (st ? 0x10000u : 0u); });
    uint32_t tot;
    const uint32_t ex = block_excl_pair(cnt, s_c, tot);
    (void)tot;
    const uint64_t S = tile_cnt[2 * (uint64_t)blockIdx.x + 1] + (ex >> 16);
    const uint32_t sel = thread_sel_counts(v, b, s0, file_off, f0, fhi, nxt0, rec_func, n_recs, S);
    uint32_t stot;
    (void)block_excl_pair(sel, s_c, stot);
    if (threadIdx.x == 0) {
        tile_sel[2 * (uint64_t)blockIdx.x] = stot & 0xFFFFu;
        tile_sel[2 * (uint64_t)blockIdx.x + 1] = stot >> 16;
    }
}

// k_fasta_emit's invariant with R and S counted over selected events only (Rs, Ss): a selected residue
// at p goes to dst[Rs(p) + Ss(p) - 1] and a selected record start puts the 0 that ends the selected
// record before it at the same expression, its own residues starting at sel_pstart = Rs + Ss.  The
// first selected start of all has position -1 (not stored); the 0 after the last selected record is
// the host's.  dst is any byte address: the range is stored byte by byte, contiguous over the
// workgroup.  all_pstart, hdr_pos and file_rec are k_fasta_emit's, over every parser record.
__global__ __launch_bounds__(FA_THREADS) void k_fasta_sel_emit(
    const uint8_t* __restrict__ raw, uint64_t n, const uint64_t* __restrict__ file_off, uint64_t n_files,
    const uint64_t* __restrict__ tile_state, const uint64_t* __restrict__ tile_cnt, const uint64_t* __restrict__ tile_sel,
    const uint16_t* __restrict__ rec_func, uint64_t n_recs, uint8_t* __restrict__ dst, uint64_t sel_bytes,
    uint64_t* __restrict__ sel_pstart, uint64_t* __restrict__ all_pstart, uint64_t* __restrict__ hdr_pos,
    uint64_t* __restrict__ file_rec) {
    __shared__ uint64_t s_f[2], s_w[FA_THREADS / 64 + 1];
    __shared__ uint32_t s_c[FA_THREADS / 64 + 1];
    __shared__ uint8_t s_out[FA_TILE];
    const uint64_t t0 = (uint64_t)blockIdx.x * FA_TILE, b = t0 + (uint64_t)threadIdx.x * FA_BYTES;
    const uint4 v = *reinterpret_cast<const uint4*>(raw + b);
    uint64_t fhi, nxt;
    const uint64_t f0 = thread_first_file(file_off, n_files, n, t0, b, s_f, fhi, nxt);
    const uint64_t nxt0 = nxt;
    const uint64_t e = block_excl_map(thread_map(v, b, file_off, f0, fhi, nxt), s_w);
    const uint32_t s0 = map_apply(e, (uint32_t)tile_state[blockIdx.x]);
    uint32_t cnt = 0;
    thread_walk(v, b, s0, file_off, f0, fhi, nxt0, [](uint64_t) {},
                [&](uint64_t, uint32_t, bool r, bool st) { cnt += (r ? 1u : 0u) + (st ? 0x10000u : 0u); });
    uint32_t tot, stot;
    const uint32_t ex = block_excl_pair(cnt, s_c, tot);
    (void)tot;
    uint64_t R = tile_cnt[2 * (uint64_t)blockIdx.x] + (ex & 0xFFFFu), S = tile_cnt[2 * (uint64_t)blockIdx.x + 1] + (ex >> 16);
    const uint32_t sel = thread_sel_counts(v, b, s0, file_off, f0, fhi, nxt0, rec_func, n_recs, S);
    const uint32_t sex = block_excl_pair(sel, s_c, stot);
    const uint64_t o0 = tile_sel[2 * (uint64_t)blockIdx.x] + tile_sel[2 * (uint64_t)blockIdx.x + 1];
    uint32_t k = (sex & 0xFFFFu) + (sex >> 16);  // the thread's first selected event in the tile's output
    bool cur = S > 0 && rec_selected(rec_func, n_recs, S - 1);
    thread_walk(
        v, b, s0, file_off, f0, fhi, nxt0, [&](uint64_t f) { file_rec[f] = S; },
        [&](uint64_t p, uint32_t c, bool r, bool st) {
            // (as in k_fasta_emit: the bounds hold by construction and are checked all the same)
            if (r) {
                if (cur) {
                    if (k < FA_TILE) s_out[k] = (uint8_t)c;
                    ++k;
                }
                ++R;
            }
            if (st) {
                cur = rec_selected(rec_func, n_recs, S);
                if (cur) {
                    if (k < FA_TILE) s_out[k] = 0;
                    ++k;
                }
                if (S < n_recs) {
                    all_pstart[S] = R + S;
                    sel_pstart[S] = cur ? o0 + k - 1 : ~0ull;  // its start is event o0 + k - 1, stored one before
                    uint64_t q = p - 1;  // the '>' that opened the record: only '\r' can lie between
                    while (q > 0 && raw[q] == '\r') --q;
                    hdr_pos[S] = q;
                }
                ++S;
            }
        });
    __syncthreads();
    const uint32_t nev = min((stot & 0xFFFFu) + (stot >> 16), FA_TILE);
    for (uint32_t i = threadIdx.x; i < nev; i += FA_THREADS)
        if (o0 + i && o0 + i < sel_bytes) dst[o0 + i - 1] = s_out[i];
}

// per parser record its length; *err |= 1 when one is too long for u32
__global__ void k_fasta_sel_len(const uint64_t* __restrict__ all_pstart, uint64_t n_recs, uint64_t rp,
                                uint32_t* __restrict__ seq_len, uint64_t* __restrict__ err) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_recs) return;
    const uint64_t len = (s + 1 < n_recs ? all_pstart[s + 1] : rp) - all_pstart[s] - 1;
    if (len > 0xFFFFFFFEull) *err = 1;
    seq_len[s] = (uint32_t)len;
}

}  // namespace

FastaWork::~FastaWork() {
    for (auto& e : ev)
        if (e) (void)hipEventDestroy(e);
}

void fasta_check_args(const uint8_t* bytes, const uint64_t* file_off, size_t n_files) {
    SKM_CHECK(file_off, SKM_E_ARG, "null file_off");
    SKM_CHECK(file_off[0] == 0, SKM_E_ARG, "file_off[0] must be 0");
    for (size_t f = 0; f < n_files; ++f)
        SKM_CHECK(file_off[f] <= file_off[f + 1], SKM_E_ARG, "file_off must ascend");
    SKM_CHECK(bytes || file_off[n_files] == 0, SKM_E_ARG, "null bytes");
}

FastaTotals fasta_parse(FastaWork& w, const uint8_t* bytes, const uint64_t* file_off, size_t n_files, hipStream_t st,
                        DevBuf& d_res, DevBuf& d_meta, DevBuf& d_scr_off, int want_residues, skm_fasta_table* tab) {
    FastaTotals T;
    const uint64_t n = file_off[n_files];
    const uint64_t nt = ceil_div(n, FA_TILE), n_pad = nt * FA_TILE;
    for (auto& e : w.ev)
        if (!e) SKM_HIP(hipEventCreate(&e));
    uint64_t tot[2] = {0, 0};
    float ms0 = 0, ms1 = 0;
    if (n) {
        alloc_reported(w.d_raw, n_pad, "FASTA file bytes");
        w.d_foff.ensure(8 * (n_files + 1));
        w.d_tmap.ensure(8 * nt);
        w.d_tcnt.ensure(16 * (nt + 1));
        SKM_HIP(hipMemcpyAsync(w.d_raw.p, bytes, n, hipMemcpyHostToDevice, st));
        // '\r' is dropped in every state: the pad bytes of the last tile parse to nothing
        if (n_pad > n) SKM_HIP(hipMemsetAsync(w.d_raw.as<uint8_t>() + n, '\r', n_pad - n, st));
        SKM_HIP(hipMemcpyAsync(w.d_foff.p, file_off, 8 * (n_files + 1), hipMemcpyHostToDevice, st));
        SKM_HIP(hipEventRecord(w.ev[0], st));
        hipLaunchKernelGGL(k_fasta_maps, dim3((uint32_t)nt), dim3(FA_THREADS), 0, st, w.d_raw.as<uint8_t>(), n,
                           w.d_foff.as<uint64_t>(), (uint64_t)n_files, w.d_tmap.as<uint64_t>());
        hipLaunchKernelGGL(k_fasta_map_scan, dim3(1), dim3(1024), 0, st, w.d_tmap.as<uint64_t>(), nt);
        hipLaunchKernelGGL(k_fasta_count, dim3((uint32_t)nt), dim3(FA_THREADS), 0, st, w.d_raw.as<uint8_t>(), n,
                           w.d_foff.as<uint64_t>(), (uint64_t)n_files, w.d_tmap.as<uint64_t>(), w.d_tcnt.as<uint64_t>());
        hipLaunchKernelGGL(k_fasta_sum_scan, dim3(1), dim3(1024), 0, st, w.d_tcnt.as<uint64_t>(), nt);
        SKM_HIP(hipGetLastError());
        SKM_HIP(hipEventRecord(w.ev[1], st));
        SKM_HIP(hipMemcpyAsync(tot, w.d_tcnt.as<uint64_t>() + 2 * nt, 16, hipMemcpyDeviceToHost, st));
        SKM_HIP(hipStreamSynchronize(st));
        SKM_HIP(hipEventElapsedTime(&ms0, w.ev[0], w.ev[1]));
    }
    const uint64_t n_recs = tot[1];
    SKM_CHECK(n_recs < 0xFFFFFFFFull, SKM_E_ARG, "too many query sequences in one batch");
    T.n_recs = n_recs;
    T.n_residues = tot[0];
    T.rp = tot[0] + n_recs;
    // the sizes query_setup gives the residue buffer: hits are written in 16-window groups
    const uint64_t rp_pad = ceil_div(T.rp + 1, LK_POS) * LK_POS;
    alloc_reported(d_res, rp_pad + 64, "packed query residues");
    d_meta.ensure(sizeof(QMeta) * std::max<uint64_t>(n_recs, 1));
    d_scr_off.ensure(8 * (n_recs + 1));
    // the download: error flag, file_rec [n_files + 1], hdr_pos [n_recs], seq_len [n_recs]
    const uint64_t tab_bytes = 8 * (1 + n_files + 1 + n_recs) + 4 * n_recs;
    w.d_tab.ensure(tab_bytes);
    uint64_t* d_err = w.d_tab.as<uint64_t>();
    uint64_t* d_file_rec = d_err + 1;
    uint64_t* d_hdr = d_file_rec + n_files + 1;
    uint32_t* d_len = reinterpret_cast<uint32_t*>(d_hdr + n_recs);
    SKM_HIP(hipMemsetAsync(w.d_tab.p, 0, 8 * (1 + n_files + 1), st));
    const uint64_t tail = T.rp ? T.rp - 1 : 0;
    SKM_HIP(hipMemsetAsync(d_res.as<uint8_t>() + tail, 0, rp_pad + 64 - tail, st));
    if (n) {
        w.d_pstart.ensure(8 * std::max<uint64_t>(n_recs, 1));
        w.d_nwin.ensure(4 * std::max<uint64_t>(n_recs, 1));
        SKM_HIP(hipEventRecord(w.ev[2], st));
        hipLaunchKernelGGL(k_fasta_emit, dim3((uint32_t)nt), dim3(FA_THREADS), 0, st, w.d_raw.as<uint8_t>(), n,
                           w.d_foff.as<uint64_t>(), (uint64_t)n_files, w.d_tmap.as<uint64_t>(), w.d_tcnt.as<uint64_t>(),
                           d_res.as<uint8_t>(), w.d_pstart.as<uint64_t>(), d_hdr, d_file_rec, n_recs, T.rp);
        if (n_recs) {
            hipLaunchKernelGGL(k_fasta_meta, dim3((uint32_t)ceil_div(n_recs, 256)), dim3(256), 0, st,
                               w.d_pstart.as<uint64_t>(), n_recs, T.rp, d_meta.as<QMeta>(), d_len, w.d_nwin.as<uint32_t>(),
                               d_err);
            w.scan.run(w.d_nwin.as<uint32_t>(), n_recs, d_scr_off.as<uint64_t>(), st);
        }
        SKM_HIP(hipGetLastError());
        SKM_HIP(hipEventRecord(w.ev[3], st));
    }
    std::vector<uint8_t> host(tab_bytes);
    SKM_HIP(hipMemcpyAsync(host.data(), w.d_tab.p, tab_bytes, hipMemcpyDeviceToHost, st));
    if (n_recs) SKM_HIP(hipMemcpyAsync(&T.n_windows, d_scr_off.as<uint64_t>() + n_recs, 8, hipMemcpyDeviceToHost, st));
    SKM_HIP(hipStreamSynchronize(st));
    if (n) SKM_HIP(hipEventElapsedTime(&ms1, w.ev[2], w.ev[3]));
    T.ms = ms0 + ms1;
    const uint64_t* h_err = reinterpret_cast<const uint64_t*>(host.data());
    SKM_CHECK(!h_err[0], SKM_E_ARG, "a record is longer than 2^32 - 2 residues");
    if (tab) {
        std::memset(tab, 0, sizeof(*tab));
        skm_fasta_table t{};
        t.n_files = n_files;
        t.n_recs = n_recs;
        t.n_residues = T.n_residues;
        t.n_windows = T.n_windows;
        t.parse_ms = T.ms;
        t.file_rec = (uint64_t*)std::malloc(8 * (n_files + 1));
        t.seq_len = (uint32_t*)std::malloc(4 * std::max<uint64_t>(n_recs, 1));
        t.hdr_pos = (uint64_t*)std::malloc(8 * std::max<uint64_t>(n_recs, 1));
        if (want_residues) t.residues = (uint8_t*)std::malloc(std::max<uint64_t>(T.rp, 1));
        try {
            SKM_CHECK(t.file_rec && t.seq_len && t.hdr_pos && (!want_residues || t.residues), SKM_E_OOM,
                      "host allocation failed");
            std::memcpy(t.file_rec, h_err + 1, 8 * (n_files + 1));
            // the files that start at the end of the bytes (empty ones) and the end itself
            for (size_t f = 0; f <= n_files; ++f)
                if (file_off[f] == n) t.file_rec[f] = n_recs;
            std::memcpy(t.hdr_pos, h_err + 1 + n_files + 1, 8 * n_recs);
            std::memcpy(t.seq_len, h_err + 1 + n_files + 1 + n_recs, 4 * n_recs);
            if (want_residues && T.rp) {
                SKM_HIP(hipMemcpyAsync(t.residues, d_res.p, T.rp, hipMemcpyDeviceToHost, st));
                SKM_HIP(hipStreamSynchronize(st));
            }
        } catch (...) {
            skm_fasta_table_free(&t);
            throw;
        }
        *tab = t;
    }
    return T;
}

FastaSelect fasta_parse_select(FastaWork& w, const uint8_t* bytes, const uint64_t* file_off, size_t n_files,
                               const uint16_t* rec_func, uint64_t n_recs, hipStream_t st,
                               const std::function<uint8_t*(uint64_t)>& reserve, std::vector<uint64_t>& sel_pstart,
                               skm_fasta_table* tab) {
    FastaSelect T;
    const uint64_t n = file_off[n_files];
    const uint64_t nt = ceil_div(n, FA_TILE), n_pad = nt * FA_TILE;
    for (auto& e : w.ev)
        if (!e) SKM_HIP(hipEventCreate(&e));
    uint64_t tot[4] = {0, 0, 0, 0};  // residues, records; selected residues, selected records
    float ms0 = 0, ms1 = 0;
    if (n) {
        alloc_reported(w.d_raw, n_pad, "FASTA file bytes");
        w.d_foff.ensure(8 * (n_files + 1));
        w.d_tmap.ensure(8 * nt);
        w.d_tcnt.ensure(16 * (nt + 1));
        w.d_tsel.ensure(16 * (nt + 1));
        w.d_rfunc.ensure(2 * std::max<uint64_t>(n_recs, 1));
        SKM_HIP(hipMemcpyAsync(w.d_raw.p, bytes, n, hipMemcpyHostToDevice, st));
        if (n_pad > n) SKM_HIP(hipMemsetAsync(w.d_raw.as<uint8_t>() + n, '\r', n_pad - n, st));
        SKM_HIP(hipMemcpyAsync(w.d_foff.p, file_off, 8 * (n_files + 1), hipMemcpyHostToDevice, st));
        if (n_recs) SKM_HIP(hipMemcpyAsync(w.d_rfunc.p, rec_func, 2 * n_recs, hipMemcpyHostToDevice, st));
        SKM_HIP(hipEventRecord(w.ev[0], st));
        hipLaunchKernelGGL(k_fasta_maps, dim3((uint32_t)nt), dim3(FA_THREADS), 0, st, w.d_raw.as<uint8_t>(), n,
                           w.d_foff.as<uint64_t>(), (uint64_t)n_files, w.d_tmap.as<uint64_t>());
        hipLaunchKernelGGL(k_fasta_map_scan, dim3(1), dim3(1024), 0, st, w.d_tmap.as<uint64_t>(), nt);
        hipLaunchKernelGGL(k_fasta_count, dim3((uint32_t)nt), dim3(FA_THREADS), 0, st, w.d_raw.as<uint8_t>(), n,
                           w.d_foff.as<uint64_t>(), (uint64_t)n_files, w.d_tmap.as<uint64_t>(), w.d_tcnt.as<uint64_t>());
        hipLaunchKernelGGL(k_fasta_sum_scan, dim3(1), dim3(1024), 0, st, w.d_tcnt.as<uint64_t>(), nt);
        // a record past the caller's n_recs counts as not selected: the counts are compared below,
        // before anything is made of the selection
        hipLaunchKernelGGL(k_fasta_sel_count, dim3((uint32_t)nt), dim3(FA_THREADS), 0, st, w.d_raw.as<uint8_t>(), n,
                           w.d_foff.as<uint64_t>(), (uint64_t)n_files, w.d_tmap.as<uint64_t>(), w.d_tcnt.as<uint64_t>(),
                           w.d_rfunc.as<uint16_t>(), n_recs, w.d_tsel.as<uint64_t>());
        hipLaunchKernelGGL(k_fasta_sum_scan, dim3(1), dim3(1024), 0, st, w.d_tsel.as<uint64_t>(), nt);
        SKM_HIP(hipGetLastError());
        SKM_HIP(hipEventRecord(w.ev[1], st));
        SKM_HIP(hipMemcpyAsync(tot, w.d_tcnt.as<uint64_t>() + 2 * nt, 16, hipMemcpyDeviceToHost, st));
        SKM_HIP(hipMemcpyAsync(tot + 2, w.d_tsel.as<uint64_t>() + 2 * nt, 16, hipMemcpyDeviceToHost, st));
        SKM_HIP(hipStreamSynchronize(st));
        SKM_HIP(hipEventElapsedTime(&ms0, w.ev[0], w.ev[1]));
    }
    T.ms = ms0;
    SKM_CHECK(tot[1] == n_recs, SKM_E_ARG,
              "the files hold " + std::to_string(tot[1]) + " records with an id, the selection describes " +
                  std::to_string(n_recs));
    T.n_recs = n_recs;
    T.n_residues = tot[0];
    T.sel_residues = tot[2];
    T.n_sel = tot[3];
    T.sel_bytes = tot[2] + tot[3];
    const uint64_t rp_all = tot[0] + n_recs;
    uint8_t* dst = T.sel_bytes ? reserve(T.sel_bytes) : nullptr;
    // the download: error flag, file_rec [n_files + 1], hdr_pos [n_recs], sel_pstart [n_recs], seq_len [n_recs]
    const uint64_t tab_bytes = 8 * (1 + n_files + 1 + 2 * n_recs) + 4 * n_recs;
    w.d_tab.ensure(tab_bytes);
    uint64_t* d_err = w.d_tab.as<uint64_t>();
    uint64_t* d_file_rec = d_err + 1;
    uint64_t* d_hdr = d_file_rec + n_files + 1;
    uint64_t* d_sps = d_hdr + n_recs;
    uint32_t* d_len = reinterpret_cast<uint32_t*>(d_sps + n_recs);
    SKM_HIP(hipMemsetAsync(w.d_tab.p, 0, 8 * (1 + n_files + 1), st));
    if (n) {
        w.d_pstart.ensure(8 * std::max<uint64_t>(n_recs, 1));
        SKM_HIP(hipEventRecord(w.ev[2], st));
        hipLaunchKernelGGL(k_fasta_sel_emit, dim3((uint32_t)nt), dim3(FA_THREADS), 0, st, w.d_raw.as<uint8_t>(), n,
                           w.d_foff.as<uint64_t>(), (uint64_t)n_files, w.d_tmap.as<uint64_t>(), w.d_tcnt.as<uint64_t>(),
                           w.d_tsel.as<uint64_t>(), w.d_rfunc.as<uint16_t>(), n_recs, dst, T.sel_bytes, d_sps,
                           w.d_pstart.as<uint64_t>(), d_hdr, d_file_rec);
        if (n_recs)
            hipLaunchKernelGGL(k_fasta_sel_len, dim3((uint32_t)ceil_div(n_recs, 256)), dim3(256), 0, st,
                               w.d_pstart.as<uint64_t>(), n_recs, rp_all, d_len, d_err);
        SKM_HIP(hipGetLastError());
        SKM_HIP(hipEventRecord(w.ev[3], st));
    }
    std::vector<uint8_t> host(tab_bytes);
    SKM_HIP(hipMemcpyAsync(host.data(), w.d_tab.p, tab_bytes, hipMemcpyDeviceToHost, st));
    SKM_HIP(hipStreamSynchronize(st));
    if (n) SKM_HIP(hipEventElapsedTime(&ms1, w.ev[2], w.ev[3]));
    T.ms = ms0 + ms1;
    const uint64_t* h = reinterpret_cast<const uint64_t*>(host.data());
    SKM_CHECK(!h[0], SKM_E_ARG, "a record is longer than 2^32 - 2 residues");
    sel_pstart.assign(h + 1 + n_files + 1 + n_recs, h + 1 + n_files + 1 + 2 * n_recs);
    std::memset(tab, 0, sizeof(*tab));
    skm_fasta_table t{};
    t.n_files = n_files;
    t.n_recs = n_recs;
    t.n_residues = T.n_residues;
    t.parse_ms = T.ms;
    t.file_rec = (uint64_t*)std::malloc(8 * (n_files + 1));
    t.seq_len = (uint32_t*)std::malloc(4 * std::max<uint64_t>(n_recs, 1));
    t.hdr_pos = (uint64_t*)std::malloc(8 * std::max<uint64_t>(n_recs, 1));
    if (!(t.file_rec && t.seq_len && t.hdr_pos)) {
        skm_fasta_table_free(&t);
        throw Error(SKM_E_OOM, "host allocation failed");
    }
    std::memcpy(t.file_rec, h + 1, 8 * (n_files + 1));
    for (size_t f = 0; f <= n_files; ++f)  // the files that start at the end of the bytes, and the end itself
        if (file_off[f] == n) t.file_rec[f] = n_recs;
    std::memcpy(t.hdr_pos, h + 1 + n_files + 1, 8 * n_recs);
    std::memcpy(t.seq_len, h + 1 + n_files + 1 + 2 * n_recs, 4 * n_recs);
    for (uint64_t r = 0; r < n_recs; ++r) t.n_windows += t.seq_len[r] >= 8 ? t.seq_len[r] - 7 : 0;
    *tab = t;
    return T;
}

}  // namespace skm

using namespace skm;

int skm_fasta_parse_info(uint32_t out[4]) {
    if (!out) return SKM_E_ARG;
    out[0] = FA_BYTES;
    out[1] = FA_WAVE_BYTES;
    out[2] = FA_TILE;
    out[3] = 0;
    return SKM_OK;
}

int skm_fasta_parse_device(const uint8_t* bytes, const uint64_t* file_off, size_t n_files, int device, int want_residues,
                           skm_fasta_table* out) {
    SKM_API_BEGIN
    SKM_CHECK(out, SKM_E_ARG, "null output");
    fasta_check_args(bytes, file_off, n_files);
    SKM_HIP(hipSetDevice(device));
    std::memset(out, 0, sizeof(*out));
    FastaWork w;
    DevBuf d_res, d_meta, d_scr_off;
    fasta_parse(w, bytes, file_off, n_files, nullptr, d_res, d_meta, d_scr_off, want_residues, out);
    SKM_API_END
}

void skm_fasta_table_free(skm_fasta_table* t) {
    if (!t) return;
    std::free(t->file_rec);
    std::free(t->seq_len);
    std::free(t->hdr_pos);
    std::free(t->residues);
    std::memset(t, 0, sizeof(*t));
}
