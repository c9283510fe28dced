// skm_output.hip -- the kept-set hand-off: a build's kept k-mers from HBM to the caller's host
// arrays, in ascending key order (skm_build_finish / skm_build_finish_slice), and final.kmers
// formatted on the device from the same arena (skm_build_write_final_kmers).
//
// The reference writes final.kmers and the .dat from one in-memory KeptKmers map in hash order
// (kmers-build-signatures.cc:198-264); this port hands the set back sorted (deterministic output).
// Round 4 downloaded the whole arena, then sorted an index permutation on ONE host thread
// (~30 s for C2's 168.7 M kept k-mers; C3's 2.89 G did not fit host memory twice over).  Now:
//
//   k_out_hist    one read of the arena's keys: a 16384-bin histogram of the sort code's top bits
//   host plan     consecutive bins into chunks of <= ~2^27 k-mers (any size works: a chunk's
//                 device scratch is sized to the largest)
//   per chunk     k_out_select (the chunk's (sort code, arena index) pairs, wave-aggregated
//                 compaction) -> rocPRIM radix sort of the pairs (43 bits) -> k_out_gather (the
//                 keys and 10-byte records in key order, double-buffered) -> D2H in 64 MB pieces
//                 through two pinned buffers, each piece copied out to the caller's arrays by the
//                 host pool while the next piece is in flight; chunk c+1 sorts while chunk c drains
//
// final.kmers (skm_build_write_final_kmers) takes the same chunks and stops before the gather:
//
//   per chunk     k_out_select -> radix sort -> k_fk_len (text bytes of every tile of 1024 lines,
//                 read through the sorted index) -> exclusive scan of the tile sizes (Scanner) ->
//                 k_fk_emit (a tile's lines staged in LDS, stored as aligned 16-byte units into one
//                 of two text buffers) -> the chunk's text size read back (8 bytes, the file
//                 offsets) -> D2H in pieces through two pinned buffers, each written to the file
//                 with pwrite by the host pool while the next piece is in flight
//
// Sort code: the little-endian key's bytes are compared from byte 7 down (u64 order), and the 40
// residue codes of ok_prot_ (skm_common.h residue_code: upper case 0..19, lower case 20..39, each
// ascending in byte value) are monotone in the byte, so sum_j code(byte j) * 40^j (< 2^43) orders
// kept keys exactly as their u64 values do.
#include <hip/hip_runtime.h>
#include <sys/mman.h>

#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstdlib>
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>
#include <string>
#include <vector>

#include "skm_common.h"
#include "skm_finalkmers.h"
#include "skm_lookup.h"
#include "skm_output.h"
#include "skm_util.h"

namespace skm {

namespace {

constexpr int OUT_BIN_BITS = 14;                        // histogram bins: top bits of the 43-bit code
constexpr int OUT_BIN_SHIFT = KEY_BITS - OUT_BIN_BITS;  // 29
constexpr uint32_t OUT_BINS = 1u << OUT_BIN_BITS;
constexpr int OUT_THREADS = 256;

__device__ __forceinline__ uint64_t sort_code(uint64_t raw) {
    uint64_t c = 0;
#pragma unroll
    for (int j = 7; j >= 0; --j) c = c * 40u + residue_code((uint32_t)(raw >> (8 * j)) & 0xFFu);
    return c;
}

__global__ __launch_bounds__(OUT_THREADS) void k_out_hist(const uint64_t* __restrict__ keys, uint64_t n,
                                                          uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[OUT_BINS];
    for (uint32_t i = threadIdx.x; i < OUT_BINS; i += OUT_THREADS) h[i] = 0;
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * OUT_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * OUT_THREADS)
        atomicAdd(&h[sort_code(keys[i]) >> OUT_BIN_SHIFT], 1u);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < OUT_BINS; i += OUT_THREADS)
        if (h[i]) atomicAdd(&hist[i], h[i]);
}

// the (sort code, arena index) pairs of the keys whose bin lies in [lo, hi).  Tiles of 16
// elements per thread (coalesced, strided by the block); the block's selected count is scanned
// over its waves and reserved with ONE atomic per tile -- a chunk selects ~1/22 of the arena's
// keys, spread over it in hash order, so a per-wave reservation put ~40 M atomics on one address
// per chunk at C3 (0.5 s per chunk)
// per chunk -- the arena index is a u32 below 2^32 kept k-mers, a u64 from there (a multi-GPU
// build hands rank 0 the union of every rank's kept set)
constexpr int SEL_ITEMS = 16;
template <class IdxT>
__global__ __launch_bounds__(OUT_THREADS) void k_out_select(const uint64_t* __restrict__ keys, uint64_t n, uint32_t lo,
                                                            uint32_t hi, unsigned long long* __restrict__ cur,
                                                            uint64_t* __restrict__ code, IdxT* __restrict__ idx) {
    constexpr int NW = OUT_THREADS / 64;
    __shared__ uint32_t wsum[NW];
    __shared__ unsigned long long base_s;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t TILE = (uint64_t)OUT_THREADS * SEL_ITEMS;
    for (uint64_t t0 = (uint64_t)blockIdx.x * TILE; t0 < n; t0 += (uint64_t)gridDim.x * TILE) {
        uint64_t c[SEL_ITEMS];
        uint32_t mask = 0;
#pragma unroll
        for (int j = 0; j < SEL_ITEMS; ++j) {
            const uint64_t i = t0 + (uint64_t)j * OUT_THREADS + tid;
            c[j] = i < n ? sort_code(keys[i]) : 0;
            const uint32_t bin = (uint32_t)(c[j] >> OUT_BIN_SHIFT);
            mask |= (i < n && bin >= lo && bin < hi) ? (1u << j) : 0u;
        }
        // exclusive prefix of the per-thread counts within the wave (shuffle scan), then over waves
        const uint32_t cnt = (uint32_t)__popc(mask);
        uint32_t incl = cnt;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t v = __shfl_up(incl, d);
            if (lane >= (uint32_t)d) incl += v;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        if (tid == 0) {
            uint32_t tot = 0;
            for (int w = 0; w < NW; ++w) tot += wsum[w];
            base_s = tot ? atomicAdd(cur, (unsigned long long)tot) : 0ull;
        }
        __syncthreads();
        uint64_t o = base_s + (incl - cnt);
        for (uint32_t w = 0; w < wave; ++w) o += wsum[w];
#pragma unroll
        for (int j = 0; j < SEL_ITEMS; ++j)
            if ((mask >> j) & 1u) {
                code[o] = c[j];
                idx[o] = (IdxT)(t0 + (uint64_t)j * OUT_THREADS + tid);
                ++o;
            }
        __syncthreads();  // wsum / base_s are rewritten by the next tile
    }
}

template <class IdxT>
__global__ __launch_bounds__(OUT_THREADS) void k_out_gather(const uint64_t* __restrict__ keys,
                                                            const skm_stored_kmer_data* __restrict__ data,
                                                            const IdxT* __restrict__ idx, uint64_t m,
                                                            uint64_t* __restrict__ okeys,
                                                            skm_stored_kmer_data* __restrict__ odata) {
    for (uint64_t j = (uint64_t)blockIdx.x * OUT_THREADS + threadIdx.x; j < m; j += (uint64_t)gridDim.x * OUT_THREADS) {
        const IdxT i = idx[j];
        okeys[j] = keys[i];
        odata[j] = data[i];
    }
}

// ---- final.kmers formatted on the device (skm_build_write_final_kmers) ----
// A tile is FK_LINES consecutive lines of a chunk's sorted order, one workgroup of FK_THREADS
// threads, FK_PER consecutive lines per thread.  A workgroup rather than a wave: its output range
// (14..22 KB) gives every one of the 256 threads several aligned 16-byte units to store, and the
// unaligned head and tail, at most 15 bytes each, are paid once per 1024 lines instead of once
// per 64.  Keys and records are read through the sorted index (no k_out_gather pass and no
// gathered copies): 18 B of random reads per line either way, and the 18 B written and read
// again by a gather are saved.
constexpr int FK_THREADS = 256, FK_PER = 4, FK_LINES = FK_THREADS * FK_PER;
constexpr uint32_t FK_IMG = FK_LINES * FK_MAX_LINE;  // the longest tile, bytes

// the bytes of thread tid's lines of tile `tile`; the keys and the two printed u16 (af = avg_from_end |
// function_index << 16) stay in registers, valid = the mask of the lines that exist
template <class IdxT>
__device__ __forceinline__ uint32_t fk_thread_lines(const uint64_t* __restrict__ keys,
                                                    const skm_stored_kmer_data* __restrict__ data, uint64_t n,
                                                    const IdxT* __restrict__ idx, uint64_t m, uint64_t tile, uint32_t tid,
                                                    uint64_t (&key)[FK_PER], uint32_t (&af)[FK_PER], uint32_t& valid, bool want_keys) {
    uint32_t bytes = 0;
    valid = 0;
#pragma unroll
    for (int q = 0; q < FK_PER; ++q) {
        const uint64_t j = tile * FK_LINES + (uint64_t)tid * FK_PER + q;
        key[q] = 0;
        af[q] = 0;
        if (j < m) {
            const uint64_t i = (uint64_t)idx[j];
            if (i < n) {  // holds by construction (k_out_select wrote arena indices); checked all the same
                valid |= 1u << q;
                af[q] = (uint32_t)data[i].avg_from_end | (uint32_t)data[i].function_index << 16;
                if (want_keys) key[q] = keys[i];
                bytes += fk_line_len(af[q] & 0xFFFFu, af[q] >> 16);
            }
        }
    }
    return bytes;
}

// sum of v over the workgroup (s_w: FK_THREADS / 64 words); excl = the exclusive prefix at this thread
__device__ __forceinline__ uint32_t fk_block_scan(uint32_t v, uint32_t* s_w, uint32_t& excl) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d, 64);
        if (lane >= (uint32_t)d) x += y;
    }
    if (lane == 63) s_w[wave] = x;
    __syncthreads();
    uint32_t before = 0, tot = 0;
#pragma unroll
    for (uint32_t w = 0; w < FK_THREADS / 64; ++w) {
        const uint32_t t = s_w[w];
        before += w < wave ? t : 0u;
        tot += t;
    }
    excl = before + x - v;
    return tot;
}

// text bytes of every tile of a chunk
template <class IdxT>
__global__ __launch_bounds__(FK_THREADS) void k_fk_len(const skm_stored_kmer_data* __restrict__ data, uint64_t n,
                                                       const IdxT* __restrict__ idx, uint64_t m,
                                                       uint32_t* __restrict__ tile_bytes) {
    __shared__ uint32_t s_w[FK_THREADS / 64];
    uint64_t key[FK_PER];
    uint32_t af[FK_PER], excl, valid;
    const uint32_t b = fk_thread_lines<IdxT>(nullptr, data, n, idx, m, blockIdx.x, threadIdx.x, key, af, valid, false);
    const uint32_t tot = fk_block_scan(b, s_w, excl);
    if (threadIdx.x == 0) tile_bytes[blockIdx.x] = tot;
}

// One tile: the lines are written into an LDS image of the tile's output range, laid out so that
// an LDS byte and the text byte it becomes have the same address modulo 16, then stored as aligned
// 16-byte units (global_store_dwordx4, consecutive lanes on consecutive units); only the bytes
// before the first and after the last whole unit go out one by one.  tile_off: the chunk's
// exclusive scan of k_fk_len's sizes (u64).  Nothing is stored beyond text[cap).
template <class IdxT>
__global__ __launch_bounds__(FK_THREADS) void k_fk_emit(const uint64_t* __restrict__ keys,
                                                        const skm_stored_kmer_data* __restrict__ data, uint64_t n,
                                                        const IdxT* __restrict__ idx, uint64_t m,
                                                        const uint64_t* __restrict__ tile_off, uint8_t* __restrict__ text,
                                                        uint64_t cap) {
    __shared__ uint32_t s_w[FK_THREADS / 64];
    __shared__ __attribute__((aligned(16))) uint8_t s_img[FK_IMG + 16];
    uint64_t key[FK_PER];
    uint32_t af[FK_PER], excl, valid;
    const uint32_t b = fk_thread_lines<IdxT>(keys, data, n, idx, m, blockIdx.x, threadIdx.x, key, af, valid, true);
    const uint32_t tot = fk_block_scan(b, s_w, excl);  // tot <= FK_IMG: FK_LINES lines of <= FK_MAX_LINE
    const uint64_t o0 = tile_off[blockIdx.x];
    if (tot == 0 || o0 > cap || tot > cap - o0) return;  // (uniform over the workgroup)
    uint8_t* const dst = text + o0;
    const uint32_t shift = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u);
    uint32_t at = shift + excl;
#pragma unroll
    for (int q = 0; q < FK_PER; ++q)
        if ((valid >> q) & 1u) at += fk_write_line(s_img + at, key[q], af[q] & 0xFFFFu, af[q] >> 16);
    __syncthreads();
    // image bytes [shift, end) -> dst[0, tot); whole units [ub, ue)
    const uint32_t end = shift + tot, ub = (shift + 15u) >> 4, ue = end >> 4;
    uint8_t* const base = dst - shift;  // 16-byte aligned
    if (ub < ue) {
        for (uint32_t u = ub + threadIdx.x; u < ue; u += FK_THREADS)
            *reinterpret_cast<uint4*>(base + 16u * u) = *reinterpret_cast<const uint4*>(s_img + 16u * u);
        for (uint32_t i = shift + threadIdx.x; i < 16u * ub; i += FK_THREADS) base[i] = s_img[i];
        for (uint32_t i = 16u * ue + threadIdx.x; i < end; i += FK_THREADS) base[i] = s_img[i];
    } else {
        for (uint32_t i = shift + threadIdx.x; i < end; i += FK_THREADS) base[i] = s_img[i];
    }
}

struct Chunk {
    uint32_t lo, hi;     // bins [lo, hi)
    uint64_t n, at;      // k-mers, output offset
};

// one read of the arena's keys into the histogram, then consecutive bins into chunks of <= 2^27
// k-mers (<= max_chunk) whose device scratch, `per` bytes per k-mer, stays within 3/4 of the memory
// free now -- the builder's work buffers are still allocated at finish, and a recall table may be
// open beside a released handle.  cmax = the largest chunk.
std::vector<Chunk> plan_chunks(const uint64_t* dkeys, uint64_t n, hipStream_t st, uint32_t grid, uint64_t per,
                               uint64_t max_chunk, uint64_t& cmax) {
    DevBuf d_hist;
    d_hist.ensure(4ull * OUT_BINS);
    SKM_HIP(hipMemsetAsync(d_hist.p, 0, 4ull * OUT_BINS, st));
    hipLaunchKernelGGL(k_out_hist, dim3(grid), dim3(OUT_THREADS), 0, st, dkeys, n, d_hist.as<uint32_t>());
    SKM_HIP(hipGetLastError());
    std::vector<uint32_t> hist(OUT_BINS);
    SKM_HIP(hipMemcpyAsync(hist.data(), d_hist.p, 4ull * OUT_BINS, hipMemcpyDeviceToHost, st));
    SKM_HIP(hipStreamSynchronize(st));
    size_t free_b = 0, total_b = 0;
    SKM_HIP(hipMemGetInfo(&free_b, &total_b));
    const uint64_t fit = std::max<uint64_t>(1ull << 16, (uint64_t)(0.75 * (double)free_b) / per);
    uint64_t target = std::max<uint64_t>(1ull << 22, std::min<uint64_t>(1ull << 27, ceil_div(n, 4)));
    target = std::min(target, std::min(fit, max_chunk));
    std::vector<Chunk> chunks;
    uint64_t tot = 0;
    cmax = 0;
    for (uint32_t b = 0; b < OUT_BINS;) {
        Chunk c{b, b, 0, tot};
        while (c.hi < OUT_BINS && (c.n == 0 || c.n + hist[c.hi] <= target)) c.n += hist[c.hi++];
        b = c.hi;
        if (c.n) {
            chunks.push_back(c);
            tot += c.n;
            cmax = std::max(cmax, c.n);
        }
    }
    SKM_CHECK(tot == n, SKM_E_STATE, "kept-set hand-off: histogram does not cover the arena");
    return chunks;
}

// host arrays for n records; large ones on 2 MB pages (fewer first-touch faults in the copy-out)
void* host_alloc(size_t bytes) {
    const size_t a = 1ull << 21;
    if (bytes < (64ull << 20)) return std::malloc(std::max<size_t>(bytes, 16));
    void* p = std::aligned_alloc(a, (bytes + a - 1) / a * a);
    if (p) (void)madvise(p, (bytes + a - 1) / a * a, MADV_HUGEPAGE);
    return p;
}

}  // namespace

namespace {

template <class IdxT>
void kept_handoff_t(const uint64_t* dkeys, const skm_stored_kmer_data* ddata, uint64_t n, hipStream_t st,
                    HostPool* pool, uint64_t** keys_out, skm_stored_kmer_data** data_out, HandoffStats* stats,
                    uint64_t max_chunk) {
    auto now = [] { return std::chrono::steady_clock::now(); };
    const auto t0 = now();
    uint64_t* hk = (uint64_t*)host_alloc(8 * n);
    skm_stored_kmer_data* hd = (skm_stored_kmer_data*)host_alloc(sizeof(skm_stored_kmer_data) * n);
    if (!hk || !hd) {
        std::free(hk);
        std::free(hd);
        throw Error(SKM_E_OOM, "host allocation failed");
    }
    *keys_out = hk;
    *data_out = hd;
    HandoffStats S;
    S.n = n;
    if (n == 0) {
        if (stats) *stats = S;
        return;
    }
    // 1. histogram and the chunk plan: the chunk's device scratch is the sort pairs in and out, the
    // double-buffered gather and the radix sort's temporary ~ one more pair array
    DevBuf d_cur;
    d_cur.ensure(8);
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(ceil_div(n, OUT_THREADS), 2048));
    const uint64_t per = 2 * (8 + sizeof(IdxT)) + 2 * (8 + sizeof(skm_stored_kmer_data)) + (8 + sizeof(IdxT));
    uint64_t cmax = 0;
    const std::vector<Chunk> chunks = plan_chunks(dkeys, n, st, grid, per, max_chunk, cmax);
    S.chunks = chunks.size();
    S.max_chunk = cmax;
    // 2. device scratch for the largest chunk; double-buffered gather output
    DevBuf kin, kout, vin, vout, tmp, gk[2], gd[2];
    kin.ensure(8 * cmax);
    kout.ensure(8 * cmax);
    vin.ensure(sizeof(IdxT) * cmax);
    vout.ensure(sizeof(IdxT) * cmax);
    size_t tmp_bytes = 0;
    SKM_HIP(rocprim::radix_sort_pairs(nullptr, tmp_bytes, kin.as<uint64_t>(), kout.as<uint64_t>(), vin.as<IdxT>(),
                                      vout.as<IdxT>(), (size_t)cmax, 0, KEY_BITS, st));
    tmp.ensure(std::max<size_t>(tmp_bytes, 16));
    for (int k = 0; k < 2; ++k) {
        gk[k].ensure(8 * cmax);
        gd[k].ensure(sizeof(skm_stored_kmer_data) * cmax + 16);
    }
    // pinned staging ring and the copy stream
    constexpr size_t PIECE = 64ull << 20;
    uint8_t* pin[2] = {nullptr, nullptr};
    hipStream_t cs = nullptr;
    hipEvent_t ev_g[2] = {}, ev_d[2] = {}, ev_p[2] = {};
    // timing: per chunk (start, selected, sorted, gathered) on st; per piece (start, end) on cs
    std::vector<hipEvent_t> tev;
    auto tmark = [&](hipStream_t s_) -> size_t {
        hipEvent_t e;
        SKM_HIP(hipEventCreate(&e));
        tev.push_back(e);
        SKM_HIP(hipEventRecord(e, s_));
        return tev.size() - 1;
    };
    std::vector<size_t> cmark, pmark;
    auto cleanup = [&]() {
        if (cs) (void)hipStreamSynchronize(cs);
        (void)hipStreamSynchronize(st);
        for (auto* p : pin)
            if (p) (void)hipHostFree(p);
        for (auto* set : {ev_g, ev_d, ev_p})
            for (int k = 0; k < 2; ++k)
                if (set[k]) (void)hipEventDestroy(set[k]);
        for (auto e : tev) (void)hipEventDestroy(e);
        if (cs) (void)hipStreamDestroy(cs);
    };
    try {
        const auto ta = now();
        for (int k = 0; k < 2; ++k) {
            SKM_HIP(hipHostMalloc(reinterpret_cast<void**>(&pin[k]), PIECE, hipHostMallocDefault));
            SKM_HIP(hipEventCreateWithFlags(&ev_g[k], hipEventDisableTiming));
            SKM_HIP(hipEventCreateWithFlags(&ev_d[k], hipEventDisableTiming));
            SKM_HIP(hipEventCreateWithFlags(&ev_p[k], hipEventDisableTiming));
        }
        SKM_HIP(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
        S.setup_s = std::chrono::duration<double>(now() - ta).count();
        auto enqueue_chunk = [&](size_t c) {  // select -> sort -> gather into buffer c & 1
            const Chunk& C = chunks[c];
            const int k = (int)(c & 1);
            if (c >= 2) SKM_HIP(hipStreamWaitEvent(st, ev_d[k], 0));  // chunk c-2 has left gk/gd[k]
            cmark.push_back(tmark(st));
            SKM_HIP(hipMemsetAsync(d_cur.p, 0, 8, st));
            hipLaunchKernelGGL(k_out_select<IdxT>, dim3(grid), dim3(OUT_THREADS), 0, st, dkeys, n, C.lo, C.hi,
                               d_cur.as<unsigned long long>(), kin.as<uint64_t>(), vin.as<IdxT>());
            SKM_HIP(hipGetLastError());
            tmark(st);
            size_t tb = tmp.bytes;
            SKM_HIP(rocprim::radix_sort_pairs(tmp.p, tb, kin.as<uint64_t>(), kout.as<uint64_t>(), vin.as<IdxT>(),
                                              vout.as<IdxT>(), (size_t)C.n, 0, KEY_BITS, st));
            tmark(st);
            const uint32_t gg = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(ceil_div(C.n, OUT_THREADS), 4096));
            hipLaunchKernelGGL(k_out_gather<IdxT>, dim3(gg), dim3(OUT_THREADS), 0, st, dkeys, ddata, vout.as<IdxT>(), C.n,
                               gk[k].as<uint64_t>(), gd[k].as<skm_stored_kmer_data>());
            SKM_HIP(hipGetLastError());
            tmark(st);
            SKM_HIP(hipEventRecord(ev_g[k], st));
        };
        // the pieces: each chunk's keys, then its records, in 64 MB pieces
        struct Piece {
            size_t chunk;
            const uint8_t* src;
            uint8_t* dst;
            size_t bytes;
            bool first, last;
        };
        std::vector<Piece> pieces;
        for (size_t c = 0; c < chunks.size(); ++c) {
            const int k = (int)(c & 1);
            const size_t first = pieces.size();
            const std::pair<const uint8_t*, uint8_t*> seg[2] = {
                {gk[k].as<uint8_t>(), reinterpret_cast<uint8_t*>(hk + chunks[c].at)},
                {gd[k].as<uint8_t>(), reinterpret_cast<uint8_t*>(hd + chunks[c].at)}};
            const size_t bytes[2] = {8 * chunks[c].n, sizeof(skm_stored_kmer_data) * chunks[c].n};
            for (int s = 0; s < 2; ++s)
                for (size_t o = 0; o < bytes[s]; o += PIECE)
                    pieces.push_back({c, seg[s].first + o, seg[s].second + o, std::min(PIECE, bytes[s] - o), false, false});
            pieces[first].first = true;
            pieces.back().last = true;
        }
        size_t enq = 0;
        auto issue = [&](size_t p) {  // D2H of piece p into pin[p & 1] on the copy stream
            const Piece& P = pieces[p];
            if (P.first) {
                while (enq <= P.chunk + 1 && enq < chunks.size()) enqueue_chunk(enq++);  // keep the sorter one ahead
                SKM_HIP(hipStreamWaitEvent(cs, ev_g[P.chunk & 1], 0));
            }
            pmark.push_back(tmark(cs));
            SKM_HIP(hipMemcpyAsync(pin[p & 1], P.src, P.bytes, hipMemcpyDeviceToHost, cs));
            tmark(cs);
            SKM_HIP(hipEventRecord(ev_p[p & 1], cs));
            if (P.last) SKM_HIP(hipEventRecord(ev_d[P.chunk & 1], cs));
        };
        const int T = pool ? pool->threads() : 1;
        issue(0);
        for (size_t p = 0; p < pieces.size(); ++p) {
            if (p + 1 < pieces.size()) issue(p + 1);  // pin[(p+1) & 1] was drained by the last iteration
            const auto tw = now();
            SKM_HIP(hipEventSynchronize(ev_p[p & 1]));
            S.wait_s += std::chrono::duration<double>(now() - tw).count();
            const auto tc = now();
            const Piece& P = pieces[p];
            const uint8_t* src = pin[p & 1];
            const int parts = (int)std::max<size_t>(1, std::min<size_t>((size_t)T * 2, P.bytes >> 20));
            auto cp = [&](int q) {
                const size_t a = P.bytes * (size_t)q / (size_t)parts, e = P.bytes * (size_t)(q + 1) / (size_t)parts;
                std::memcpy(P.dst + a, src + a, e - a);
            };
            if (pool)
                pool->run(parts, cp);
            else
                for (int q = 0; q < parts; ++q) cp(q);
            S.copy_s += std::chrono::duration<double>(now() - tc).count();
            S.bytes += P.bytes;
        }
        SKM_HIP(hipStreamSynchronize(cs));
        SKM_HIP(hipStreamSynchronize(st));
        float ms = 0;
        for (size_t m : cmark) {
            SKM_HIP(hipEventElapsedTime(&ms, tev[m], tev[m + 1]));
            S.select_ms += ms;
            SKM_HIP(hipEventElapsedTime(&ms, tev[m + 1], tev[m + 2]));
            S.sort_ms += ms;
            SKM_HIP(hipEventElapsedTime(&ms, tev[m + 2], tev[m + 3]));
            S.gather_ms += ms;
        }
        for (size_t m : pmark) {
            SKM_HIP(hipEventElapsedTime(&ms, tev[m], tev[m + 1]));
            S.d2h_ms += ms;
        }
    } catch (...) {
        cleanup();
        throw;
    }
    cleanup();
    S.total_s = std::chrono::duration<double>(now() - t0).count();
    if (stats) *stats = S;
}

}  // namespace

void kept_handoff(const uint64_t* dkeys, const skm_stored_kmer_data* ddata, uint64_t n, hipStream_t st,
                  HostPool* pool, uint64_t** keys_out, skm_stored_kmer_data** data_out, HandoffStats* stats,
                  uint64_t index_limit, uint64_t max_chunk) {
    // index_limit (test hook, 0 = 2^32): hand-offs of at least that many k-mers take u64 arena indices
    const uint64_t lim = index_limit ? index_limit : (1ull << 32);
    if (n < lim)
        kept_handoff_t<uint32_t>(dkeys, ddata, n, st, pool, keys_out, data_out, stats, max_chunk ? max_chunk : ~0ull);
    else
        kept_handoff_t<uint64_t>(dkeys, ddata, n, st, pool, keys_out, data_out, stats, max_chunk ? max_chunk : ~0ull);
    if (stats) stats->wide_index = n >= lim ? 1 : 0;
}

namespace {

// bytes [0, len) of src to fd at file offset off, split over the pool; false (errno in *err) on failure
bool pwrite_all(HostPool* pool, int fd, const uint8_t* src, size_t len, uint64_t off, int* err) {
    const int T = pool ? pool->threads() : 1;
    const int parts = (int)std::max<size_t>(1, std::min<size_t>((size_t)T * 2, len >> 20));
    std::atomic<int> bad{0};
    auto wr = [&](int q) {
        size_t a = len * (size_t)q / (size_t)parts;
        const size_t e = len * (size_t)(q + 1) / (size_t)parts;
        while (a < e) {
            const ssize_t r = ::pwrite(fd, src + a, e - a, (off_t)(off + a));
            if (r < 0 && errno == EINTR) continue;
            if (r <= 0) {
                bad.store(r < 0 ? errno : EIO);
                return;
            }
            a += (size_t)r;
        }
    };
    if (pool && parts > 1)
        pool->run(parts, wr);
    else
        for (int q = 0; q < parts; ++q) wr(q);
    *err = bad.load();
    return *err == 0;
}

template <class IdxT>
void final_kmers_write_t(const uint64_t* dkeys, const skm_stored_kmer_data* ddata, uint64_t n, hipStream_t st,
                         HostPool* pool, int fd, const char* path, skm_final_kmers_stats& S, uint64_t max_chunk,
                         uint64_t piece_bytes) {
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto since = [&](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double>(now() - t).count(); };
    // 1. the hand-off's histogram and chunk plan.  A chunk's device scratch per k-mer: the sort pairs
    // in and out, the radix sort's temporary ~ one more pair array, and the two text buffers at the
    // longest line (no gathered keys or records: k_fk_emit reads through the sorted index); the
    // tile sizes and offsets are 12 bytes per FK_LINES lines
    DevBuf d_cur;
    d_cur.ensure(8);
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(ceil_div(n, OUT_THREADS), 2048));
    const uint64_t per = 3 * (8 + sizeof(IdxT)) + 2 * FK_MAX_LINE + 1;
    uint64_t cmax = 0;
    const std::vector<Chunk> chunks = plan_chunks(dkeys, n, st, grid, per, max_chunk, cmax);
    S.chunks = chunks.size();
    // 2. device scratch for the largest chunk; double-buffered text
    const uint64_t tmax = ceil_div(cmax, FK_LINES), tcap = (uint64_t)FK_MAX_LINE * cmax;
    DevBuf kin, kout, vin, vout, tmp, d_tlen, d_toff, txt[2];
    Scanner scan;
    kin.ensure(8 * cmax);
    kout.ensure(8 * cmax);
    vin.ensure(sizeof(IdxT) * cmax);
    vout.ensure(sizeof(IdxT) * cmax);
    size_t tmp_bytes = 0;
    SKM_HIP(rocprim::radix_sort_pairs(nullptr, tmp_bytes, kin.as<uint64_t>(), kout.as<uint64_t>(), vin.as<IdxT>(),
                                      vout.as<IdxT>(), (size_t)cmax, 0, KEY_BITS, st));
    tmp.ensure(std::max<size_t>(tmp_bytes, 16));
    d_tlen.ensure(4 * tmax);
    d_toff.ensure(8 * (tmax + 1));
    scan.tiles.ensure(8 * tmax);  // (no reallocation between chunks)
    scan.total.ensure(8);
    for (int k = 0; k < 2; ++k) txt[k].ensure(tcap + 16);
    // pinned pieces (no larger than a chunk's text can be), the chunks' text sizes, the copy stream
    const size_t PIECE = (size_t)std::min<uint64_t>(piece_bytes ? piece_bytes : (64ull << 20), std::max<uint64_t>(tcap, 4096));
    uint8_t* pin[2] = {nullptr, nullptr};
    uint64_t* h_tot = nullptr;
    hipStream_t cs = nullptr;
    hipEvent_t ev_g[2] = {}, ev_d[2] = {}, ev_p[2] = {};
    // timing: per chunk (start, selected, sorted, formatted) on st; per piece (start, end) on cs
    std::vector<hipEvent_t> tev;
    auto tmark = [&](hipStream_t s_) -> size_t {
        hipEvent_t e;
        SKM_HIP(hipEventCreate(&e));
        tev.push_back(e);
        SKM_HIP(hipEventRecord(e, s_));
        return tev.size() - 1;
    };
    std::vector<size_t> cmark, pmark;
    auto cleanup = [&]() {
        if (cs) (void)hipStreamSynchronize(cs);
        (void)hipStreamSynchronize(st);
        for (auto* p : pin)
            if (p) (void)hipHostFree(p);
        if (h_tot) (void)hipHostFree(h_tot);
        for (auto* set : {ev_g, ev_d, ev_p})
            for (int k = 0; k < 2; ++k)
                if (set[k]) (void)hipEventDestroy(set[k]);
        for (auto e : tev) (void)hipEventDestroy(e);
        if (cs) (void)hipStreamDestroy(cs);
    };
    try {
        for (int k = 0; k < 2; ++k) {
            SKM_HIP(hipHostMalloc(reinterpret_cast<void**>(&pin[k]), PIECE, hipHostMallocDefault));
            SKM_HIP(hipEventCreateWithFlags(&ev_g[k], hipEventDisableTiming));
            SKM_HIP(hipEventCreateWithFlags(&ev_d[k], hipEventDisableTiming));
            SKM_HIP(hipEventCreateWithFlags(&ev_p[k], hipEventDisableTiming));
        }
        SKM_HIP(hipHostMalloc(reinterpret_cast<void**>(&h_tot), 8 * chunks.size(), hipHostMallocDefault));
        SKM_HIP(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
        auto enqueue_chunk = [&](size_t c) {  // select -> sort -> sizes -> scan -> text into buffer c & 1
            const Chunk& C = chunks[c];
            const int k = (int)(c & 1);
            if (c >= 2) SKM_HIP(hipStreamWaitEvent(st, ev_d[k], 0));  // chunk c-2 has left txt[k]
            cmark.push_back(tmark(st));
            SKM_HIP(hipMemsetAsync(d_cur.p, 0, 8, st));
            hipLaunchKernelGGL(k_out_select<IdxT>, dim3(grid), dim3(OUT_THREADS), 0, st, dkeys, n, C.lo, C.hi,
                               d_cur.as<unsigned long long>(), kin.as<uint64_t>(), vin.as<IdxT>());
            SKM_HIP(hipGetLastError());
            tmark(st);
            size_t tb = tmp.bytes;
            SKM_HIP(rocprim::radix_sort_pairs(tmp.p, tb, kin.as<uint64_t>(), kout.as<uint64_t>(), vin.as<IdxT>(),
                                              vout.as<IdxT>(), (size_t)C.n, 0, KEY_BITS, st));
            tmark(st);
            const uint64_t nt = ceil_div(C.n, FK_LINES);
            hipLaunchKernelGGL(k_fk_len<IdxT>, dim3((uint32_t)nt), dim3(FK_THREADS), 0, st, ddata, n, vout.as<IdxT>(), C.n,
                               d_tlen.as<uint32_t>());
            SKM_HIP(hipGetLastError());
            scan.run(d_tlen.as<uint32_t>(), nt, d_toff.as<uint64_t>(), st);
            hipLaunchKernelGGL(k_fk_emit<IdxT>, dim3((uint32_t)nt), dim3(FK_THREADS), 0, st, dkeys, ddata, n,
                               vout.as<IdxT>(), C.n, d_toff.as<uint64_t>(), txt[k].as<uint8_t>(), tcap);
            SKM_HIP(hipGetLastError());
            tmark(st);
            // the chunk's text bytes: the 8 bytes the host reads per chunk (its file offsets)
            SKM_HIP(hipMemcpyAsync(h_tot + c, d_toff.as<uint64_t>() + nt, 8, hipMemcpyDeviceToHost, st));
            SKM_HIP(hipEventRecord(ev_g[k], st));
        };
        // at most two pieces in flight, one per pinned buffer; the older one is written to the file
        // while the newer one's copy runs
        struct Fly {
            int slot;
            size_t bytes;
            uint64_t off;
        };
        Fly fly[2];
        size_t nfly = 0, np = 0;
        auto drain = [&]() {  // the oldest piece in flight: wait for its copy, write it
            const Fly f = fly[0];
            fly[0] = fly[1];
            --nfly;
            const auto tw = now();
            SKM_HIP(hipEventSynchronize(ev_p[f.slot]));
            S.wait_s += since(tw);
            const auto tc = now();
            int err = 0;
            const bool ok = pwrite_all(pool, fd, pin[f.slot], f.bytes, f.off, &err);
            S.write_s += since(tc);
            if (!ok) throw Error(SKM_E_IO, std::string("cannot write ") + path + ": " + std::strerror(err));
        };
        uint64_t file_off = 0;
        enqueue_chunk(0);
        for (size_t c = 0; c < chunks.size(); ++c) {
            const int k = (int)(c & 1);
            if (c + 1 < chunks.size()) enqueue_chunk(c + 1);  // keep the sorter one ahead
            const auto tw = now();
            SKM_HIP(hipEventSynchronize(ev_g[k]));
            S.wait_s += since(tw);
            const uint64_t tot = h_tot[c];
            SKM_CHECK(tot >= FK_MIN_LINE * chunks[c].n && tot <= tcap, SKM_E_STATE,
                      "final.kmers: a chunk's text size is out of range");
            SKM_HIP(hipStreamWaitEvent(cs, ev_g[k], 0));
            for (uint64_t o = 0; o < tot; o += PIECE) {
                if (nfly == 2) drain();  // frees pin[np & 1]
                const int slot = (int)(np & 1);
                const size_t bytes = (size_t)std::min<uint64_t>(PIECE, tot - o);
                pmark.push_back(tmark(cs));
                SKM_HIP(hipMemcpyAsync(pin[slot], txt[k].as<uint8_t>() + o, bytes, hipMemcpyDeviceToHost, cs));
                tmark(cs);
                SKM_HIP(hipEventRecord(ev_p[slot], cs));
                fly[nfly++] = Fly{slot, bytes, file_off + o};
                ++np;
            }
            SKM_HIP(hipEventRecord(ev_d[k], cs));
            file_off += tot;
        }
        while (nfly) drain();
        SKM_HIP(hipStreamSynchronize(cs));
        SKM_HIP(hipStreamSynchronize(st));
        S.bytes = file_off;
        S.pieces = np;
        float ms = 0;
        for (size_t m : cmark) {
            SKM_HIP(hipEventElapsedTime(&ms, tev[m], tev[m + 1]));
            S.select_ms += ms;
            SKM_HIP(hipEventElapsedTime(&ms, tev[m + 1], tev[m + 2]));
            S.sort_ms += ms;
            SKM_HIP(hipEventElapsedTime(&ms, tev[m + 2], tev[m + 3]));
            S.format_ms += ms;
        }
        for (size_t m : pmark) {
            SKM_HIP(hipEventElapsedTime(&ms, tev[m], tev[m + 1]));
            S.d2h_ms += ms;
        }
    } catch (...) {
        cleanup();
        throw;
    }
    cleanup();
}

}  // namespace

void final_kmers_write(const uint64_t* dkeys, const skm_stored_kmer_data* ddata, uint64_t n, hipStream_t st,
                       HostPool* pool, int fd, const char* path, skm_final_kmers_stats* stats, uint64_t index_limit,
                       uint64_t max_chunk, uint64_t piece_bytes) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t lim = index_limit ? index_limit : (1ull << 32);
    skm_final_kmers_stats S{};
    S.n_kmers = n;
    S.wide_index = n >= lim ? 1u : 0u;
    if (n) {
        if (n < lim)
            final_kmers_write_t<uint32_t>(dkeys, ddata, n, st, pool, fd, path, S, max_chunk ? max_chunk : ~0ull, piece_bytes);
        else
            final_kmers_write_t<uint64_t>(dkeys, ddata, n, st, pool, fd, path, S, max_chunk ? max_chunk : ~0ull, piece_bytes);
    }
    S.total_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (stats) *stats = S;
}

}  // namespace skm

using namespace skm;

int skm_final_kmers_info(uint32_t out[4]) {
    if (!out) return SKM_E_ARG;
    out[0] = FK_LINES;
    out[1] = FK_THREADS;
    out[2] = FK_MAX_LINE;
    out[3] = 0;
    return SKM_OK;
}

int skm_debug_final_kmers_host(const uint64_t* keys, const skm_stored_kmer_data* data, size_t n, uint8_t* out,
                               size_t cap, uint64_t* len) {
    SKM_API_BEGIN
    SKM_CHECK(len && ((keys && data) || n == 0) && (out || cap == 0), SKM_E_ARG, "null argument");
    uint64_t at = 0;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t l = fk_line_len(data[i].avg_from_end, data[i].function_index);
        if (at + l <= cap) fk_write_line(out + at, keys[i], data[i].avg_from_end, data[i].function_index);
        at += l;
    }
    *len = at;
    SKM_API_END
}
