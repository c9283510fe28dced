// skm_util.h -- error plumbing and small device helpers shared by libskm translation units.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>
#include <string>

#include "../../include/skm.h"

namespace skm {

// Internal errors are C++ exceptions carrying an SKM_E_* code; every extern "C" entry point
// catches them (SKM_API_BEGIN/END) so nothing crosses the C boundary.
struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

void set_last_error(const std::string& msg);

#define SKM_HIP(call)                                                                               \
    do {                                                                                            \
        hipError_t _e = (call);                                                                     \
        if (_e != hipSuccess)                                                                       \
            throw ::skm::Error(_e == hipErrorOutOfMemory ? SKM_E_OOM : SKM_E_HIP,                   \
                               std::string(#call) + ": " + hipGetErrorString(_e));                  \
    } while (0)

#define SKM_CHECK(cond, code, msg)                           \
    do {                                                     \
        if (!(cond)) throw ::skm::Error((code), (msg));      \
    } while (0)

#define SKM_API_BEGIN try {
#define SKM_API_END                                          \
    }                                                        \
    catch (const ::skm::Error& e) {                          \
        ::skm::set_last_error(e.what());                     \
        return e.code;                                       \
    }                                                        \
    catch (const std::bad_alloc&) {                          \
        ::skm::set_last_error("host allocation failed");     \
        return SKM_E_OOM;                                    \
    }                                                        \
    catch (const std::exception& e) {                        \
        ::skm::set_last_error(e.what());                     \
        return SKM_E_ARG;                                    \
    }                                                        \
    return SKM_OK;

// RAII device buffer (hipMalloc).  Grows but never shrinks.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    void ensure(size_t n) {
        if (n <= bytes && p) return;
        if (p) SKM_HIP(hipFree(p));
        p = nullptr;
        bytes = 0;
        size_t alloc = n ? n : 16;
        SKM_HIP(hipMalloc(&p, alloc));
        bytes = alloc;
    }
    void release() {
        if (p) SKM_HIP(hipFree(p));
        p = nullptr;
        bytes = 0;
    }
    template <typename T>
    T* as() const {
        return reinterpret_cast<T*>(p);
    }
};

// hipMalloc of one of the large buffers (a DB made from a build's arena: the range-reduced table,
// the BDZ construction's state and the BDZ DB's arrays; the device FASTA parser's raw bytes and
// residues) into an empty or smaller DevBuf; a failure names the bytes asked for and the bytes free
inline void alloc_reported(DevBuf& buf, uint64_t bytes, const char* what) {
    if (buf.p && bytes <= buf.bytes) return;
    buf.release();
    if (bytes < 16) bytes = 16;
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        size_t fr = 0, tot = 0;
        (void)hipMemGetInfo(&fr, &tot);
        throw Error(e == hipErrorOutOfMemory ? SKM_E_OOM : SKM_E_HIP,
                    std::string(what) + ": " + std::to_string(bytes) + " bytes asked for, " + std::to_string(fr) +
                        " bytes free on the device (" + hipGetErrorString(e) + ")");
    }
    buf.p = p;
    buf.bytes = bytes;
}

// the best-call kernel over a resident CSR of calls (skm_bestcall.hip): scratch for the collapsed
// lists and the results, kept by whoever owns the calls.  best_calls_resident fills *out (best,
// n_seqs, n_calls, n_deferred, kernel_ms), resolving deferred sequences on the host.
struct BestWork {
    DevBuf d_work, d_best;
    hipEvent_t ev[2] = {};
    ~BestWork();
};
void best_calls_resident(const skm_kmer_call* d_calls, const uint64_t* d_call_off, uint64_t n_seqs, uint64_t n_calls,
                         const skm_fidx* fx, int device, hipStream_t st, BestWork& w, skm_best_calls* out);
// the same into a caller's array h_best[n_seqs] (a batch of a larger result: skm_build_recall), and
// the argument check both make first (SKM_E_ARG: fx without device tables, or for another device)
void best_calls_into(const skm_kmer_call* d_calls, const uint64_t* d_call_off, uint64_t n_seqs, uint64_t n_calls,
                     const skm_fidx* fx, int device, hipStream_t st, BestWork& w, skm_best_call* h_best, float* ms,
                     uint64_t* n_deferred);
void best_calls_check(const skm_fidx* fx, int device);

inline uint64_t ceil_div(uint64_t a, uint64_t b) { return (a + b - 1) / b; }
inline int ilog2_ceil(uint64_t x) {
    int b = 0;
    while ((1ull << b) < x) ++b;
    return b;
}

}  // namespace skm
