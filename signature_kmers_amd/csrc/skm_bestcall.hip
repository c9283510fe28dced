// skm_bestcall.hip -- find_best_call (call_functions.tcc:347-659) for a batch: the function-index
// tables (skm_fidx), the kernel over a resident CSR of calls, and the host batch function.  The
// decision itself is skm_bestcall.h, shared by both; sequences it declines go through
// skm_find_best_call (skm_host.cpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "skm_bestcall.h"
#include "skm_strutil.h"
#include "skm_util.h"

using namespace skm;

struct skm_fidx {
    std::vector<std::string> names;   // [nfunc]
    std::vector<const char*> cnames;  // the same, for skm_find_best_call
    std::vector<BestFunc> ent;        // [nfunc + 1]
    size_t max_name = 0;
    int device = -1;
    DevBuf d_ent;
    BestTables host() const { return BestTables{ent.data(), (uint32_t)names.size()}; }
    BestTables dev() const { return BestTables{d_ent.as<BestFunc>(), (uint32_t)names.size()}; }
};

namespace {

constexpr int BC_BLOCK = 256;

// one lane per sequence: most sequences have 0-3 calls, the lists live in global scratch that the
// call offsets already partition (sequence s owns work[call_off[s], call_off[s + 1]))
__global__ __launch_bounds__(BC_BLOCK) void k_best_calls(const skm_kmer_call* __restrict__ calls,
                                                         const uint64_t* __restrict__ call_off, uint32_t n_seqs,
                                                         skm_kmer_call* __restrict__ work, BestTables tb,
                                                         skm_best_call* __restrict__ best) {
    const uint32_t s = blockIdx.x * BC_BLOCK + threadIdx.x;
    if (s >= n_seqs) return;
    const uint64_t a = call_off[s], b = call_off[s + 1];
    skm_best_call r;
    best_call_one(calls + a, b - a, work + a, tb, &r);
    best[s] = r;
}

std::string fidx_name(const skm_fidx* fx, uint32_t fi) {
    return (fi == SKM_UNDEFINED_FUNCTION || fi >= fx->names.size()) ? std::string() : fx->names[fi];
}

// a sequence the core declined: skm_find_best_call on its calls.  The pair of a "f1 ?? f2" result
// is recovered from the string: the first two functions of the sequence, in ascending index, whose
// names compose it (functions that share a name compose the same string).
void resolve_deferred(const skm_fidx* fx, const skm_kmer_call* calls, size_t n, skm_best_call* out) {
    std::vector<char> buf(2 * fx->max_name + 8);
    skm_best_call r;
    r.fi_a = r.fi_b = SKM_UNDEFINED_FUNCTION;
    r.flags = 0;
    const int rc = skm_find_best_call(calls, n, fx->cnames.data(), fx->names.size(), &r.fi, &r.score, &r.offset,
                                      buf.data(), buf.size());
    SKM_CHECK(rc == SKM_OK, rc, skm_last_error());
    const std::string func(buf.data());
    if (r.fi == SKM_UNDEFINED_FUNCTION && !func.empty()) {
        std::vector<uint16_t> fs;
        for (size_t i = 0; i < n; ++i) fs.push_back(calls[i].function_index);
        std::sort(fs.begin(), fs.end());
        fs.erase(std::unique(fs.begin(), fs.end()), fs.end());
        for (uint16_t a : fs)
            for (uint16_t b : fs)
                if (a != b && !(r.flags & SKM_BEST_PAIR) && fidx_name(fx, a) + " ?? " + fidx_name(fx, b) == func) {
                    r.fi_a = a;
                    r.fi_b = b;
                    r.flags = SKM_BEST_PAIR;
                }
        SKM_CHECK(r.flags & SKM_BEST_PAIR, SKM_E_STATE, "deferred best call: the pair of '" + func + "' was not found");
    }
    *out = r;
}

void best_alloc(skm_best_calls* out, uint64_t n_seqs) {
    std::memset(out, 0, sizeof(*out));
    out->best = (skm_best_call*)std::malloc(sizeof(skm_best_call) * std::max<uint64_t>(n_seqs, 1));
    SKM_CHECK(out->best, SKM_E_OOM, "host allocation failed");
    out->n_seqs = n_seqs;
}

void launch_best(const skm_kmer_call* d_calls, const uint64_t* d_call_off, uint64_t n_seqs, uint64_t n_calls,
                 const skm_fidx* fx, hipStream_t st, BestWork& w, skm_best_call* h_best, float* ms) {
    *ms = 0.0f;
    if (!n_seqs) return;
    w.d_work.ensure(sizeof(skm_kmer_call) * std::max<uint64_t>(n_calls, 1));
    w.d_best.ensure(sizeof(skm_best_call) * n_seqs);
    if (!w.ev[0]) {
        SKM_HIP(hipEventCreate(&w.ev[0]));
        SKM_HIP(hipEventCreate(&w.ev[1]));
    }
    SKM_HIP(hipEventRecord(w.ev[0], st));
    hipLaunchKernelGGL(k_best_calls, dim3((uint32_t)ceil_div(n_seqs, BC_BLOCK)), dim3(BC_BLOCK), 0, st, d_calls, d_call_off,
                       (uint32_t)n_seqs, w.d_work.as<skm_kmer_call>(), fx->dev(), w.d_best.as<skm_best_call>());
    SKM_HIP(hipGetLastError());
    SKM_HIP(hipEventRecord(w.ev[1], st));
    SKM_HIP(hipMemcpyAsync(h_best, w.d_best.p, sizeof(skm_best_call) * n_seqs, hipMemcpyDeviceToHost, st));
    SKM_HIP(hipStreamSynchronize(st));
    SKM_HIP(hipEventElapsedTime(ms, w.ev[0], w.ev[1]));
}

}  // namespace

namespace skm {

BestWork::~BestWork() {
    for (auto& e : ev)
        if (e) (void)hipEventDestroy(e);
}

void best_calls_check(const skm_fidx* fx, int device) {
    SKM_CHECK(fx->device >= 0, SKM_E_ARG, "the function-index tables were made without a device (skm_fidx_create device < 0)");
    SKM_CHECK(fx->device == device, SKM_E_ARG, "the function-index tables were made for another device than the query's");
}

void best_calls_into(const skm_kmer_call* d_calls, const uint64_t* d_call_off, uint64_t n_seqs, uint64_t n_calls,
                     const skm_fidx* fx, int device, hipStream_t st, BestWork& w, skm_best_call* h_best, float* ms,
                     uint64_t* n_deferred) {
    best_calls_check(fx, device);
    SKM_CHECK(n_seqs < 0xFFFFFFFFull, SKM_E_ARG, "too many sequences in one batch");
    launch_best(d_calls, d_call_off, n_seqs, n_calls, fx, st, w, h_best, ms);
    uint64_t nd = 0;
    for (uint64_t s = 0; s < n_seqs; ++s) nd += (h_best[s].flags & SKM_BEST_DEFERRED) != 0;
    if (nd) {  // only now are calls downloaded: the deferred sequences' own
        std::vector<uint64_t> off(n_seqs + 1);
        SKM_HIP(hipMemcpyAsync(off.data(), d_call_off, 8 * (n_seqs + 1), hipMemcpyDeviceToHost, st));
        SKM_HIP(hipStreamSynchronize(st));
        std::vector<skm_kmer_call> c;
        for (uint64_t s = 0; s < n_seqs; ++s) {
            if (!(h_best[s].flags & SKM_BEST_DEFERRED)) continue;
            c.resize(off[s + 1] - off[s]);
            SKM_HIP(hipMemcpyAsync(c.data(), d_calls + off[s], sizeof(skm_kmer_call) * c.size(), hipMemcpyDeviceToHost, st));
            SKM_HIP(hipStreamSynchronize(st));
            resolve_deferred(fx, c.data(), c.size(), &h_best[s]);
        }
    }
    *n_deferred = nd;
}

void best_calls_resident(const skm_kmer_call* d_calls, const uint64_t* d_call_off, uint64_t n_seqs, uint64_t n_calls,
                         const skm_fidx* fx, int device, hipStream_t st, BestWork& w, skm_best_calls* out) {
    best_calls_check(fx, device);
    SKM_CHECK(n_seqs < 0xFFFFFFFFull, SKM_E_ARG, "too many sequences in one batch");
    best_alloc(out, n_seqs);
    try {
        out->n_calls = n_calls;
        best_calls_into(d_calls, d_call_off, n_seqs, n_calls, fx, device, st, w, out->best, &out->kernel_ms,
                        &out->n_deferred);
    } catch (...) {
        skm_best_calls_free(out);
        throw;
    }
}

}  // namespace skm

extern "C" {

int skm_fidx_create(skm_fidx** out, const char* const* function_index, size_t nfunc, int device) {
    SKM_API_BEGIN
    SKM_CHECK(out && (function_index || !nfunc), SKM_E_ARG, "null argument");
    SKM_CHECK(nfunc < 0xFFFFFFFFull, SKM_E_ARG, "too many functions");
    std::unique_ptr<skm_fidx> fx(new skm_fidx());
    fx->names.resize(nfunc);
    for (size_t i = 0; i < nfunc; ++i)
        if (function_index[i]) fx->names[i] = function_index[i];
    for (const auto& s : fx->names) {
        fx->cnames.push_back(s.c_str());
        fx->max_name = std::max(fx->max_name, s.size());
    }
    // name ranks: dense, "" always ranked (it is what every index outside the table is called)
    std::map<std::string, uint32_t> rank;
    rank[""] = 0;
    for (const auto& s : fx->names) rank[s] = 0;
    uint32_t r = 0;
    for (auto& kv : rank) kv.second = r++;
    // one string pool for whole names and parts
    std::map<std::string, uint32_t> pool;
    auto id_of = [&](const std::string& s) {
        auto it = pool.find(s);
        if (it == pool.end()) it = pool.emplace(s, (uint32_t)pool.size()).first;
        return it->second;
    };
    fx->ent.resize(nfunc + 1);
    for (size_t i = 0; i <= nfunc; ++i) {
        const std::string name = i < nfunc ? fx->names[i] : std::string();
        BestFunc& e = fx->ent[i];
        std::memset(&e, 0, sizeof(e));
        e.rank = rank[name];
        e.whole = id_of(name);
        const std::vector<std::string> parts = skm_str::split(name, " / ");  // call_functions.tcc:487
        if (parts.size() > SKM_BEST_MAX_PARTS) {
            e.nparts = SKM_BEST_COMPLEX;
        } else {
            e.nparts = (uint32_t)parts.size();
            for (size_t p = 0; p < parts.size(); ++p) e.parts[p] = id_of(parts[p]);
        }
    }
    fx->device = device < 0 ? -1 : device;
    if (device >= 0) {
        SKM_HIP(hipSetDevice(device));
        fx->d_ent.ensure(sizeof(BestFunc) * fx->ent.size());
        SKM_HIP(hipMemcpy(fx->d_ent.p, fx->ent.data(), sizeof(BestFunc) * fx->ent.size(), hipMemcpyHostToDevice));
    }
    *out = fx.release();
    SKM_API_END
}

void skm_fidx_destroy(skm_fidx* fx) {
    if (!fx) return;
    if (fx->device >= 0) (void)hipSetDevice(fx->device);
    delete fx;
}

int skm_best_call_name(const skm_fidx* fx, const skm_best_call* c, char* out, size_t cap) {
    if (!fx || !c || (!out && cap)) {
        set_last_error("null argument");
        return SKM_E_ARG;
    }
    std::string s;
    if (c->flags & SKM_BEST_PAIR)
        s = fidx_name(fx, c->fi_a) + " ?? " + fidx_name(fx, c->fi_b);
    else
        s = fidx_name(fx, c->fi);
    if (cap) {
        const size_t n = std::min(s.size(), cap - 1);
        std::memcpy(out, s.data(), n);
        out[n] = 0;
    }
    return (int)s.size();
}

int skm_best_calls_host(const skm_calls* calls, const skm_fidx* fx, int n_threads, skm_best_calls* out) {
    SKM_API_BEGIN
    SKM_CHECK(calls && fx && out, SKM_E_ARG, "null argument");
    SKM_CHECK(calls->call_off && (calls->calls || !calls->n_calls), SKM_E_ARG, "null array");
    const uint64_t ns = calls->n_seqs;
    SKM_CHECK(calls->call_off[0] == 0 && calls->call_off[ns] == calls->n_calls, SKM_E_ARG, "call_off does not span the calls");
    for (uint64_t s = 0; s < ns; ++s)
        SKM_CHECK(calls->call_off[s] <= calls->call_off[s + 1], SKM_E_ARG, "call_off does not ascend");
    best_alloc(out, ns);
    out->n_calls = calls->n_calls;
    out->n_windows = calls->n_windows;
    try {
        std::vector<skm_kmer_call> work(std::max<uint64_t>(calls->n_calls, 1));
        const BestTables tb = fx->host();
        const int nt = (int)std::max<uint64_t>(1, std::min<uint64_t>(n_threads < 1 ? 1 : n_threads, ceil_div(ns, 4096)));
        std::atomic<uint64_t> next(0), deferred(0);
        std::atomic<int> err(SKM_OK);
        std::string err_msg;
        auto body = [&]() {
            try {
                uint64_t nd = 0;
                for (;;) {
                    const uint64_t lo = next.fetch_add(4096), hi = std::min(ns, lo + 4096);
                    if (lo >= ns) break;
                    for (uint64_t s = lo; s < hi; ++s) {
                        const uint64_t a = calls->call_off[s], n = calls->call_off[s + 1] - a;
                        if (!best_call_one(calls->calls + a, n, work.data() + a, tb, &out->best[s])) {
                            resolve_deferred(fx, calls->calls + a, n, &out->best[s]);
                            ++nd;
                        }
                    }
                }
                deferred += nd;
            } catch (const Error& e) {
                if (err.exchange(e.code) == SKM_OK) err_msg = e.what();
            }
        };
        std::vector<std::thread> th;
        for (int t = 1; t < nt; ++t) th.emplace_back(body);
        body();
        for (auto& t : th) t.join();
        SKM_CHECK(err.load() == SKM_OK, err.load(), err_msg);
        out->n_deferred = deferred.load();
    } catch (...) {
        skm_best_calls_free(out);
        throw;
    }
    SKM_API_END
}

int skm_debug_best_calls(const skm_kmer_call* calls, const uint64_t* call_off, size_t n_seqs, const skm_fidx* fx,
                         int device, skm_best_call* best, uint8_t* deferred, float* ms) {
    SKM_API_BEGIN
    SKM_CHECK(fx && call_off && (n_seqs == 0 || (best && deferred)), SKM_E_ARG, "null argument");
    SKM_CHECK(fx->device >= 0 && fx->device == device, SKM_E_ARG, "the function-index tables were not made for this device");
    SKM_CHECK(n_seqs < 0xFFFFFFFFull, SKM_E_ARG, "too many sequences in one batch");
    SKM_CHECK(call_off[0] == 0, SKM_E_ARG, "call_off must start at 0");
    for (size_t s = 0; s < n_seqs; ++s) SKM_CHECK(call_off[s] <= call_off[s + 1], SKM_E_ARG, "call_off does not ascend");
    const uint64_t nc = call_off[n_seqs];
    SKM_CHECK(calls || !nc, SKM_E_ARG, "null calls");
    SKM_HIP(hipSetDevice(device));
    DevBuf d_calls, d_off;
    BestWork w;
    d_calls.ensure(sizeof(skm_kmer_call) * std::max<uint64_t>(nc, 1));
    d_off.ensure(8 * (n_seqs + 1));
    if (nc) SKM_HIP(hipMemcpy(d_calls.p, calls, sizeof(skm_kmer_call) * nc, hipMemcpyHostToDevice));
    SKM_HIP(hipMemcpy(d_off.p, call_off, 8 * (n_seqs + 1), hipMemcpyHostToDevice));
    float t = 0.0f;
    launch_best(d_calls.as<skm_kmer_call>(), d_off.as<uint64_t>(), n_seqs, nc, fx, nullptr, w, best, &t);
    for (size_t s = 0; s < n_seqs; ++s) {
        deferred[s] = (best[s].flags & SKM_BEST_DEFERRED) != 0;
        best[s].flags &= (uint16_t)~SKM_BEST_DEFERRED;
    }
    if (ms) *ms = t;
    SKM_API_END
}

void skm_best_calls_free(skm_best_calls* c) {
    if (!c) return;
    std::free(c->best);
    std::memset(c, 0, sizeof(*c));
}

}  // extern "C"
