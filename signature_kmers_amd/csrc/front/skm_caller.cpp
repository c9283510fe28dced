// skm_caller.cpp -- see skm_caller.h.
#include "skm_caller.h"

#include "../skm_strutil.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <fstream>
#include <memory>
#include <mutex>
#include <thread>

namespace skmf {

bool read_function_index(const std::string& path, std::vector<std::string>& table, std::string& err) {
    // call_functions.tcc:123-148: max id over the lines, then function_index_[stoi(parts[0])] =
    // parts[1] with parts = split(line, "\t") (operators.h:80-91).  One read instead of two; a
    // line without a tab (parts[1] out of range in the reference) names the empty string.
    std::ifstream f(path);
    if (!f) {
        err = "cannot read " + path;
        return false;
    }
    std::vector<std::pair<int, std::string>> rows;
    int max_id = 0;
    std::string line;
    while (std::getline(f, line, '\n')) {
        const std::vector<std::string> parts = skm_str::split(line, "\t");
        int id = 0;
        try {
            id = std::stoi(parts[0]);
        } catch (const std::exception&) {
            err = "bad function.index line in " + path + ": '" + line + "'";
            return false;
        }
        if (id < 0) {
            err = "negative function index in " + path + ": '" + line + "'";
            return false;
        }
        max_id = std::max(max_id, id);
        rows.emplace_back(id, parts.size() > 1 ? parts[1] : std::string());
    }
    table.assign((size_t)max_id + 1, std::string());
    for (auto& r : rows) table[(size_t)r.first] = r.second;
    return true;
}

namespace {
int g_mean_mode = 0, g_mad_mode = 0;
}

void set_boost_math_modes(int mean_mode, int mad_mode) {
    g_mean_mode = mean_mode;
    g_mad_mode = mad_mode;
}

bool best_call_tables(const std::string& mode, const std::vector<std::string>& function_index, int device,
                      skm_fidx** fx, std::string& err) {
    *fx = nullptr;
    if (mode == "host") return true;
    if (mode != "device") {
        err = "--best-call must be host or device";
        return false;
    }
    std::vector<const char*> p(function_index.size());
    for (size_t i = 0; i < function_index.size(); ++i) p[i] = function_index[i].c_str();
    if (skm_fidx_create(fx, p.data(), p.size(), device)) {
        err = skm_last_error();
        return false;
    }
    return true;
}

bool annot_opts_for(const std::vector<std::string>& function_index, bool ignore_hypo, skm_annot_opts& o,
                    std::string& err) {
    auto hit = std::find(function_index.begin(), function_index.end(), "hypothetical protein");
    if (hit == function_index.end()) {  // process_aa_seq exits here (call_functions.tcc:269-274)
        err = "Cannot find hypothetical protein index";
        return false;
    }
    o = skm_annot_opts{};
    o.min_hits = 5;
    o.max_gap = 200;
    o.ignore_hypo = ignore_hypo ? 1 : 0;
    o.hypo_index = (int32_t)(hit - function_index.begin());
    o.mean_mode = g_mean_mode;
    o.mad_mode = g_mad_mode;
    return true;
}

namespace {
// a batch packed as skm_annotate lays it out on the device (every sequence followed by a 0, back
// to back), so the library uploads it as it is instead of packing a second copy; files are
// copied by the host threads
struct PackedBatch {
    std::unique_ptr<uint8_t[]> res;
    std::vector<uint64_t> off;
    std::vector<uint32_t> len;
};

void pack_batch(const std::vector<const FastaFile*>& files, int n_threads, PackedBatch& b) {
    std::vector<uint64_t> rbase(files.size() + 1, 0), sbase(files.size() + 1, 0);
    for (size_t f = 0; f < files.size(); ++f) {
        uint64_t nb = 0;
        for (size_t r = 0; r < files[f]->size(); ++r) nb += (uint64_t)files[f]->len[r] + 1;
        rbase[f + 1] = rbase[f] + nb;
        sbase[f + 1] = sbase[f] + files[f]->size();
    }
    b.res.reset(new uint8_t[std::max<uint64_t>(rbase.back(), 1)]);
    b.off.resize(sbase.back());
    b.len.resize(sbase.back());
    std::unique_ptr<uint8_t[]>& res = b.res;
    std::vector<uint64_t>& off = b.off;
    std::vector<uint32_t>& len = b.len;
    std::atomic<size_t> nextf{0};
    auto cp = [&]() {
        for (size_t f; (f = nextf.fetch_add(1)) < files.size();) {
            const FastaFile& F = *files[f];
            uint64_t p = rbase[f];
            for (size_t r = 0; r < F.size(); ++r) {
                std::memcpy(res.get() + p, F.residues.data() + F.off[r], F.len[r]);
                res[p + F.len[r]] = 0;
                off[sbase[f] + r] = p;
                len[sbase[f] + r] = F.len[r];
                p += (uint64_t)F.len[r] + 1;
            }
        }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < std::max(1, std::min<int>(n_threads, (int)files.size())); ++t) th.emplace_back(cp);
    cp();
    for (auto& t : th) t.join();
}

// the device's records against the headers-only host parse, file by file
int check_fasta_table(const skm_fasta_table& tab, const std::vector<const FastaFile*>& files, std::string& err) {
    for (size_t f = 0; f < files.size(); ++f) {
        const uint64_t r0 = tab.file_rec[f], nr = tab.file_rec[f + 1] - r0;
        bool same = nr == files[f]->size();
        for (size_t r = 0; same && r < nr; ++r) same = tab.seq_len[r0 + r] == files[f]->len[r];
        if (!same) {
            err = "device FASTA parse differs from the host parse of " + files[f]->path + " (" + std::to_string(nr) +
                  " records on the device, " + std::to_string(files[f]->size()) + " on the host, or other lengths)";
            return SKM_E_STATE;
        }
    }
    return SKM_OK;
}
}  // namespace

int annotate_batch(skm_db* db, const std::vector<const FastaFile*>& files, const skm_annot_opts& o, int n_threads,
                   skm_calls* calls, std::string& err) {
    *calls = skm_calls{};
    PackedBatch b;
    pack_batch(files, n_threads, b);
    const int rc = skm_annotate(db, b.res.get(), b.off.data(), b.len.data(), b.off.size(), &o, calls);
    if (rc) err = skm_last_error();
    return rc;
}

int annotate_batch_best(skm_db* db, const std::vector<const FastaFile*>& files, const skm_annot_opts& o, int n_threads,
                        const skm_fidx* fx, skm_best_calls* best, std::string& err) {
    *best = skm_best_calls{};
    PackedBatch b;
    pack_batch(files, n_threads, b);
    const int rc = skm_annotate_best(db, b.res.get(), b.off.data(), b.len.data(), b.off.size(), &o, fx, best);
    if (rc) err = skm_last_error();
    return rc;
}

int annotate_batch_fasta(skm_db* db, const std::vector<const FastaFile*>& files, const uint8_t* bytes,
                         const uint64_t* file_off, const skm_annot_opts& o, skm_calls* calls, std::string& err) {
    *calls = skm_calls{};
    skm_fasta_table tab{};
    int rc = skm_annotate_fasta(db, bytes, file_off, files.size(), &o, calls, &tab);
    if (rc) {
        err = skm_last_error();
        return rc;
    }
    rc = check_fasta_table(tab, files, err);
    skm_fasta_table_free(&tab);
    if (rc) skm_calls_free(calls);
    return rc;
}

int annotate_batch_fasta_best(skm_db* db, const std::vector<const FastaFile*>& files, const uint8_t* bytes,
                              const uint64_t* file_off, const skm_annot_opts& o, const skm_fidx* fx, skm_best_calls* best,
                              std::string& err) {
    *best = skm_best_calls{};
    skm_fasta_table tab{};
    int rc = skm_annotate_fasta_best(db, bytes, file_off, files.size(), &o, fx, best, &tab);
    if (rc) {
        err = skm_last_error();
        return rc;
    }
    rc = check_fasta_table(tab, files, err);
    skm_fasta_table_free(&tab);
    if (rc) skm_best_calls_free(best);
    return rc;
}

int best_calls_batch(const skm_calls& calls, const std::vector<const FastaFile*>& files,
                     const std::vector<const char*>& fidx, int n_threads, const std::vector<std::vector<SeqCall>*>& out,
                     std::string& err) {
    std::vector<std::pair<size_t, size_t>> where;  // (file, record) per batch sequence
    for (size_t f = 0; f < files.size(); ++f)
        for (size_t r = 0; r < files[f]->size(); ++r) where.emplace_back(f, r);
    if (where.size() != calls.n_seqs) {
        err = "find_best_call: call list does not match the batch";
        return SKM_E_STATE;
    }
    std::atomic<size_t> next{0};
    std::atomic<int> first_rc{0};
    std::mutex err_mu;  // skm_last_error() is per thread: the failing worker records its own message
    std::string worker_err;
    auto work = [&]() {
        std::vector<char> fb(1 << 16);
        const size_t chunk = 4096;
        for (size_t s0; (s0 = next.fetch_add(chunk)) < where.size();) {
            for (size_t s = s0; s < std::min(where.size(), s0 + chunk); ++s) {
                SeqCall& c = (*out[where[s].first])[where[s].second];
                float offset = 0;
                int r = skm_find_best_call(calls.calls + calls.call_off[s], calls.call_off[s + 1] - calls.call_off[s],
                                           fidx.data(), fidx.size(), &c.fi, &c.score, &offset, fb.data(), fb.size());
                if (r) {
                    std::lock_guard<std::mutex> lk(err_mu);
                    if (!first_rc) {
                        first_rc = r;
                        worker_err = skm_last_error();
                    }
                }
                c.func = fb.data();
            }
        }
    };
    const int nt = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(1, n_threads), where.size() / 4096 + 1));
    std::vector<std::thread> th;
    for (int t = 1; t < nt; ++t) th.emplace_back(work);
    work();
    for (auto& t : th) t.join();
    if (first_rc) err = worker_err.empty() ? std::string("find_best_call failed") : worker_err;
    return first_rc;
}

namespace {
int compose_best_where(const skm_best_calls& best, const std::vector<std::pair<size_t, size_t>>& where, const skm_fidx* fx,
                       int n_threads, const std::vector<std::vector<SeqCall>*>& out, std::string& err);
}

int compose_best_batch(const skm_best_calls& best, const std::vector<const FastaFile*>& files, const skm_fidx* fx,
                       int n_threads, const std::vector<std::vector<SeqCall>*>& out, std::string& err) {
    std::vector<std::pair<size_t, size_t>> where;  // (file, record) per batch sequence
    for (size_t f = 0; f < files.size(); ++f)
        for (size_t r = 0; r < files[f]->size(); ++r) where.emplace_back(f, r);
    return compose_best_where(best, where, fx, n_threads, out, err);
}

namespace {
// best[s] is the call of record where[s].second of file where[s].first
int compose_best_where(const skm_best_calls& best, const std::vector<std::pair<size_t, size_t>>& where, const skm_fidx* fx,
                       int n_threads, const std::vector<std::vector<SeqCall>*>& out, std::string& err) {
    if (where.size() != best.n_seqs) {
        err = "best calls: the result does not match the batch";
        return SKM_E_STATE;
    }
    std::atomic<size_t> next{0};
    std::atomic<int> first_rc{0};
    auto work = [&]() {
        std::vector<char> fb(1 << 16);
        const size_t chunk = 4096;
        for (size_t s0; (s0 = next.fetch_add(chunk)) < where.size();) {
            for (size_t s = s0; s < std::min(where.size(), s0 + chunk); ++s) {
                SeqCall& c = (*out[where[s].first])[where[s].second];
                const skm_best_call& b = best.best[s];
                c.fi = b.fi;
                c.score = b.score;
                if (b.fi == 0xFFFF && !(b.flags & SKM_BEST_PAIR)) {  // name(0xFFFF) is ""
                    c.func.clear();
                    continue;
                }
                int n = skm_best_call_name(fx, &b, fb.data(), fb.size());
                if (n >= (int)fb.size()) {
                    fb.resize((size_t)n + 1);
                    n = skm_best_call_name(fx, &b, fb.data(), fb.size());
                }
                if (n < 0) first_rc = n;
                c.func = fb.data();
            }
        }
    };
    const int nt = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(1, n_threads), where.size() / 4096 + 1));
    std::vector<std::thread> th;
    for (int t = 1; t < nt; ++t) th.emplace_back(work);
    work();
    for (auto& t : th) t.join();
    if (first_rc) err = "skm_best_call_name failed";
    return first_rc;
}
}  // namespace

int call_files_resident(skm_build* b, skm_db* db, const std::vector<const FastaFile*>& files,
                        const std::vector<BuildBatch>& batches, const std::vector<std::string>& function_index,
                        int n_threads, const skm_fidx* fx, std::vector<std::vector<SeqCall>>& out, std::string& err,
                        ResidentRecall* stats, uint64_t max_batch_residues) {
    ResidentRecall st;
    skm_annot_opts o{};
    if (!annot_opts_for(function_index, false, o, err)) return SKM_E_ARG;
    if (batches.size() != files.size()) {
        err = "resident recall: one selection per file is needed";
        return SKM_E_ARG;
    }
    out.assign(files.size(), std::vector<SeqCall>());
    std::vector<std::vector<SeqCall>*> outp;
    for (size_t f = 0; f < files.size(); ++f) {
        out[f].resize(files[f]->size());
        outp.push_back(&out[f]);
    }
    // the resident sequences in add order = the selections in file order; the rest of the records
    std::vector<std::pair<size_t, size_t>> res_where, up_where;
    for (size_t f = 0; f < files.size(); ++f) {
        size_t k = 0;
        const std::vector<uint32_t>& rec = batches[f].rec;
        for (size_t r = 0; r < files[f]->size(); ++r) {
            if (k < rec.size() && rec[k] == r) {
                res_where.emplace_back(f, r);
                ++k;
            } else {
                up_where.emplace_back(f, r);
            }
        }
        if (k != rec.size()) {
            err = "resident recall: the selection of " + files[f]->path + " does not ascend over its records";
            return SKM_E_STATE;
        }
    }
    uint64_t n_res = 0;
    int rc = skm_build_resident_seqs(b, &n_res, nullptr);
    if (!rc && n_res != res_where.size()) {
        err = "resident recall: the build holds " + std::to_string(n_res) + " sequences, the selections name " +
              std::to_string(res_where.size());
        return SKM_E_STATE;
    }
    auto t0 = std::chrono::steady_clock::now();
    skm_best_calls best{};
    skm_recall_stats rs{};
    if (!rc) rc = skm_build_recall(b, db, &o, nullptr, fx, &best, nullptr, &rs);
    st.device_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (rc) {
        err = skm_last_error();
        return rc;
    }
    st.resident_seqs = rs.n_seqs;
    st.batches = rs.n_batches;
    st.deferred = rs.n_deferred;
    rc = compose_best_where(best, res_where, fx, n_threads, outp, err);
    skm_best_calls_free(&best);
    if (rc) return rc;
    // the left-out records, packed as skm_annotate lays a batch out, up to max_batch_residues a batch
    st.uploaded_seqs = up_where.size();
    for (size_t s0 = 0; s0 < up_where.size();) {
        size_t s1 = s0;
        uint64_t bytes = 0;
        while (s1 < up_where.size()) {
            const uint64_t add = (uint64_t)files[up_where[s1].first]->len[up_where[s1].second] + 1;
            if (s1 > s0 && bytes + add > max_batch_residues) break;
            bytes += add;
            ++s1;
        }
        PackedBatch pb;
        pb.res.reset(new uint8_t[std::max<uint64_t>(bytes, 1)]);
        pb.off.resize(s1 - s0);
        pb.len.resize(s1 - s0);
        uint64_t p = 0;
        for (size_t s = s0; s < s1; ++s) {
            const FastaFile& F = *files[up_where[s].first];
            const size_t r = up_where[s].second;
            std::memcpy(pb.res.get() + p, F.residues.data() + F.off[r], F.len[r]);
            pb.res[p + F.len[r]] = 0;
            pb.off[s - s0] = p;
            pb.len[s - s0] = F.len[r];
            p += (uint64_t)F.len[r] + 1;
        }
        t0 = std::chrono::steady_clock::now();
        rc = skm_annotate_best(db, pb.res.get(), pb.off.data(), pb.len.data(), pb.off.size(), &o, fx, &best);
        st.device_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (rc) {
            err = skm_last_error();
            return rc;
        }
        st.deferred += best.n_deferred;
        const std::vector<std::pair<size_t, size_t>> where(up_where.begin() + s0, up_where.begin() + s1);
        rc = compose_best_where(best, where, fx, n_threads, outp, err);
        skm_best_calls_free(&best);
        if (rc) return rc;
        s0 = s1;
    }
    if (stats) *stats = st;
    return SKM_OK;
}

int call_files(skm_db* db, const std::vector<const FastaFile*>& files, const std::vector<std::string>& function_index,
               bool ignore_hypo, int n_threads, std::vector<std::vector<SeqCall>>& out, std::string& err,
               double* device_ms, uint64_t max_batch_residues, double* host_ms, const FastaBytes* raw,
               const skm_fidx* fx, uint64_t* n_deferred) {
    const auto t_begin = std::chrono::steady_clock::now();
    double dev_ms = 0;
    uint64_t deferred = 0;
    skm_annot_opts o{};
    if (!annot_opts_for(function_index, ignore_hypo, o, err)) return SKM_E_ARG;
    std::vector<const char*> fidx(function_index.size());
    for (size_t i = 0; i < function_index.size(); ++i) fidx[i] = function_index[i].c_str();
    out.assign(files.size(), std::vector<SeqCall>());
    for (size_t f = 0; f < files.size(); ++f) out[f].resize(files[f]->size());
    size_t f0 = 0;
    while (f0 < files.size()) {
        // one device batch: whole files up to max_batch_residues residues
        size_t f1 = f0;
        uint64_t nres = 0;
        while (f1 < files.size() && (f1 == f0 || nres + files[f1]->n_residues <= max_batch_residues))
            nres += files[f1++]->n_residues;
        const std::vector<const FastaFile*> batch(files.begin() + f0, files.begin() + f1);
        skm_calls calls{};
        skm_best_calls best{};  // fx: find_best_call on the device too, 16 B per sequence come back
        auto t0 = std::chrono::steady_clock::now();
        int rc;
        if (raw) {  // the batch's files as they lie in raw, their offsets from the first one's start
            std::vector<uint64_t> off(raw->file_off.begin() + f0, raw->file_off.begin() + f1 + 1);
            const uint64_t base = off[0];
            for (auto& x : off) x -= base;
            rc = fx ? annotate_batch_fasta_best(db, batch, raw->bytes.get() + base, off.data(), o, fx, &best, err)
                    : annotate_batch_fasta(db, batch, raw->bytes.get() + base, off.data(), o, &calls, err);
        } else {
            rc = fx ? annotate_batch_best(db, batch, o, n_threads, fx, &best, err)
                    : annotate_batch(db, batch, o, n_threads, &calls, err);
        }
        dev_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (rc) return rc;
        std::vector<std::vector<SeqCall>*> outp;
        for (size_t f = f0; f < f1; ++f) outp.push_back(&out[f]);
        if (fx) {
            deferred += best.n_deferred;
            rc = compose_best_batch(best, batch, fx, n_threads, outp, err);
            skm_best_calls_free(&best);
        } else {
            rc = best_calls_batch(calls, batch, fidx, n_threads, outp, err);
            skm_calls_free(&calls);
        }
        if (rc) return rc;
        f0 = f1;
    }
    if (device_ms) *device_ms = dev_ms;
    if (n_deferred) *n_deferred = deferred;
    if (host_ms)
        *host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count() - dev_ms;
    return SKM_OK;
}

}  // namespace skmf
