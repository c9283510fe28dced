// skm_mdbatch.cpp -- see skm_mdbatch.h
#include "skm_mdbatch.h"

#include <dirent.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstring>
#include <fstream>
#include <iostream>
#include <unordered_map>

#include "skm.h"
#include "skm_front.h"

namespace skmf {

bool path_exists(const std::string& p) {
    struct stat sb;
    return stat(p.c_str(), &sb) == 0;
}
bool is_regular_file(const std::string& p) {
    struct stat sb;
    return stat(p.c_str(), &sb) == 0 && S_ISREG(sb.st_mode);
}
bool is_directory(const std::string& p) {
    struct stat sb;
    return stat(p.c_str(), &sb) == 0 && S_ISDIR(sb.st_mode);
}

std::string quoted_path(const std::string& p) {
    std::string q = "\"";
    for (char c : p) {
        if (c == '"' || c == '&') q += '&';  // boost::io::quoted(string, '&')
        q += c;
    }
    q += '"';
    return q;
}

bool list_directories(const std::string& dir, std::vector<std::string>& out, std::string& err) {
    DIR* d = opendir(dir.c_str());
    if (!d) {
        err = "cannot open directory " + dir;
        return false;
    }
    while (struct dirent* e = readdir(d)) {
        if (!std::strcmp(e->d_name, ".") || !std::strcmp(e->d_name, "..")) continue;
        std::string p = path_join(dir, e->d_name);
        if (is_directory(p)) out.push_back(p);
    }
    closedir(d);
    return true;
}

namespace {

// one problem's records, packed behind the batch's
struct Loaded {
    const MdProblem* prob = nullptr;
    std::string label;                  // comma-joined usable inputs
    std::vector<std::string> index_id;  // SeqIdMap: index -> id
    std::vector<size_t> index_len;      // first record's length
    uint64_t n_seqs = 0, windows = 0;
};

struct Batch {
    std::vector<Loaded> probs;
    std::vector<uint8_t> residues;
    std::vector<uint64_t> off, prob_seq{0};
    std::vector<uint32_t> len, idx, nidx;
    uint64_t windows = 0;
    void clear() { *this = Batch(); }
};

// parse a problem's usable files onto the end of the batch; false: no usable file
bool load_problem(const MdProblem& p, Batch& b, Loaded& L) {
    L.prob = &p;
    std::unordered_map<std::string, uint32_t> id_to_index;
    for (const std::string& in : p.inputs) {
        struct stat sb;
        if (stat(in.c_str(), &sb) != 0 || !S_ISREG(sb.st_mode) || sb.st_size == 0) continue;
        FastaFile f;
        parse_fasta_file(in, f);  // an unreadable file parses as empty (fs::ifstream)
        for (size_t r = 0; r < f.size(); ++r) {
            auto it = id_to_index.find(f.ids[r]);
            if (it == id_to_index.end()) {
                it = id_to_index.emplace(f.ids[r], (uint32_t)L.index_id.size()).first;
                L.index_id.push_back(f.ids[r]);
                L.index_len.push_back(f.len[r]);
            }
            b.off.push_back(b.residues.size());
            b.len.push_back(f.len[r]);
            b.idx.push_back(it->second);
            b.residues.insert(b.residues.end(), f.residues.begin() + f.off[r], f.residues.begin() + f.off[r] + f.len[r]);
            L.windows += (f.len[r] >= 8 ? f.len[r] - 7 : 0) + 1;
            ++L.n_seqs;
        }
        if (!L.label.empty()) L.label += ",";
        L.label += in;
    }
    return !L.label.empty();
}

bool run_batch(skm_db* db, Batch& b, const MdBatchConfig& cfg, std::string& err) {
    if (b.probs.empty()) return true;
    const size_t P = b.probs.size();
    if (b.residues.empty()) b.residues.push_back(0);  // only empty sequences: still a non-null array
    skm_matrix_batch* mb = nullptr;
    if (skm_matrix_batch_create(&mb, db, b.residues.data(), b.off.data(), b.len.data(), b.idx.data(), b.prob_seq.data(),
                                b.nidx.data(), P)) {
        err = skm_last_error();
        return false;
    }
    skm_matrix_batch_opts o;
    std::memset(&o, 0, sizeof(o));
    o.hypo_index = cfg.hypo_index;
    skm_pairs pairs;
    std::memset(&pairs, 0, sizeof(pairs));
    std::vector<uint64_t> prob_off(P + 1, 0), groups(P, 0);
    bool ok = skm_matrix_batch_run(mb, &o) == 0 && skm_matrix_batch_pairs(mb, &pairs, prob_off.data()) == 0 &&
              (!cfg.verbose || skm_matrix_batch_group_counts(mb, groups.data()) == 0);
    if (!ok) err = skm_last_error();
    skm_matrix_batch_destroy(mb);
    // every output under a temporary name first: an existing output file means "done" to the
    // folder tool's resume logic, so none may appear before its batch succeeded
    std::vector<std::string> tmp(P);
    for (size_t p = 0; ok && p < P; ++p) {
        const Loaded& L = b.probs[p];
        if (cfg.verbose) {
            std::cerr << L.label << " Start all to all comparison\n";
            std::cerr << "kmer_hit_map size " << groups[p] << "\n";
            std::cerr << L.label << " all to all done\n";
        }
        tmp[p] = L.prob->output + ".tmp." + std::to_string((long)getpid());
        std::ofstream of(tmp[p], std::ios::binary | std::ios::trunc);
        std::string buf;
        for (uint64_t i = prob_off[p]; i < prob_off[p + 1]; ++i) {
            const uint32_t* t = pairs.pairs + 3 * i;
            buf += L.index_id[t[0]];
            buf += '\t';
            buf += L.index_id[t[1]];
            buf += '\t';
            buf += std::to_string(t[2]);
            buf += '\t';
            buf += md_score_text(t[2], L.index_len[t[0]], L.index_len[t[1]]);
            buf += '\n';
            if (buf.size() > (1u << 20)) {
                of.write(buf.data(), (std::streamsize)buf.size());
                buf.clear();
            }
        }
        of.write(buf.data(), (std::streamsize)buf.size());
        of.close();
        if (!of) {
            err = "cannot write " + tmp[p];
            ok = false;
        }
    }
    for (size_t p = 0; p < P; ++p) {
        if (tmp[p].empty()) continue;
        if (ok && std::rename(tmp[p].c_str(), b.probs[p].prob->output.c_str()) != 0) {
            err = "cannot rename " + tmp[p] + " to " + b.probs[p].prob->output;
            ok = false;
        }
        if (!ok) (void)std::remove(tmp[p].c_str());
    }
    skm_pairs_free(&pairs);
    b.clear();
    return ok;
}

}  // namespace

bool run_matrix_problems(skm_db* db, const std::vector<MdProblem>& work, const MdBatchConfig& cfg, std::string& err) {
    Batch b;
    for (const MdProblem& p : work) {
        Batch one;  // parsed on its own, so a problem that does not fit starts the next batch
        Loaded L;
        if (!load_problem(p, one, L)) {
            if (cfg.verbose) {
                std::cerr << " Start all to all comparison\nkmer_hit_map size 0\n";
                std::cerr << "Skip compute " << quoted_path(p.inputs.empty() ? std::string() : p.inputs[0]) << "\n";
            }
            continue;
        }
        if (!b.probs.empty() && b.windows + L.windows > cfg.batch_windows && !run_batch(db, b, cfg, err)) return false;
        const uint64_t r0 = b.residues.size();
        b.residues.insert(b.residues.end(), one.residues.begin(), one.residues.end());
        for (uint64_t o : one.off) b.off.push_back(r0 + o);
        b.len.insert(b.len.end(), one.len.begin(), one.len.end());
        b.idx.insert(b.idx.end(), one.idx.begin(), one.idx.end());
        b.nidx.push_back((uint32_t)L.index_id.size());
        b.prob_seq.push_back(b.prob_seq.back() + L.n_seqs);
        b.windows += L.windows;
        b.probs.push_back(std::move(L));
    }
    return run_batch(db, b, cfg, err);
}

}  // namespace skmf
