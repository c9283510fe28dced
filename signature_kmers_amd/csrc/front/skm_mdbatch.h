// skm_mdbatch.h -- host front end shared by kmers-matrix-distance-folder and
// kmers-matrix-distance-merge: one MatrixDistance<Caller>::compute() (matrix_distance.h:45-170)
// per problem, many problems per device pass (skm_matrix_batch_*).
//
// A problem is a list of input FASTA files and one output file.  Its usable files (regular,
// size > 0; matrix_distance.h:92-93) are parsed in order into one record list with one SeqIdMap
// across the files; records with an empty id are dropped (call_functions.tcc:171); an id's
// protein length is the length of the first record carrying it (prot_sizes.insert does not
// overwrite, matrix_distance.h:84; the reference at --n-threads 1).  A problem without a usable
// file creates no output file (:116-121); one with sequences and no pairs an empty one.
// Output line (:165-166): seq1 \t seq2 \t count \t score \n, ordered by (id1, id2) index (the
// reference prints the hash order of its maps).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

struct skm_db;

namespace skmf {

// score = float(count) / float(len1 + len2) (the sum in size_t), printed as ostream << float
// prints it: six significant digits, %g
inline std::string md_score_text(uint32_t count, size_t len1, size_t len2) {
    const float score = static_cast<float>(count) / static_cast<float>(len1 + len2);
    char b[64];
    std::snprintf(b, sizeof b, "%g", (double)score);
    return b;
}

struct MdProblem {
    std::vector<std::string> inputs;
    std::string output;
};

struct MdBatchConfig {
    int hypo_index = -1;
    bool verbose = false;
    // upper bound on query windows per device batch; a larger single problem is a batch of its own
    uint64_t batch_windows = 1ull << 26;
};

// Runs every problem, in order, in batches.  Each output is written under a temporary name and
// renamed when its batch succeeded.  Returns false (err set) at the first failing batch; the
// outputs of earlier batches stay.
bool run_matrix_problems(skm_db* db, const std::vector<MdProblem>& work, const MdBatchConfig& cfg, std::string& err);

// sub-directories of dir in readdir order
bool list_directories(const std::string& dir, std::vector<std::string>& out, std::string& err);
bool is_regular_file(const std::string& p);
bool is_directory(const std::string& p);
bool path_exists(const std::string& p);
// operator<< of a filesystem path: double-quoted, '"' and '\\' escaped with '\\'
std::string quoted_path(const std::string& p);

}  // namespace skmf
