// skm_caller.h -- FunctionCaller<KmerDb>::process_fasta_stream for the CLIs
// (call_functions.tcc:109-257): every record with a non-empty id is one query; the windows are
// looked up and the HitSet calls made on the GPU (skm_annotate), find_best_call runs on the host
// or -- the CLIs' --best-call device -- on the resident calls (skm_annotate_best).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "skm.h"
#include "skm_front.h"

namespace skmf {

struct SeqCall {
    uint16_t fi = 0xFFFF;
    float score = 0.0f;
    std::string func;
};

// FunctionCaller::read_function_index (call_functions.tcc:123-148): column 0 = index, column 1 =
// name; the table is sized max index + 1.
bool read_function_index(const std::string& path, std::vector<std::string>& table, std::string& err);

// Boost.Math statistics the reference was compiled against (call_functions.tcc:51-53; SURVEY
// A.6): mean_mode 0 = the >= 1.76 four-lane mean, 1 = the single running mean; mad_mode 0 =
// |x(mid) - median|, 1 = the older median_absolute_deviation that returns |x(mid)|.  Process-wide
// setting for call_files (the CLIs' --boost-math-stats option); default 0 / 0.
void set_boost_math_modes(int mean_mode, int mad_mode);

// Query every sequence of every file (in order) against db.  out[f][r] is the call for record r
// of file f.  Files are batched so one device batch holds <= max_batch_residues residues.
// raw: the files' bytes (parse_fasta_files_bytes; files[f] is raw's file f) -- the sequence bodies
// are then parsed on the device (annotate_batch_fasta) and the files need no residues.
// device_ms: wall ms in skm_annotate (packing, upload, device pipeline, calls download);
// host_ms: wall ms of the rest (batch assembly, find_best_call on n_threads host threads).
// fx (best_call_tables, --best-call device): find_best_call runs on the device after the HitSet
// kernels (skm_annotate_best / skm_annotate_fasta_best) and the host only composes the names;
// *n_deferred = the sequences the device left to skm_find_best_call (0 without fx).
int call_files(skm_db* db, const std::vector<const FastaFile*>& files, const std::vector<std::string>& function_index,
               bool ignore_hypo, int n_threads, std::vector<std::vector<SeqCall>>& out, std::string& err,
               double* device_ms = nullptr, uint64_t max_batch_residues = 2000000000ull, double* host_ms = nullptr,
               const FastaBytes* raw = nullptr, const skm_fidx* fx = nullptr, uint64_t* n_deferred = nullptr);

// --best-call host|device: device makes the function-index tables on `device` (release them with
// skm_fidx_destroy), host leaves *fx null; false with err for any other word or a failed upload
bool best_call_tables(const std::string& mode, const std::vector<std::string>& function_index, int device,
                      skm_fidx** fx, std::string& err);

// The two halves of call_files, for callers that pipeline them (kmers-call-functions overlaps
// parsing, the device and find_best_call over groups of files, as the reference overlaps its
// per-file tasks with its writer thread, kmers-call-functions.cc:147-189).
// annot_opts_for: process_aa_seq's options (min_hits 5, max_gap 200, the hypothetical-protein
// index -- an error when the function index has none, call_functions.tcc:269-274).
bool annot_opts_for(const std::vector<std::string>& function_index, bool ignore_hypo, skm_annot_opts& o,
                    std::string& err);
// the device half for one batch of whole files: the windows looked up and the HitSet calls made
// (skm_annotate over their sequences, in file order); *calls is released with skm_calls_free
int annotate_batch(skm_db* db, const std::vector<const FastaFile*>& files, const skm_annot_opts& o, int n_threads,
                   skm_calls* calls, std::string& err);
// annotate_batch from the files' bytes (file f at bytes[file_off[f], file_off[f + 1]), as
// parse_fasta_files_bytes lays them out): FastaParser's sequence bodies parsed on the device
// (skm_annotate_fasta), no packing copy.  files are the headers-only host parses; the device's
// record counts and lengths must equal theirs (else SKM_E_STATE, err names the file).
int annotate_batch_fasta(skm_db* db, const std::vector<const FastaFile*>& files, const uint8_t* bytes,
                         const uint64_t* file_off, const skm_annot_opts& o, skm_calls* calls, std::string& err);
// the two device halves with find_best_call on the resident calls: *best is released with
// skm_best_calls_free
int annotate_batch_best(skm_db* db, const std::vector<const FastaFile*>& files, const skm_annot_opts& o, int n_threads,
                        const skm_fidx* fx, skm_best_calls* best, std::string& err);
int annotate_batch_fasta_best(skm_db* db, const std::vector<const FastaFile*>& files, const uint8_t* bytes,
                              const uint64_t* file_off, const skm_annot_opts& o, const skm_fidx* fx, skm_best_calls* best,
                              std::string& err);
// their host half: name composition only (skm_best_call_name) on n_threads threads
int compose_best_batch(const skm_best_calls& best, const std::vector<const FastaFile*>& files, const skm_fidx* fx,
                       int n_threads, const std::vector<std::vector<SeqCall>*>& out, std::string& err);
// the host half: find_best_call per sequence on n_threads threads; out[f] is the call vector of
// files[f] (sized by the caller)
int best_calls_batch(const skm_calls& calls, const std::vector<const FastaFile*>& files,
                     const std::vector<const char*>& fidx, int n_threads, const std::vector<std::vector<SeqCall>*>& out,
                     std::string& err);


// kmers-build-signatures --recall-source device: the recall pass with the records that were
// selected into the build read in place from the build's resident sequences (skm_build_recall: no
// second pack and upload of them), and only the records select_build_sequences left out -- no
// function, an unkept function, a deleted fid -- uploaded as call_files uploads them.  batches[f] is
// files[f]'s selection as it was added to b (every file, in order).  find_best_call runs on the
// device for both sets (fx must hold device tables); out[f][r] as call_files fills it.
struct ResidentRecall {
    uint64_t resident_seqs = 0, uploaded_seqs = 0, batches = 0, deferred = 0;
    double device_ms = 0;  // wall ms in skm_build_recall and skm_annotate_best
};
int call_files_resident(skm_build* b, skm_db* db, const std::vector<const FastaFile*>& files,
                        const std::vector<BuildBatch>& batches, const std::vector<std::string>& function_index,
                        int n_threads, const skm_fidx* fx, std::vector<std::vector<SeqCall>>& out, std::string& err,
                        ResidentRecall* stats, uint64_t max_batch_residues = 2000000000ull);

}  // namespace skmf
