// kmers-matrix-distance-folder -- drop-in for the reference's main (kmers-matrix-distance-folder.cc).
//
//   kmers-matrix-distance-folder [options] data-dir input-dir output-dir
// The all-vs-all shared-signature-k-mer matrix (MatrixDistance::compute, matrix_distance.h:45-170)
// of every regular file of input-dir, written to the file of the same name in output-dir.  Files
// whose output already exists are skipped (the reference's resume behaviour); every other
// "<input>" "<output>" pair is printed to stderr first.  The problems run on the GPU many at a
// time (skm_matrix_batch_*, front/skm_mdbatch.h); an output appears under its name only once its
// batch succeeded.  Lines: seq1 \t seq2 \t count \t score, ordered by (seq1, seq2) index (the
// reference prints the hash order of its maps).  -j / --j and --debug-hits are accepted and have
// no effect.  Extra options: --device N, --batch-windows W (query windows per device batch).
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "skm.h"
#include "skm_caller.h"
#include "skm_front.h"
#include "skm_mdbatch.h"

using namespace skmf;

namespace {
void die(const std::string& m) {
    std::cerr << m << "\n";
    std::exit(1);
}
}  // namespace

int main(int argc, char** argv) {
    Options op;
    op.specs = {{"data-dir", 'd', false, false},  {"input-dir", 0, false, false},  {"output-dir", 0, false, false},
                {"n-threads", 'j', false, false}, {"j", 0, false, false},          {"debug-hits", 0, true, false},
                {"verbose", 0, true, false},      {"help", 'h', true, false},      {"device", 0, false, false},
                {"batch-windows", 0, false, false}};
    op.positional = {"data-dir", "input-dir", "output-dir"};
    std::string err;
    if (!op.parse(argc, argv, err)) die(err);
    if (op.has("help")) {
        std::cout << "Usage: " << argv[0] << " data-dir input-dir output-dir\nAllowed options:\n"
                  << "  -d [ --data-dir ] arg   Data directory\n"
                  << "  --input-dir arg         Input directory\n"
                  << "  --output-dir arg        Output directory\n"
                  << "  -j [ --n-threads ] arg  Number of threads\n"
                  << "  --j arg                 Number of threads\n"
                  << "  --debug-hits            Debug kmer hits\n"
                  << "  --verbose               Enable verbose mode\n"
                  << "  --device arg            HIP device ordinal (default 0)\n"
                  << "  --batch-windows arg     query windows per device batch (default 67108864)\n"
                  << "  -h [ --help ]           show this help message\n\n";
        return 0;
    }
    // every check that needs no GPU comes before the first HIP call
    const std::string data_dir = op.get("data-dir"), input_dir = op.get("input-dir"), output_dir = op.get("output-dir");
    const std::string db_base = path_join(data_dir, "kmer_data");
    const std::string mph = db_base + ".mph", dat = db_base + ".dat";
    if (!path_exists(mph)) die("Database " + quoted_path(db_base) + " does not exist");
    std::vector<std::string> fidx;
    if (!read_function_index(path_join(data_dir, "function.index"), fidx, err)) die(err);
    MdBatchConfig cfg;
    for (size_t i = 0; i < fidx.size() && cfg.hypo_index < 0; ++i)
        if (fidx[i] == "hypothetical protein") cfg.hypo_index = (int)i;
    if (cfg.hypo_index < 0) die("Cannot find hypothetical protein index");  // call_functions.tcc:269-274
    cfg.verbose = op.has("verbose");
    if (op.has("batch-windows")) cfg.batch_windows = std::strtoull(op.get("batch-windows").c_str(), nullptr, 10);
    std::vector<std::string> files;
    if (!list_regular_files(input_dir, files, err)) die(err);
    std::vector<MdProblem> work;
    for (const std::string& f : files) {
        const std::string out = path_join(output_dir, path_filename(f));
        if (!path_exists(out)) work.push_back({{f}, out});
    }
    for (const MdProblem& w : work) std::cerr << quoted_path(w.inputs[0]) << " " << quoted_path(w.output) << "\n";
    if (work.empty()) return 0;

    skm_db* db = nullptr;
    if (skm_db_open(&db, mph.c_str(), dat.c_str(), std::atoi(op.get("device", "0").c_str()))) {
        std::cerr << skm_last_error() << "\n";
        return 1;
    }
    const bool ok = run_matrix_problems(db, work, cfg, err);
    skm_db_close(db);
    if (!ok) {
        std::cerr << err << "\n";
        return 1;
    }
    return 0;
}
