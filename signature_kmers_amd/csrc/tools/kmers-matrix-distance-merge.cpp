// kmers-matrix-distance-merge -- drop-in for the reference's main (kmers-matrix-distance-merge.cc).
//
//   kmers-matrix-distance-merge [options] data-dir base-dir output-dir [family-ids...]
// base-dir is the genus.data directory of a family build: its genus directories are the
// sub-directories holding a regular file local.family.defs.  For every family id (the given ones,
// or "0" .. "nfunc-1" from function.index) the all-vs-all shared-signature-k-mer matrix
// (MatrixDistance::compute, matrix_distance.h:45-170) over <genus>/fasta_by_function/<id> of every
// genus directory -- one SeqIdMap across the files, in genus order -- is written to
// output-dir/<id>; a family without a usable input file gets no output file.  The problems run on
// the GPU many at a time (skm_matrix_batch_*, front/skm_mdbatch.h).  Lines: seq1 \t seq2 \t count
// \t score, ordered by (seq1, seq2) index (the reference prints the hash order of its maps).
// -j and --debug-hits are accepted and have no effect.  Extra options: --device N,
// --batch-windows W (query windows per device batch).
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
    op.specs = {{"data-dir", 'd', false, false},  {"base-dir", 0, false, false},   {"output-dir", 0, false, false},
                {"family-ids", 0, false, true},   {"n-threads", 'j', false, false}, {"debug-hits", 0, true, false},
                {"verbose", 0, true, false},      {"help", 'h', true, false},      {"device", 0, false, false},
                {"batch-windows", 0, false, false}};
    op.positional = {"data-dir", "base-dir", "output-dir", "family-ids"};
    std::string err;
    if (!op.parse(argc, argv, err)) die(err);
    if (op.has("help")) {
        std::cout << "Usage: " << argv[0] << " data-dir input-dir output-dir\nAllowed options:\n"
                  << "  -d [ --data-dir ] arg   Data directory\n"
                  << "  --base-dir arg          Bae directory\n"
                  << "  --output-dir arg        Output directory\n"
                  << "  --family-ids arg        Family ids\n"
                  << "  -j [ --n-threads ] arg  Number of threads\n"
                  << "  --debug-hits            Debug kmer hits\n"
                  << "  --verbose               Enable verbose mode\n"
                  << "  --device arg            HIP device ordinal (default 0)\n"
                  << "  --batch-windows arg     query windows per device batch (default 67108864)\n"
                  << "  -h [ --help ]           show this help message\n\n";
        return 0;
    }
    // every check that needs no GPU comes before the first HIP call; the reference checks the base
    // directory before it opens the DB
    const std::string data_dir = op.get("data-dir"), base_dir = op.get("base-dir"), output_dir = op.get("output-dir");
    if (!is_directory(base_dir)) die("Base directory " + quoted_path(base_dir) + " is not a valid directory");
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
    std::vector<std::string> fams = op.all("family-ids");
    if (fams.empty())
        for (size_t i = 0; i < fidx.size(); ++i) fams.push_back(std::to_string(i));
    std::vector<std::string> subdirs, genus_dirs;
    if (!list_directories(base_dir, subdirs, err)) die(err);
    for (const std::string& g : subdirs)
        if (is_regular_file(path_join(g, "local.family.defs"))) genus_dirs.push_back(g);
    if (genus_dirs.empty()) die("No valid genus directories found in " + quoted_path(base_dir));
    std::vector<MdProblem> work;
    for (const std::string& fam : fams) {
        MdProblem p;
        for (const std::string& g : genus_dirs) p.inputs.push_back(path_join(path_join(g, "fasta_by_function"), fam));
        p.output = path_join(output_dir, fam);
        work.push_back(std::move(p));
    }

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
