// kmers-build-signatures -- drop-in for the reference's main (kmers-build-signatures.cc:126-373).
//
// Same options, same files in --kmer-data-dir (function.index, otu.index, genomes, final.kmers,
// distinct_functions, recall.report.d/<fasta>, kmer_data.mph/.dat with --perfect-hash) and the
// same stdout lines.  The k-mer extraction, group-by, 80 % cut and statistics run on one MI355X
// through libskm (skm_build_*); the recall pass runs the GPU annotate path against an exact-key
// DB of the kept k-mers (KeptKmerDB semantics, skm_db_open_kept); the perfect hash is built on a
// host thread while the recall runs (as the reference does, kmers-build-signatures.cc:268-276).
//
// Result order: final.kmers is written in ascending k-mer key order and distinct_functions in
// ascending function index; the reference writes both in TBB hash-table order, so compare them
// as sets.  --nudb-file is not supported (NuDB is out of scope).
// Extra options: --device N (HIP device), --dump-extract FILE (write the build input arrays and
// stop before touching the GPU; used by the CPU tests), --mph-seed N, --recall-db host|device (the
// recall DB from the downloaded kept k-mers, or built on the GPU from the resident ones),
// --perfect-hash-source host|device (likewise for kmer_data.mph / .dat: skm_build_mph_db; the files
// are the same), --final-kmers-source host|device (final.kmers formatted by the host threads from
// the downloaded kept k-mers, or sorted, formatted and streamed out by the GPU from the resident
// ones: skm_build_write_final_kmers; the file is the same).  With all three on `device` (or no
// --perfect-hash) the kept set never comes to the host: skm_build_finish is not called, the three
// stdout lines and distinct_functions come from skm_build_stats.
// --recall-source host|device: the recall pass packs and uploads every training protein again, or
// (device) reads the proteins that were selected into the build in place from the build's resident
// sequences (skm_build_recall) and uploads only the records the selection left out; every output is
// the same.  The build handle then lives until the recall is done, and keeps its sequences where
// it releases its work buffers.
// --fasta-parse host|device: the sequence bodies of the training files are parsed into host strings
// and packed into the build by host threads, or (device) the host parses headers only and every
// group of whole files (--fasta-group-mb, default 256) goes to the GPU as raw bytes, where the
// records the selection names are parsed straight into the build's resident buffer
// (skm_build_add_fasta).  The records the selection left out are parsed on the host from their byte
// ranges alone, for the recall (the parse error reports of those ranges, which can hold records with
// an empty id too, appear a second time on stderr).  Needs one GPU and --recall-source device; every output is the same.
// Multi-GPU: --n-gpus N forks one process per GPU (rank r on device r) before
// any GPU or thread use; or, under an external launcher (RANK / WORLD_SIZE / LOCAL_RANK in the
// environment, e.g. torchrun --no-python), each launched process is one rank and rank 0 hands the
// RCCL unique id to the others through --comm-file (default <kmer-data-dir>/.skm_comm_id).
// Every rank parses every file's headers (the FunctionMap needs them all) but keeps residues only
// for the files it builds (rank 0, which runs the recall pass, keeps all); rank r builds the
// contiguous range of files r*F/N .. (r+1)*F/N, the ranks exchange occurrences by owner GPU (RCCL all-to-all) and
// rank 0 gathers the kept k-mers and writes every output, exactly as one process would.
// --comm host joins the forked ranks through socketpairs instead of RCCL (several ranks may then
// share one GPU: --device is every rank's device; used by the tests).
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <iostream>
#include <map>
#include <sstream>
#include <thread>
#include <vector>
#include <atomic>
#include <condition_variable>
#include <mutex>

#include "skm.h"
#include "skm_caller.h"
#include "skm_front.h"
#include "skm_mesh.h"

using namespace skmf;

namespace {

const int K = 8;
const unsigned MaxSequencesPerFile = 100000;

double now_s() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

void die(const std::string& m) {
    std::cerr << m << "\n";
    std::exit(1);
}

std::string quoted(const std::string& p) { return "\"" + p + "\""; }

// final.kmers (kmers-build-signatures.cc:212-216): "KMER\tavg_from_end\tfunction_index\t\n" per
// kept k-mer.  Blocks of lines are sized first (the decimal widths), then formatted and written
// at their offsets (pwrite) by `threads` threads, so formatting and writing overlap.
void write_final_kmers(const std::string& path, const skm_kept& kept, int threads) {
    const uint64_t B = 1u << 20;  // lines per block
    const uint64_t nb = (kept.n + B - 1) / B;
    const int T = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(1, threads), nb));
    auto ndig = [](unsigned v) { return v < 10 ? 1 : v < 100 ? 2 : v < 1000 ? 3 : v < 10000 ? 4 : 5; };
    auto fmt_u = [](char* p, unsigned v) {  // decimal, returns the digits written
        char t[8];
        int n = 0;
        do {
            t[n++] = (char)('0' + v % 10);
            v /= 10;
        } while (v);
        for (int i = 0; i < n; ++i) p[i] = t[n - 1 - i];
        return n;
    };
    std::vector<uint64_t> off(nb + 1, 0);
    auto par = [&](const std::function<void(uint64_t)>& f) {
        std::atomic<uint64_t> next{0};
        auto work = [&] {
            for (uint64_t b; (b = next.fetch_add(1)) < nb;) f(b);
        };
        std::vector<std::thread> th;
        for (int t = 1; t < T; ++t) th.emplace_back(work);
        work();
        for (auto& x : th) x.join();
    };
    par([&](uint64_t b) {
        uint64_t n = 0;
        for (uint64_t i = b * B, e = std::min<uint64_t>(kept.n, i + B); i < e; ++i)
            n += 12 + ndig(kept.data[i].avg_from_end) + ndig(kept.data[i].function_index);
        off[b + 1] = n;
    });
    for (uint64_t b = 0; b < nb; ++b) off[b + 1] += off[b];
    const int fd = ::open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) die("cannot write " + path);
    std::atomic<bool> ok{true};
    par([&](uint64_t b) {
        std::string o(off[b + 1] - off[b], '\0');
        char* p = &o[0];
        for (uint64_t i = b * B, e = std::min<uint64_t>(kept.n, i + B); i < e; ++i) {
            std::memcpy(p, &kept.keys[i], 8);
            p[8] = '\t';
            p += 9;
            p += fmt_u(p, kept.data[i].avg_from_end);
            *p++ = '\t';
            p += fmt_u(p, kept.data[i].function_index);
            *p++ = '\t';
            *p++ = '\n';
        }
        for (uint64_t w = 0; w < o.size();) {
            const ssize_t r = ::pwrite(fd, o.data() + w, o.size() - w, (off_t)(off[b] + w));
            if (r <= 0) {
                ok = false;
                return;
            }
            w += (uint64_t)r;
        }
    });
    if (::close(fd) != 0 || !ok) die("cannot write " + path);
}

// binary dump of the build input (--dump-extract): u64 n_seqs, u64 n_residues, then
// residues[n_residues], off u64[n], len u32[n], func u16[n], seq_id u32[n]
void dump_extract(const std::string& path, const std::vector<FastaFile>& files, const std::vector<BuildBatch>& batches) {
    std::vector<uint8_t> res;
    std::vector<uint64_t> off;
    std::vector<uint32_t> len, sid;
    std::vector<uint16_t> fn;
    for (size_t f = 0; f < files.size(); ++f) {
        const BuildBatch& b = batches[f];
        for (size_t s = 0; s < b.off.size(); ++s) {
            off.push_back(res.size());
            res.insert(res.end(), files[f].residues.begin() + b.off[s], files[f].residues.begin() + b.off[s] + b.len[s]);
            len.push_back(b.len[s]);
            fn.push_back(b.func[s]);
            sid.push_back(b.seq_id[s]);
        }
    }
    std::ofstream o(path, std::ios::binary);
    uint64_t n = off.size(), nr = res.size();
    o.write((const char*)&n, 8);
    o.write((const char*)&nr, 8);
    o.write((const char*)res.data(), (std::streamsize)nr);
    o.write((const char*)off.data(), (std::streamsize)(8 * n));
    o.write((const char*)len.data(), (std::streamsize)(4 * n));
    o.write((const char*)fn.data(), (std::streamsize)(2 * n));
    o.write((const char*)sid.data(), (std::streamsize)(4 * n));
    if (!o) die("cannot write " + path);
}

bool read_whole_file(const std::string& path, std::vector<uint8_t>& buf) {
    FILE* fp = std::fopen(path.c_str(), "rb");
    if (!fp) return false;
    for (;;) {
        const size_t at = buf.size();
        buf.resize(at + (4u << 20));
        const size_t got = std::fread(buf.data() + at, 1, 4u << 20, fp);
        buf.resize(at + got);
        if (got < (4u << 20)) break;
    }
    const bool ok = !std::ferror(fp);
    std::fclose(fp);
    return ok;
}

// --fasta-parse device: files [f0, f1) into the build in groups of whole files of up to group_bytes,
// each group one skm_build_add_fasta call over the files' bytes.  files are the headers-only host
// parses and batches their selections (wait_selected(f) returns once batches[f] is made).  The
// device's table is checked against the host parse file by file.  The records a selection left out
// are parsed on the host from their byte ranges (a run's first '>' to the next selected record's, or
// the file's end): files[f].residues then holds these records' residues alone and off[r] points into it for
// them -- what call_files_resident reads; host_bytes counts them.
void add_files_on_device(skm_build* b, std::vector<FastaFile>& files, const std::vector<BuildBatch>& batches, size_t f0,
                         size_t f1, uint64_t group_bytes, int device, const std::function<void(size_t)>& wait_selected,
                         uint64_t& host_bytes) {
    // test hook (tests/test_gpu_cli_build_fasta.py): the device is given one record more in this file
    const char* extra = std::getenv("SKM_CLI_FASTA_EXTRA_RECORD");
    std::vector<uint64_t> fsize(f1, 0);
    for (size_t f = f0; f < f1; ++f) {
        struct stat sb;
        if (::stat(files[f].path.c_str(), &sb) == 0) fsize[f] = (uint64_t)sb.st_size;
    }
    std::vector<uint8_t> buf;
    std::vector<uint64_t> foff;
    std::vector<uint16_t> rfunc;
    std::vector<uint32_t> rid;
    for (size_t g0 = f0; g0 < f1;) {
        size_t g1 = g0;
        uint64_t bytes = 0;
        while (g1 < f1 && (g1 == g0 || bytes + fsize[g1] <= group_bytes)) bytes += fsize[g1++];
        buf.clear();
        foff.assign(1, 0);
        rfunc.clear();
        rid.clear();
        for (size_t f = g0; f < g1; ++f) {
            wait_selected(f);
            if (!read_whole_file(files[f].path, buf)) die("cannot read " + files[f].path);
            if (extra && (size_t)std::atol(extra) == f) {
                const char* inj = "\n>injected\n";
                buf.insert(buf.end(), inj, inj + std::strlen(inj));
            }
            foff.push_back(buf.size());
            const size_t base = rfunc.size();
            rfunc.resize(base + files[f].size(), (uint16_t)SKM_UNDEFINED_FUNCTION);
            rid.resize(base + files[f].size(), 0);
            const BuildBatch& bb = batches[f];
            for (size_t s = 0; s < bb.rec.size(); ++s) {
                rfunc[base + bb.rec[s]] = bb.func[s];
                rid[base + bb.rec[s]] = bb.seq_id[s];
            }
        }
        const size_t nf = g1 - g0;
        skm_fasta_table tab{};
        int rc = skm_build_add_fasta(b, buf.data(), foff.data(), nf, rfunc.data(), rid.data(), rfunc.size(), &tab);
        const std::string add_err = rc ? skm_last_error() : "";
        // a refused group is parsed without the build, for the table that names the file
        if (rc == SKM_E_ARG && skm_fasta_parse_device(buf.data(), foff.data(), nf, device, 0, &tab) != SKM_OK) tab = {};
        if (rc && !tab.file_rec) die("skm_build_add_fasta: " + add_err);
        for (size_t i = 0; i < nf; ++i) {
            const FastaFile& F = files[g0 + i];
            const uint64_t r0 = tab.file_rec[i], n = tab.file_rec[i + 1] - r0;
            if (n != F.size())
                die("device FASTA parse of " + F.path + ": " + std::to_string(n) + " records, the host parse has " +
                    std::to_string(F.size()));
            for (size_t r = 0; r < F.size(); ++r)
                if (tab.seq_len[r0 + r] != F.len[r])
                    die("device FASTA parse of " + F.path + ": record " + F.ids[r] + " has " +
                        std::to_string(tab.seq_len[r0 + r]) + " residues, the host parse has " + std::to_string(F.len[r]));
        }
        if (rc) die("skm_build_add_fasta: " + add_err);
        for (size_t i = 0; i < nf; ++i) {
            FastaFile& F = files[g0 + i];
            const uint64_t r0 = tab.file_rec[i];
            const std::vector<uint32_t>& rec = batches[g0 + i].rec;
            // every run of consecutive left-out records in one parse, appended to `lo`
            FastaFile lo;
            std::vector<size_t> lo_rec;
            size_t k = 0;
            for (size_t r = 0; r < F.size();) {
                if (k < rec.size() && rec[k] == r) {
                    ++k;
                    F.off[r++] = 0;
                    continue;
                }
                size_t e = r;
                while (e < F.size() && !(k < rec.size() && rec[k] == e)) lo_rec.push_back(e++);
                const uint64_t a = tab.hdr_pos[r0 + r], z = e < F.size() ? tab.hdr_pos[r0 + e] : foff[i + 1];
                parse_fasta_buffer((const char*)buf.data() + a, (size_t)(z - a), lo, true);
                r = e;
            }
            if (lo.size() != lo_rec.size())
                die("host parse of the left-out records of " + F.path + " from their byte ranges: " +
                    std::to_string(lo.size()) + " records, the selection leaves out " + std::to_string(lo_rec.size()));
            for (size_t j = 0; j < lo_rec.size(); ++j) {
                const size_t r = lo_rec[j];
                if (lo.len[j] != F.len[r] || lo.ids[j] != F.ids[r])
                    die("host parse of record " + F.ids[r] + " of " + F.path + " from its byte range differs from the file's parse");
                F.off[r] = lo.off[j];
                host_bytes += F.len[r];
            }
            F.residues = std::move(lo.residues);
        }
        skm_fasta_table_free(&tab);
        g0 = g1;
    }
}

}  // namespace

int main(int argc, char** argv) {
    {  // libskm runs up to 10 streams at once: 16 hardware queues (read at the first HIP call)
        const char* q = getenv("GPU_MAX_HW_QUEUES");
        if (!q || atoi(q) < 16) setenv("GPU_MAX_HW_QUEUES", "16", 1);
    }
    Options op;
    op.specs = {{"definition-dir", 'D', false, true},  {"fasta-dir", 'F', false, true},
                {"fasta-keep-functions-dir", 'K', false, true}, {"good-functions", 0, false, true},
                {"good-roles", 0, false, true},        {"deleted-features-file", 0, false, false},
                {"ignored-functions-file", 0, false, false}, {"kmer-data-dir", 0, false, false},
                {"nudb-file", 0, false, false},        {"min-reps-required", 0, false, false},
                {"final-kmers", 0, false, false},      {"n-threads", 0, false, false},
                {"perfect-hash", 0, false, false},     {"perfect-hash-data", 0, false, false},
                {"help", 'h', true, false},            {"device", 0, false, false},
                {"dump-extract", 0, false, false},     {"mph-seed", 0, false, false},
                {"n-gpus", 0, false, false},           {"comm", 0, false, false},
                {"comm-file", 0, false, false},        {"recall-db", 0, false, false},
                {"perfect-hash-source", 0, false, false}, {"best-call", 0, false, false},
                {"final-kmers-source", 0, false, false}, {"recall-source", 0, false, false},
                {"fasta-parse", 0, false, false},      {"fasta-group-mb", 0, false, false}};
    std::string err;
    if (!op.parse(argc, argv, err)) die(err);
    if (op.has("help")) {
        std::cout << "Usage: " << argv[0] << " [options]\nAllowed options:\n"
                  << "  -D [ --definition-dir ] arg          Directory of function definition files\n"
                  << "  -F [ --fasta-dir ] arg               Directory of fasta files of protein data\n"
                  << "  -K [ --fasta-keep-functions-dir ] arg Directory of fasta files of protein data (keep functions defined here)\n"
                  << "  --good-functions arg                 File containing list of functions to be kept\n"
                  << "  --good-roles arg                     File containing list of roles to be kept\n"
                  << "  --deleted-features-file arg          File containing list of deleted feature IDs\n"
                  << "  --ignored-functions-file arg         File containing list of functions for which we do not create signatures\n"
                  << "  --kmer-data-dir arg                  Write kmer data files to this directory\n"
                  << "  --min-reps-required arg              Minimum number of genomes a function must be seen in\n"
                  << "  --final-kmers arg                    Write final.kmers file\n"
                  << "  --n-threads arg                      Number of host threads (results do not depend on it)\n"
                  << "  --perfect-hash arg                   Compute perfect hash of signature kmers and store in this file\n"
                  << "  --perfect-hash-data arg              Kmer data stored by perfect hash\n"
                  << "  --device arg                         HIP device ordinal (default 0)\n"
                  << "  --n-gpus arg                         ranks (one process and GPU each, power of two)\n"
                  << "  --comm arg                           rccl (default) or host (socketpairs; ranks may share a GPU)\n"
                  << "  --comm-file arg                      RCCL id rendezvous file under an external launcher\n"
                  << "  --recall-db arg                      host (default): the recall DB from the downloaded kept k-mers;\n"
                  << "                                       device: built on the GPU from the build's resident kept k-mers (one GPU)\n"
                  << "  --perfect-hash-source arg            host (default): the perfect hash from the downloaded kept k-mers;\n"
                  << "                                       device: hash and data files written from the DB built on the GPU\n"
                  << "                                       from the build's resident kept k-mers (needs --perfect-hash, one GPU)\n"
                  << "  --final-kmers-source arg             host (default): final.kmers formatted on the host from the downloaded\n"
                  << "                                       kept k-mers; device: sorted, formatted and streamed out by the GPU from\n"
                  << "                                       the build's resident kept k-mers (needs --final-kmers, one GPU); with\n"
                  << "                                       --recall-db device and --perfect-hash-source device (or no\n"
                  << "                                       --perfect-hash) the kept k-mers are never copied to the host\n"
                  << "  --best-call arg                      host (default) | device: where the recall pass runs find_best_call\n"
                  << "  --recall-source arg                  host (default): the recall pass packs and uploads every protein again;\n"
                  << "                                       device: the proteins selected into the build are recalled in place from\n"
                  << "                                       the build's resident sequences, only the others are uploaded, and\n"
                  << "                                       find_best_call runs on the device (one GPU; the outputs are the same)\n"
                  << "  --fasta-parse arg                    host (default): the sequence bodies are parsed and packed on the host;\n"
                  << "                                       device: the host parses headers only and the GPU parses the selected\n"
                  << "                                       records from the files' bytes into the build (one GPU, needs\n"
                  << "                                       --recall-source device; the outputs are the same)\n"
                  << "  --fasta-group-mb arg                 --fasta-parse device: whole files per device parse, up to this many MB\n"
                  << "                                       (default 256; a larger file is a group of its own)\n"
                  << "  -h [ --help ]                        show this help message\n";
        return 1;
    }
    const double t_start = now_s();
    const double t_startup = process_age_s();  // before main: loader, libskm, HIP runtime
    // ranks: forked here (before any thread or GPU use), or given by an external launcher
    Mesh mesh;
    const std::string comm = op.get("comm", "rccl");
    if (comm != "rccl" && comm != "host") die("--comm must be rccl or host");
    const std::string recall_db = op.get("recall-db", "host");
    if (recall_db != "host" && recall_db != "device") die("--recall-db must be host or device");
    const char* env_ws = std::getenv("WORLD_SIZE");
    const bool launched = env_ws && std::atoi(env_ws) > 1 && !op.has("n-gpus");
    if (recall_db == "device" && (launched || std::atoi(op.get("n-gpus", "1").c_str()) > 1))
        die("--recall-db device needs one GPU: the kept k-mers of a multi-rank build are sharded over the ranks");
    const std::string best_call = op.get("best-call", "host");
    if (best_call != "host" && best_call != "device") die("--best-call must be host or device");
    const std::string ph_source = op.get("perfect-hash-source", "host");
    if (ph_source != "host" && ph_source != "device") die("--perfect-hash-source must be host or device");
    if (ph_source == "device" && op.get("perfect-hash").empty())
        die("--perfect-hash-source device needs --perfect-hash: it names the file the hash is written to");
    if (ph_source == "device" && (launched || std::atoi(op.get("n-gpus", "1").c_str()) > 1))
        die("--perfect-hash-source device needs one GPU: the kept k-mers of a multi-rank build are sharded over the ranks");
    const std::string fk_source = op.get("final-kmers-source", "host");
    if (fk_source != "host" && fk_source != "device") die("--final-kmers-source must be host or device");
    if (fk_source == "device" && op.get("final-kmers").empty())
        die("--final-kmers-source device needs --final-kmers: it names the file the k-mers are written to");
    if (fk_source == "device" && (launched || std::atoi(op.get("n-gpus", "1").c_str()) > 1))
        die("--final-kmers-source device needs one GPU: the kept k-mers of a multi-rank build are sharded over the ranks");
    const std::string recall_source = op.get("recall-source", "host");
    if (recall_source != "host" && recall_source != "device") die("--recall-source must be host or device");
    if (recall_source == "device" && (launched || std::atoi(op.get("n-gpus", "1").c_str()) > 1))
        die("--recall-source device needs one GPU: a rank of a multi-rank build holds only its own shard's sequences");
    const bool recall_resident = recall_source == "device";
    const std::string fasta_parse = op.get("fasta-parse", "host");
    if (fasta_parse != "host" && fasta_parse != "device") die("--fasta-parse must be host or device");
    if (fasta_parse == "device" && (launched || std::atoi(op.get("n-gpus", "1").c_str()) > 1 || !recall_resident))
        die("--fasta-parse device needs one GPU and --recall-source device: the host keeps no training residues to "
            "upload again for the recall");
    const bool fasta_dev = fasta_parse == "device" && !op.has("dump-extract");  // the dump stays on the host parse
    const double fasta_group_mb = std::atof(op.get("fasta-group-mb", "256").c_str());  // fractions are taken too
    if (!(fasta_group_mb > 0)) die("--fasta-group-mb must be positive");
    const uint64_t fasta_group_bytes = (uint64_t)std::max(1.0, fasta_group_mb * 1048576.0);
    const int release_level = recall_resident ? 2 : 1;  // 2 keeps the resident sequences for the recall
    // every consumer of the kept set on the device: no host copy of it is made
    const bool kept_on_device = fk_source == "device" && recall_db == "device" &&
                                (ph_source == "device" || op.get("perfect-hash").empty());
    int local_rank = 0;
    if (launched) {
        if (comm == "host") die("--comm host needs --n-gpus (forked ranks)");
        mesh.world = std::atoi(env_ws);
        mesh.rank = std::atoi(std::getenv("RANK") ? std::getenv("RANK") : "0");
        local_rank = std::atoi(std::getenv("LOCAL_RANK") ? std::getenv("LOCAL_RANK") : "0");
    } else {
        const int ng = std::atoi(op.get("n-gpus", "1").c_str());
        if (ng < 1 || ng > 64 || (ng & (ng - 1))) die("--n-gpus must be a power of two in [1, 64]");
        if (!mesh_fork(ng, mesh, err)) die(err);
        mesh.watch_children();
        local_rank = mesh.rank;
    }
    const int rank = mesh.rank, world = mesh.world;
    if (rank != 0 && !std::freopen("/dev/null", "w", stdout)) die("cannot silence rank stdout");
    // host threads for parsing / find_best_call only: results never depend on it
    int n_threads = std::atoi(op.get("n-threads", "0").c_str());
    if (n_threads < 2) n_threads = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    if (world > 1) n_threads = std::max(1, n_threads / std::min(world, 8));
    const int device = std::atoi(op.get("device", "0").c_str()) + (world > 1 && comm == "rccl" ? local_rank : 0);
    const int min_reps_required = std::atoi(op.get("min-reps-required", "3").c_str());
    const std::string kmer_data_dir = op.get("kmer-data-dir");
    std::string final_kmers = op.get("final-kmers");
    std::string ph_file = op.get("perfect-hash"), ph_data = op.get("perfect-hash-data");
    if (!ph_file.empty()) {
        if (path_is_relative(ph_file)) ph_file = path_join(kmer_data_dir, ph_file);
        if (path_is_relative(ph_data)) ph_data = path_join(kmer_data_dir, ph_data);
    }
    const uint32_t mph_seed = (uint32_t)std::strtoul(op.get("mph-seed", "1").c_str(), nullptr, 10);

    // the HIP runtime initialises on a thread of its own while the host parses (the first HIP call
    // of a process costs ~0.3-0.5 s)
    double t_hip_init = 0;
    std::thread hip_warm([&] {
        const double th = now_s();
        int ndev = 0;
        (void)skm_device_count(&ndev);
        t_hip_init = now_s() - th;
    });
    std::vector<std::string> definition_files, fasta_files, keep_files;
    auto populate = [&](const std::vector<std::string>& dirs, std::vector<std::string>& out) {
        for (const auto& d : dirs)
            if (!list_regular_files(d, out, err)) die(err);
    };
    populate(op.all("definition-dir"), definition_files);
    populate(op.all("fasta-dir"), fasta_files);
    populate(op.all("fasta-keep-functions-dir"), keep_files);
    std::cout << "definitions: ";
    for (auto& x : op.all("definition-dir")) std::cout << x << " ";
    std::cout << std::endl << "fasta: ";
    for (auto& x : op.all("fasta-dir")) std::cout << x << " ";
    std::cout << std::endl << "keep: ";
    for (auto& x : op.all("fasta-keep-functions-dir")) std::cout << x << " ";
    std::cout << std::endl;

    std::vector<std::string> good_functions, good_roles;
    for (auto& f : op.all("good-functions")) {
        bool ok;
        auto v = load_lines(f, &ok);
        if (!ok) std::cerr << "could not open " << f << "\n";
        good_functions.insert(good_functions.end(), v.begin(), v.end());
    }
    for (auto& f : op.all("good-roles")) {
        bool ok;
        auto v = load_lines(f, &ok);
        if (!ok) std::cerr << "could not open " << f << "\n";
        good_roles.insert(good_roles.end(), v.begin(), v.end());
    }

    // the FASTA files parse on the host threads while this thread loads the definitions (the two are
    // independent until the FunctionMap reads the records, below)
    std::cerr << "load fasta\n";
    std::vector<std::string> all_paths = fasta_files;  // fasta-dir files, then keep-dir files (signature_build.tcc:26-35)
    all_paths.insert(all_paths.end(), keep_files.begin(), keep_files.end());
    std::vector<FastaFile> files;
    // this rank's contiguous range of files (global file numbering keeps seq_id = file*100000+k)
    const size_t f0 = all_paths.size() * (size_t)rank / (size_t)world,
                 f1 = all_paths.size() * (size_t)(rank + 1) / (size_t)world;
    const bool dump = op.has("dump-extract");
    // The FunctionMap needs every file's headers; residues are kept only for the files this rank
    // builds -- and on rank 0, whose recall pass reads every sequence, for all of them.
    std::vector<char> keep_res(all_paths.size(), 0);
    for (size_t f = 0; f < all_paths.size(); ++f) keep_res[f] = !fasta_dev && (rank == 0 || dump || (f >= f0 && f < f1));
    double t0 = now_s();
    bool parsed_ok = true;
    std::string parse_err;
    double t_files = 0;  // the parser thread's own time
    std::thread parser([&] {
        parsed_ok = parse_fasta_files(all_paths, files, n_threads, parse_err, &keep_res);
        t_files = now_s() - t0;
    });
    const double td = now_s();
    FunctionMap fm;
    fm.add_good_roles(good_roles);
    fm.add_good_functions(good_functions);
    fm.load_id_assignments(definition_files, n_threads);
    const double t_defs = now_s() - td;

    std::set<std::string> deleted_fids, ignored_functions;
    if (op.has("deleted-features-file"))
        for (auto& l : load_lines(op.get("deleted-features-file"))) deleted_fids.insert(l);
    if (op.has("ignored-functions-file"))
        for (auto& l : load_lines(op.get("ignored-functions-file"))) ignored_functions.insert(l);

    if (!kmer_data_dir.empty() && !ensure_directory(kmer_data_dir)) die("Error creating " + quoted(kmer_data_dir));

    parser.join();
    if (!parsed_ok) die(parse_err);
    const double t_fm0 = now_s();
    try {
        fm.load_fasta_files(files, deleted_fids, n_threads);
    } catch (const std::exception& e) {
        die(std::string("terminate called after throwing an instance of 'std::out_of_range': ") + e.what());
    }
    const double t_parse = now_s() - t0, t_fm = now_s() - t_fm0;

    unsigned nkept_f = fm.process_kept_functions(min_reps_required, ignored_functions);
    std::cout << "kept " << nkept_f << " functions\n";
    if (!kmer_data_dir.empty()) {
        if (!fm.write_function_index(kmer_data_dir)) die("cannot write function.index");
        std::ofstream(path_join(kmer_data_dir, "otu.index")).close();
        std::ofstream g(path_join(kmer_data_dir, "genomes"));
        g << "empty genomes\n";
    }

    std::cerr << "extract kmers\n";
    std::vector<BuildBatch> batches(files.size());
    // Sequence selection runs on a worker pool, file by file, while this thread streams every
    // finished file (in order) into the build: skm_build_add_batch packs it into a pinned staging
    // buffer whose DMA to HBM overlaps the next file's packing and the workers' selection.
    const size_t s0 = dump ? 0 : f0, s1 = dump ? files.size() : f1;
    std::mutex sel_mu;
    std::condition_variable sel_cv;
    std::vector<char> sel_done(files.size(), 0);
    std::atomic<size_t> sel_next{s0};
    auto sel_work = [&]() {
        for (size_t f; (f = sel_next.fetch_add(1)) < s1;) {
            select_build_sequences(fm, files[f], (unsigned)f, MaxSequencesPerFile, deleted_fids, batches[f]);
            std::lock_guard<std::mutex> g(sel_mu);
            sel_done[f] = 1;
            sel_cv.notify_all();
        }
    };
    std::vector<std::thread> sel_pool;
    for (int t = 0; t < std::max(1, n_threads - 1); ++t) sel_pool.emplace_back(sel_work);
    auto join_selection = [&]() {
        for (auto& t : sel_pool)
            if (t.joinable()) t.join();
    };
    if (dump) {
        hip_warm.join();
        join_selection();
        if (rank != 0) return 0;
        dump_extract(op.get("dump-extract"), files, batches);
        std::cerr << "wrote build input to " << op.get("dump-extract") << "\n";
        std::cerr << "phases: parse " << t_parse << " parse_files " << t_files << " defs " << t_defs << " fm_load " << t_fm
                  << "\n";
        if (!mesh.wait_children(err)) die(err);
        return 0;
    }

    skm_build* b = nullptr;
    skm_build_opts bo{};
    bo.k = K;
    bo.max_seqs_per_file = MaxSequencesPerFile;
    bo.n_functions = std::max(1u, nkept_f);
    bo.canonical_order = 1;
    bo.rank = rank;
    bo.world_size = world;
    auto check = [](int rc, const char* what) {
        if (rc) die(std::string(what) + ": " + skm_last_error());
    };
    hip_warm.join();
    const double t_create0 = now_s();
    check(skm_build_create(&b, &device, 1, &bo), "skm_build_create");
    {
        uint64_t nres = 0, nseq = 0;
        for (size_t f = f0; f < f1; ++f) {
            nres += files[f].n_residues;
            nseq += files[f].size();
        }
        check(skm_build_reserve(b, nres, nseq), "skm_build_reserve");
    }
    // test hook (tests/test_gpu_cli.py): this rank fails before joining the communicator
    if (const char* fail = std::getenv("SKM_CLI_FAIL_RANK"))
        if (world > 1 && std::atoi(fail) == rank) die("injected failure (SKM_CLI_FAIL_RANK)");
    skm_transport tp = mesh.transport();
    if (world > 1 && comm == "host") {
        check(skm_build_set_transport(b, &tp), "skm_build_set_transport");
    } else if (world > 1) {
        uint8_t id[128] = {0};
        if (rank == 0) check(skm_comm_unique_id(id), "skm_comm_unique_id");
        if (launched) {
            const std::string cf = op.get("comm-file", path_join(kmer_data_dir.empty() ? "." : kmer_data_dir, ".skm_comm_id"));
            if (!file_rendezvous(cf, rank, id, 300.0, err)) die(err);
        } else if (!mesh.share_id(id, err)) {
            die(err);
        }
        check(skm_build_set_comm(b, id), "skm_build_set_comm");
    }
    const double t_create = now_s() - t_create0;
    const double t_add0 = now_s();
    uint64_t host_residue_bytes = 0;
    double t_add_fasta = 0;
    if (fasta_dev) {
        add_files_on_device(b, files, batches, f0, f1, fasta_group_bytes, device,
                            [&](size_t f) {
                                std::unique_lock<std::mutex> g(sel_mu);
                                sel_cv.wait(g, [&] { return sel_done[f] != 0; });
                            },
                            host_residue_bytes);
        uint64_t ctr[51] = {0};
        if (skm_build_counters(b, ctr, 51) > 50) t_add_fasta = 1e-6 * (double)ctr[50];
    }
    for (size_t f = f0; f < f1 && !fasta_dev; ++f) {
        {
            std::unique_lock<std::mutex> g(sel_mu);
            sel_cv.wait(g, [&] { return sel_done[f] != 0; });
        }
        const BuildBatch& bb = batches[f];
        if (bb.off.empty()) continue;
        check(skm_build_add_batch(b, files[f].residues.data(), bb.off.data(), bb.len.data(), bb.func.data(),
                                  bb.seq_id.data(), bb.off.size()),
              "skm_build_add_batch");
    }
    join_selection();
    const double t_add = now_s() - t_add0;
    std::cerr << "process kmers\n";
    t0 = now_s();
    check(skm_build_prepare(b), "skm_build_prepare");
    const double t_prepare = now_s() - t0;
    t0 = now_s();
    check(skm_build_run(b), "skm_build_run");
    const double t_run = now_s() - t0;
    t0 = now_s();
    skm_kept kept{};
    if (kept_on_device)
        check(skm_build_stats(b, &kept), "skm_build_stats");
    else
        check(skm_build_finish(b, &kept), "skm_build_finish");
    const uint64_t kept_host_bytes = kept.keys ? (8 + sizeof(skm_stored_kmer_data)) * kept.n : 0;
    const double t_finish = now_s() - t0;
    float ph[12] = {0};
    int nph = skm_build_last_timings(b, ph, 12);
    const double t_build = t_prepare + t_run + t_finish;
    // --perfect-hash-source device: the hash and its data file from the arena while the handle still
    // holds it; its DB is closed before the recall table is allocated (the peel state and that table
    // are the two largest transients)
    double t_mph = 0;
    if (ph_source == "device") {
        const double tm = now_s();
        std::cerr << "build perfect hash into " << quoted(ph_file) << " with data in " << quoted(ph_data) << "\n";
        skm_mph_db_opts mo{};
        mo.seed = mph_seed;
        mo.release_work = release_level;
        mo.mph_path = ph_file.c_str();
        mo.dat_path = ph_data.c_str();
        skm_db* mdb = nullptr;
        check(skm_build_mph_db(b, &mo, &mdb, nullptr), "skm_build_mph_db");
        skm_db_close(mdb);
        t_mph = now_s() - tm;
        std::cerr << "Wrote " << kept.n << " values\n";
    }
    // --recall-db device: the recall DB from the arena while the handle still holds it (the work
    // buffers go first: the table needs their room at the headline size)
    skm_db* kdb = nullptr;
    if (recall_db == "device") {
        skm_kept_db_opts ko{};
        ko.release_work = release_level;
        check(skm_build_kept_db(b, &ko, &kdb), "skm_build_kept_db");
    }
    // --final-kmers-source device: the handle lives until the final.kmers thread has written the file;
    // --recall-source device: until the recall has read its sequences
    if (fk_source != "device" && !recall_resident) {
        skm_build_destroy(b);
        b = nullptr;
    }
    if (rank != 0) {  // rank 0 holds every kept k-mer and the all-reduced statistics
        skm_kept_free(&kept);
        return 0;
    }
    std::cout << "Kept " << kept.n << " kmers\n";
    std::cout << "distinct_signatures=" << kept.distinct_signatures << "\n";
    std::cout << "num_seqs_with_a_signature=" << kept.n_seqs_with_signature << "\n";

    std::thread final_kmers_thread;
    double t_final_kmers = 0;
    if (!final_kmers.empty() && path_is_relative(final_kmers)) {
        final_kmers = path_join(kmer_data_dir, final_kmers);
        std::cerr << "Updated final_kmers to " << quoted(final_kmers) << "\n";
    }
    auto start_final_kmers = [&]() {
        if (final_kmers.empty()) return;
        final_kmers_thread = std::thread([&]() {
            const double tk = now_s();
            std::cerr << "writing kmers to " << quoted(final_kmers) << "\n";
            if (fk_source == "device")  // from here on this thread alone touches the build handle
                check(skm_build_write_final_kmers(b, final_kmers.c_str(), nullptr), "skm_build_write_final_kmers");
            else
                write_final_kmers(final_kmers, kept, std::max(1, n_threads / 2));
            t_final_kmers = now_s() - tk;
            std::cerr << "writing kmers to " << quoted(final_kmers) << " complete\n";
        });
    };
    // A handle is driven by one thread at a time.  With --recall-source device and
    // --final-kmers-source device both the recall and the dump use the build handle: the recall
    // (tens of milliseconds of device time) goes first and the dump's thread starts after it, beside
    // the reports; the recall's batch buffers are then allocated before the dump sizes its chunk
    // from the memory that is free.
    const bool dump_after_recall = recall_resident && fk_source == "device";
    if (!dump_after_recall) start_final_kmers();

    {
        std::ofstream df(path_join(kmer_data_dir, "distinct_functions"));
        for (uint32_t f = 0; f < kept.n_functions; ++f)
            if (kept.distinct_functions[f]) df << f << "\t" << fm.lookup_function((uint16_t)f) << "\t" << kept.distinct_functions[f] << "\n";
    }

    const std::string report_dir = path_join(kmer_data_dir, "recall.report.d");
    if (mkdir(report_dir.c_str(), 0777) != 0) std::cerr << "mkdir " << quoted(report_dir) << " failed\n";
    const std::string fi_file = path_join(kmer_data_dir, "function.index");

    std::thread perfect_hash_thread;
    int ph_rc = 0;
    std::string ph_err;
    if (!ph_file.empty() && ph_source == "host") {
        const uint32_t seed = mph_seed;
        perfect_hash_thread = std::thread([&, seed]() {
            const double tm = now_s();
            std::cerr << "build perfect hash into " << quoted(ph_file) << " with data in " << quoted(ph_data) << "\n";
            ph_rc = skm_mph_build_device(kept.keys, kept.data, kept.n, seed, ph_file.c_str(), ph_data.c_str(), device);
            t_mph = now_s() - tm;
            if (ph_rc)
                ph_err = skm_last_error();
            else
                std::cerr << "Wrote " << kept.n << " values\n";
        });
    }

    // recall of the training sequences with the new k-mers (kmers-build-signatures.cc:238-349)
    std::vector<std::string> fidx;
    if (!read_function_index(fi_file, fidx, err)) die(err);
    std::cerr << "Begin recall\n";
    t0 = now_s();
    if (!kdb) check(skm_db_open_kept(&kdb, kept.keys, kept.data, kept.n, device), "skm_db_open_kept");
    std::vector<const FastaFile*> fptr;
    for (auto& f : files) fptr.push_back(&f);
    std::vector<std::vector<SeqCall>> calls;
    double recall_dev_ms = 0;
    uint64_t recall_deferred = 0;
    skm_fidx* fx = nullptr;  // --best-call device: find_best_call on the recall's resident calls
    if (!best_call_tables(recall_resident ? "device" : best_call, fidx, device, &fx, err)) die(err);
    ResidentRecall rr;
    if (recall_resident) {
        if (call_files_resident(b, kdb, fptr, batches, fidx, n_threads, fx, calls, err, &rr)) die(err);
        if (dump_after_recall) start_final_kmers();
        recall_dev_ms = rr.device_ms;
        recall_deferred = rr.deferred;
    } else if (call_files(kdb, fptr, fidx, false, n_threads, calls, err, &recall_dev_ms, 2000000000ull, nullptr, nullptr,
                          fx, &recall_deferred)) {
        die(err);
    }
    skm_fidx_destroy(fx);
    skm_db_close(kdb);
    {  // one report per file (kmers-build-signatures.cc:300-349), the files on the host threads
        std::atomic<size_t> next_f{0};
        auto report = [&]() {
            for (size_t f; (f = next_f.fetch_add(1)) < files.size();) {
                std::map<std::string, std::string> data;  // saver::data (first emplace wins), sorted by id
                for (size_t r = 0; r < files[f].size(); ++r) {
                    const std::string& id = files[f].ids[r];
                    const SeqCall& c = calls[f][r];
                    std::string orig, orig_stripped;
                    fm.lookup_original_assignment(id, orig, orig_stripped);
                    if (orig_stripped != c.func && !data.count(id))
                        data.emplace(id, id + "\t" + orig + "\t" + orig_stripped + "\t" + c.func + "\t" +
                                             std::to_string((int)c.fi) + "\t" + fmt_g(c.score) + "\n");
                }
                std::string text;
                for (auto& e : data) text += e.second;
                std::ofstream of(path_join(report_dir, files[f].filename));
                of.write(text.data(), (std::streamsize)text.size());
            }
        };
        std::vector<std::thread> th;
        for (int t = 1; t < std::min<int>(n_threads, (int)files.size()); ++t) th.emplace_back(report);
        report();
        for (auto& t : th) t.join();
    }
    const double t_recall = now_s() - t0;
    const double t_recall_dev = recall_dev_ms / 1000.0;

    if (op.has("nudb-file")) std::cerr << "--nudb-file: NuDB output is not supported by this build; skipped\n";
    if (perfect_hash_thread.joinable()) {
        std::cerr << "Awaiting completion of perfect hash creation\n";
        perfect_hash_thread.join();
        if (ph_rc) die("perfect hash: " + ph_err);
    }
    if (final_kmers_thread.joinable()) {
        std::cerr << "Awaiting completion of final kmers dump\n";
        final_kmers_thread.join();
    }
    skm_build_destroy(b);
    skm_kept_free(&kept);
    if (!mesh.wait_children(err)) die(err);
    std::cerr << "timing: parse " << t_parse << " s, build " << t_build << " s (device pipeline "
              << (nph > 7 ? ph[7] : 0.0f) << " ms), recall " << t_recall << " s, total " << now_s() - t_start << " s\n";
    // one machine-readable line of the phases (bench.py's cli_build leg)
    std::cerr << "phases: parse " << t_parse << " add " << t_add << " prepare " << t_prepare << " run " << t_run
              << " finish " << t_finish << " final_kmers " << t_final_kmers << " mph " << t_mph << " recall "
              << t_recall << " recall_device " << t_recall_dev << " total " << now_s() - t_start << " startup "
              << t_startup << " defs " << t_defs << " hip_init " << t_hip_init << " create " << t_create
              << " parse_files " << t_files << " fm_load " << t_fm << " recall_deferred " << recall_deferred
              << " kept_host_bytes " << kept_host_bytes;
    if (fasta_dev) std::cerr << " add_fasta " << t_add_fasta << " host_residue_bytes " << host_residue_bytes;
    if (recall_resident)  // appended pairs (the line's readers take pairs); host mode's line is unchanged
        std::cerr << " recall_resident_seqs " << rr.resident_seqs << " recall_uploaded_seqs " << rr.uploaded_seqs
                  << " recall_batches " << rr.batches;
    std::cerr << "\n";
    std::cerr << "all done\n";
    fast_exit(0);  // every output file is closed by now
}
