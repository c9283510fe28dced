/*
 * skm.h -- C-ABI of libskm, the MI355X-native signature-k-mer engine.
 *
 * This is the drop-in boundary for the reference's hot path (olsonanl/signature_kmers @ 2024-11-15).
 * The reference has no FFI; its boundary is a C++ template API.  Each entry point below names the
 * reference interface it replaces (paths relative to the reference's src/).
 *
 * Conventions
 *   - Plain C types only.  No exceptions cross the boundary.
 *   - Return value: 0 = OK, < 0 = error class (SKM_E_*).  skm_last_error() holds a message
 *     (thread-local).
 *   - Host buffers passed in are caller-owned and are copied before the call returns.
 *   - Buffers returned in out-structs are library-owned; release them with the matching *_free.
 *   - A k-mer key is the 8 residue bytes as a little-endian uint64 (byte 0 = first residue),
 *     i.e. Kmer<8> = std::array<char,8> reinterpreted (kmer_data.h:37).
 *   - Handles are driven from one host thread at a time.
 */
#ifndef SKM_H
#define SKM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SKM_OK 0
#define SKM_E_ARG -1      /* invalid argument / limit exceeded                    */
#define SKM_E_HIP -2      /* HIP runtime error (incl. no device)                  */
#define SKM_E_OOM -3      /* device or host allocation failed                     */
#define SKM_E_IO -4       /* file I/O or format error                             */
#define SKM_E_COMM -5     /* RCCL error                                           */
#define SKM_E_STATE -6    /* call out of order                                    */

#define SKM_UNDEFINED_FUNCTION 0xFFFFu /* kmer_data.h:23 UndefinedFunction */

/* StoredKmerData (kmer_data.h:114-128): five little-endian u16, 10 bytes, the kmer_data.dat
 * record (perfect_hash.h:62 writes sizeof(StoredKmerData)=10 per MPH slot).  Natural layout:
 * sizeof 10, alignof 2, offsets 0/2/4/6/8 -- equal to the reference as g++ compiles it
 * (tests/golden/ref_split.npz `layout`, tests/test_ref_pin_cpu.py). */
typedef struct skm_stored_kmer_data {
    uint16_t avg_from_end;
    uint16_t function_index;
    uint16_t mean;
    uint16_t median;
    uint16_t var;
} skm_stored_kmer_data;

/* KmerCall (call_functions.h:23-48). 24 bytes. */
typedef struct skm_kmer_call {
    uint32_t start;
    uint32_t end;
    int32_t count;
    uint16_t function_index;
    uint16_t pad;
    uint32_t protein_length_median;
    float protein_length_med_avg_dev;
} skm_kmer_call;

const char* skm_last_error(void);
const char* skm_version(void);
int skm_device_count(int* n);
/* hipMemGetInfo of a device: the bytes free for allocation right now, and the device's total */
int skm_device_mem_info(int device, uint64_t* free_bytes, uint64_t* total_bytes);

/* ------------------------------------------------------------------------------------------
 * Signature build.  Replaces SignatureBuilder<K>::extract_kmers + process_kmers
 * (signature_build.h:55-110, signature_build.tcc:48-293) as driven by kmers-build-signatures.cc
 * :193-196, and the consumers kept_kmers()/kmer_stats() (signature_build.h:106-107).
 * ------------------------------------------------------------------------------------------ */
typedef struct skm_build skm_build;

typedef struct skm_build_opts {
    int32_t k;                  /* must be 8 (kmers-build-signatures.cc:17 K=8)                 */
    uint32_t max_seqs_per_file; /* 100000 (kmers-build-signatures.cc:18); informational        */
    uint32_t n_functions;       /* size of function.index (FunctionIndex upper bound, < 65535)  */
    int32_t canonical_order;    /* 1: n_threads=1 reference semantics (the only mode)           */
    int32_t rank;               /* this process's rank (0 for single GPU)                        */
    int32_t world_size;         /* number of GPUs/processes: 1, 2, 4 or 8                        */
} skm_build_opts;

/* Kept k-mers (KeptKmers<8>, signature_build.h:52-53) + KmerStatistics (:44-50). */
typedef struct skm_kept {
    uint64_t* keys;                  /* [n] k-mer keys, sorted ascending                       */
    skm_stored_kmer_data* data;      /* [n] packed 10-byte records                              */
    uint64_t n;                      /* kept k-mers ("Kept N kmers")                            */
    uint32_t* distinct_functions;    /* [n_functions] kept k-mers per best function              */
    uint32_t* seqs_with_func;        /* [n_functions] sequences per function                    */
    uint32_t n_functions;
    uint64_t n_seqs_with_signature;  /* "num_seqs_with_a_signature="                            */
    uint64_t distinct_signatures;    /* "distinct_signatures="                                  */
    uint64_t n_windows;              /* windows examined (metric units)                         */
    uint64_t n_records;              /* valid windows (occurrences)                             */
} skm_kept;

/* devices: HIP device ordinals (n_devices == 1 per process; multi-GPU is one process per GPU). */
int skm_build_create(skm_build** out, const int* devices, int n_devices, const skm_build_opts* opts);

/* One batch of sequences in reference emission order (file order, then sequence order).
 * residues: concatenated residue bytes; sequence s is residues[seq_off[s] .. +seq_len[s]).
 * seq_func: FunctionIndex of the sequence's assigned function, or 0xFFFF when the sequence has
 *           no kept function (the reference skips it, signature_build.tcc:133-158).
 * seq_id:   file_number*max_seqs_per_file + k (signature_build.tcc:91,138).                   */
int skm_build_add_batch(skm_build* b, const uint8_t* residues, const uint64_t* seq_off,
                        const uint32_t* seq_len, const uint16_t* seq_func, const uint32_t* seq_id,
                        size_t n_seqs);

/* skm_build_add_batch with FastaParser in front of it (fasta_parser.h:38-144 feeding the selection
 * of signature_build.tcc:84-102 and :93-158), on the device: the files' raw bytes in (bytes /
 * file_off / n_files as skm_fasta_parse_device takes them, declared below with skm_fasta_table),
 * the selected records' residues parsed straight into the build's resident buffer -- no host copy of
 * a residue.  rec_func[r] and rec_id[r] describe parser record r of this call (the records with a
 * non-empty id, in file order: skm_fasta_table's numbering): rec_func as seq_func (0xFFFF = the
 * record is not selected, e.g. no kept function or a deleted feature), rec_id as seq_id (may be
 * NULL, with the same rule).  Staged add_batch residues are flushed first, so add_batch and
 * add_fasta calls may be mixed and give the sequence order of the calls; works at any world size
 * (a rank adds its own files).  tab (optional, overwritten; skm_fasta_table_free) gets the table
 * over every parser record, without residues, for the caller to check against its headers-only
 * parse.  SKM_E_ARG, with the handle's input as it was before the call (a handle that was prepared
 * stays prepared, unless the refusal is the record longer than 1,048,575 residues, which is found
 * after the parse wrote its scratch past the packed residues: the next call prepares again): n_recs differs from the number of
 * parser records the device finds (the message gives both), a selected rec_func >= n_functions, a
 * selected record longer than 1,048,575 residues (an unselected one may be), or the argument
 * errors of skm_fasta_parse_device. */
struct skm_fasta_table;
int skm_build_add_fasta(skm_build* b, const uint8_t* bytes, const uint64_t* file_off, size_t n_files,
                        const uint16_t* rec_func, const uint32_t* rec_id, uint64_t n_recs,
                        struct skm_fasta_table* tab);

/* Optional capacity hint: the total residues and sequences that will be added, so the HBM
 * residue buffer is allocated once instead of grown.  Batches stream to HBM as they are added,
 * packed into two pinned staging buffers that alternate (the host packs one while the DMA engine
 * copies the other); the caller may overlap parsing with add_batch (kmers-build-signatures does).
 * Replaces nothing in the reference (its build reads the FASTA into host memory,
 * signature_build.tcc:48-70); new in this port. */
int skm_build_reserve(skm_build* b, uint64_t n_residues, uint64_t n_seqs);

/* Flush the last staging buffer, pack the metadata into HBM (idempotent). */
int skm_build_prepare(skm_build* b);
/* Run the device pipeline over the resident input; results stay on the device. */
int skm_build_run(skm_build* b);
/* Device time (ms) of the last run's phases: [0]=extract-count [1]=scan [2]=extract-scatter
 * [3]=bucket-process (partition + group-by) [4]=overflow (own stream, overlaps [3]) [5]=chains
 * [6]=stats (+ reductions) [7]=total [8]=exchange (world_size > 1) [9]=level-2 partition kernel
 * [10]=group-by kernel alone [11]=groups of > 64 members (k_big_groups + append);
 * returns entries written. */
int skm_build_last_timings(skm_build* b, float* ms, int cap);
/* [12] of skm_build_last_timings: the long-chain tail -- device time from the end of the last
 * key-range pass on the group-by stream until the last stashed P^2 / variance chain is done.
 * [13], [14]: the start and end of the run's first giant-chain launch (k_heavy's chains of
 * >= 2^giant_class samples; with route_first the heavy-only pass 0's), in ms from the run's
 * start; -1 when no giant chain ran.
 * [15], [16]: the main stream's waits for a pass tail on the tail stream (one GPU with key-range
 * passes), summed over the passes: [15] a staging's wait for the end of the tail of the pass
 * before last, whose element buffer it overwrites (inside [2]'s span); [16] a group-by's wait for
 * the previous tail's job sort, after which the job and big-group lists are free. */
/* Per-kernel device time (diagnostics and the bench's roofline): with enable != 0 every kernel
 * launch of a run -- or only the launches of the kernel named `only` (e.g. "k_bucket_process";
 * NULL = all) -- is bracketed by an event pair on its stream, and after the run's host
 * synchronisation the durations are summed by kernel name.  skm_build_kernel_timings returns the
 * number of kernels of the last run and writes, for the first `cap`, the total ms and launch count
 * and (names != NULL) their names, one per line.  New in this port (the reference has no device
 * code; its only timing is the stderr phase banners, kmers-build-signatures.cc:178-325). */
int skm_build_set_kernel_timing(skm_build* b, int enable, const char* only);
int skm_build_kernel_timings(skm_build* b, char* names, size_t names_cap, float* ms, uint64_t* launches, int cap);
/* Counters of the last run: [0]=windows [1]=kept (owned by this rank) [2]=overflow sub-buckets
 * [3]=chain jobs [4]=chain samples [5]=sequences [6]=occurrences grouped on this rank
 * [7]=occurrences in overflow sub-buckets [8]=k-mers kept by the overflow path
 * [9]=groups of > 64 members handed to k_big_groups [10]=k-mers kept among them
 * [11]=key-range passes [12]=valid windows (occurrences) this rank extracts [13]=giant chains
 * (heavy k-mers whose P^2 / variance chains start right after k_heavy) [14]=the longest of them
 * [15]=redone steps since create (a run that outgrew a data-sized work buffer -- the overflow
 * scratch, the split path, the stashed long chains -- records its demand and is redone once with
 * the buffers grown; the capacities persist, so later runs on the same input are not)
 * [16..19]=capacities of those buffers (overflow scratch elements, split-path elements, stashed
 * long-chain samples, stashed long jobs) [20..23]=the last run's demands on them [24]=samples of
 * the stashed long chains (chains of >= 2^14 samples with key-range passes) [25]=occurrences of
 * heavy k-mers routed into the first half of the key-range passes ("route_heavy_min");
 * [26]=host microseconds in skm_build_add_batch (all calls; the residues are packed by a pool of
 * host threads, SKM_HOST_THREADS or min(16, hardware threads)), and prepare's phases in
 * microseconds: [27] the residue / metadata upload, [28] the pass plan (device tallies of the pass
 * sizes, heavy-key routing sketch and filter), [29] allocations and the rest; [30] residue scans
 * per run that emit the key-range passes' window positions (k_pass_emit, one per group of up to
 * four passes; 0 without key-range passes); [31] of [26]: microseconds packing residues into the
 * pinned staging buffers, [32] of [26]: microseconds waiting for a staging buffer's DMA to end;
 * totals over the passes of the run; the last skm_build_finish / _finish_slice's kept-set
 * hand-off (device radix sort in key-range chunks, streamed through pinned staging): [33] its
 * host microseconds, [34] of them waiting for the device / PCIe, [35] copying pieces out on the
 * host pool, [36] chunks, and its device microseconds summed over the chunks: [37] selection,
 * [38] radix sort, [39] gather, [40] the D2H pieces; [41] the largest hand-off chunk (k-mers),
 * [42] 1 if the hand-off used 64-bit arena indices (>= 2^32 k-mers); [43] the kept arena's
 * capacity (k-mers); [44] device bytes free after prepare; [45] reserved, always 0 (it keeps
 * the places of the slots after it); [46] overflow sub-buckets whose light remainder (what is left once
 * the heavy k-mers are split off, at most 2048 occurrences) was grouped by the LDS hash path
 * (k_ovf_light) instead of the overflow sort, [47] the occurrences in them (both 0 with
 * "ovf_light" 0; their kept k-mers count in [8], those of their groups of > 64 members in [10]);
 * [48] (bucket, part) tasks of the group-by's queue that held a batch (k_bucket_process: a bucket
 * is eight parts of its level-2 sub-buckets, or one task when it is grouped unpartitioned), [49]
 * the LDS batches (process_sub calls) they made; both totals over the passes of the run, and both
 * fixed by the input and the pass count, not by the schedule;
 * [50] device microseconds of skm_build_add_fasta's parses (all calls; the call's host time counts
 * in [26]);
 * returns entries written. */
int skm_build_counters(skm_build* b, uint64_t* out, int cap);
/* Host transport: the rank collectives of a multi-process build run by the caller on host
 * buffers, for ranks joined by a channel other than RCCL (the tests drive it with
 * torch.distributed gloo; production multi-GPU runs use skm_build_set_comm).  The library stages
 * device data through host memory around each call.  Every callback returns 0 on success. */
typedef struct skm_transport {
    void* ctx;
    /* variable all-to-all (bytes): send + soff[q] (scnt[q] bytes) goes to rank q, which receives
     * it at recv + roff[p] (rcnt[p] bytes) for source p */
    int (*alltoallv)(void* ctx, const void* send, const uint64_t* scnt, const uint64_t* soff, void* recv,
                     const uint64_t* rcnt, const uint64_t* roff);
    /* in-place element-wise reduction over the ranks: op 0 = u32 sum (mod 2^32), 1 = u8 max */
    int (*allreduce)(void* ctx, void* data, uint64_t count, int op);
    /* every rank's bytes_per_rank[r] bytes, concatenated in rank order into recv */
    int (*allgatherv)(void* ctx, const void* send, void* recv, const uint64_t* bytes_per_rank);
} skm_transport;
/* Join the ranks through a host transport instead of RCCL (world_size > 1; copied). */
int skm_build_set_transport(skm_build* b, const skm_transport* tp);
/* Test hooks (host only, no device): the exchange planning of one key-range pass as rank `rank`
 * of `world`: bucket_starts [world*nb1+1] are this rank's owner-major level-1 bucket starts; the
 * per-bucket counts go through tp->alltoallv; out: recv_off/recv_cnt [world] (elements, source
 * order) and vstart [nb1+1] (bucket-major starts of the received elements).  And a self-check of
 * the three callbacks (returns 0 when every collective gave the expected result). */
int skm_debug_exchange_plan(const skm_transport* tp, int rank, int world, uint32_t nb1, const uint64_t* bucket_starts,
                            uint64_t* recv_off, uint64_t* recv_cnt, uint64_t* vstart);
int skm_debug_transport_check(const skm_transport* tp, int rank, int world);

/* Build options beyond skm_build_opts (take effect at the next prepare/run):
 *   "key_range_passes"        0 = automatic; else P = 1, 2, 4 .. 64 passes over disjoint k-mer
 *                             ranges (top bits of the key hash).  The reference holds the whole
 *                             proteome in one multimap (signature_build.h:61,122); a GPU shard
 *                             whose occurrences exceed the work buffers is grouped pass by pass,
 *                             with identical results (each k-mer lives in exactly one pass).
 *   "device_memory_budget_mb" memory the automatic pass count plans for (0 = free memory).
 * Diagnostic tunables (defaults are the tuned values): "overflow_heavy_min",
 *   "overflow_inline_min", "overflow_inline_prio", "overflow_long_class", "overflow_chain_wgs",
 *   "chain_prio", "bucket_prio", "chain_lds_kb", "host_timing",
 *   "heavy_min" (occurrences that send a k-mer to the heavy path), "split_min" (overflow
 *   sub-buckets at least this large are split into heavy keys + a light remainder),
 *   "ovf_light" (1, the default: a light remainder of at most 2048 occurrences is grouped by the
 *   LDS hash path of the group-by, k_ovf_light; 0: every remainder goes through the overflow
 *   sort, as larger ones always do -- same results),
 *   "heavy_lsd" (1: every heavy k-mer through round 3's Boyer-Moore + LSD-sort path instead of
 *   the one-read bucketed path; it is the fallback for > 4096 functions or crowded buckets),
 *   "giant_class" (heavy chains of >= 2^class samples start right after the heavy kernel on
 *   their own streams; 0 = off; default: 14 with one pass or world_size > 1, off with key-range
 *   passes on one GPU),
 *   "giant_passes", "prefetch" (the next pass group's positions, k_pass_emit, during the group-by of the group's
 *   last pass, 1),
 *   "overflow_grid" / "split_grid" / "chain_grid" (persistent-grid sizes), "stream_priority"
 *   (1: the group-by stream at the highest priority), "chain_batches" (key-range passes: the
 *   stashed long chains leave in this many batches, 2) / "chain_streams" (over 1..4 streams, 1),
 *   "work_buffer_elements" (capacity of the data-sized work buffers; tests force the
 *   grow-and-redo path with a small value; 0 = automatic), "poison_jobs" (tests: canary jobs in
 *   the stashed long-job list), "route_heavy_min" (one GPU, >= 4 key-range passes: k-mers with at
 *   least this many occurrences -- estimated at prepare from a count-min sketch of 1/64 of the
 *   windows -- are grouped in the first half of the passes, so their long P^2 chains run beside
 *   the later passes instead of after the last one; 16384; 0 = off), "route_vacate" (the last
 *   this many passes hold no routed heavy key, whose keys are spread over the others by hash;
 *   0 = the second half, mapped to pass - P/2), "route_first" (every routed heavy k-mer in a
 *   heavy-only pass 0, the light keys of pass 0 spread over the others, the pass count doubled
 *   below four passes: 1 = on, 0 = off; default on at world_size > 1), "route_first_min" (its
 *   occurrence threshold, 131072), "tail_async" (one GPU, key-range passes: a pass's big groups,
 *   chains and accounting on their own stream beside the next pass's staging; 1),
 *   "stage_round" (key-range passes: 1 = the staged position scatter in half rounds of 2048
 *   elements, four workgroups per CU, the default; 0 = rounds of 4096), "serial_overflow"
 *   (diagnostics: 1 = a pass's overflow path starts after its group-by kernel; 0), "chain_cus"
 *   (the stashed long chains' stream confined to this many CUs, a multiple of 8; 0 = all),
 *   "side_cus" (the same for the overflow streams and the next pass's selection),
 *   "big_split" (tail_async: the two big-group size classes on two tail streams; 0),
 *   "heavy_grid" (k_heavy's persistent grid, 512),
 *   "lane_long" (key-range passes: stashed long chains below this many samples run one lane each,
 *   64 chains per wave, instead of on a wave pair; 2^20; 0 = all on wave pairs), "lane_grid"
 *   (their grid, 256), "lane_tail" (the threshold for the batch after the last pass, 2^16),
 *   "lane_streams" (their batches rotate over 1..4 streams, 1),
 *   "sub_target" (k_partition's target elements per level-2 sub-bucket; 0 = 768),
 *   "part_order" (k_partition's workgroups take the buckets of more than twice the mean size
 *   first; 1), "big_grid" / "big_grid_large" (k_big_groups' persistent grids),
 *   "emit_group" (key-range passes emitted per residue scan: 0 = 4, or 1, 2, 4, 8, 16),
 *   "handoff_index_limit" / "handoff_max_chunk" (tests: force the hand-off's 64-bit indices /
 *   small chunks), "final_kmers_piece_kb" (tests: skm_build_write_final_kmers' pinned piece size
 *   in KB, 1 .. 2^20; 0 = 64 MB).
 * Unknown names and out-of-range values return SKM_E_ARG. */
int skm_build_set_option(skm_build* b, const char* name, int64_t value);
/* Diagnostics: copy the per-phase cycle sums of the last run (if enabled) into out, then
 * enable/disable stamping for subsequent runs. */
int skm_build_debug_stamps(skm_build* b, int enable, uint64_t* out, int cap);
/* Diagnostics: lengths of the first cap chain jobs of the last pass in execution order (longest
 * first; the overflow's list when the pass had overflow sub-buckets). */
int skm_build_debug_jobs(skm_build* b, uint32_t* out, int cap);
/* Diagnostics: element counts of the last pass's overflow sub-buckets as the partition listed
 * them; returns how many there are (at most cap written). */
int skm_build_debug_overflow(skm_build* b, uint32_t* out, int cap);
/* Diagnostics (read-only, after a run): the geometry of the extraction front end, at most cap of
 * out[0..11) = residue bytes with separators (rp), emission rows (sel_wg), windows per emission
 * row (sel_span), passes emitted per residue scan (emit_g), the staged scatter's span and
 * workgroups over a pass's position list (pf_span, pf_nwg), the one-pass extract workgroups and
 * their span (nwg, span), pass_bits, owner_bits, b1_bits.  The five key-range-pass values
 * (sel_wg .. pf_nwg) are 0 after a one-pass run.  Returns 11, SKM_E_STATE without a completed run. */
int skm_build_debug_front(skm_build* b, uint64_t* out, int cap);
/* Diagnostics (read-only, after skm_build_prepare): the resident input as the kernels read it --
 * *rp = the packed residue bytes (every sequence's residues and a 0 after each), *nseq = the
 * sequences; res_out (optional, res_cap >= *rp bytes) gets d_res[0, rp), meta_out (optional,
 * meta_cap >= *nseq records) the sequence table, 16 bytes a sequence: pstart u64, len u32, func
 * u16, pad u16.  Call it with both NULL for the sizes.  New in this port (the reference keeps its
 * input in host strings, signature_build.tcc:48-70).  SKM_E_STATE before prepare. */
int skm_build_debug_input(skm_build* b, uint8_t* res_out, uint64_t res_cap, void* meta_out, uint64_t meta_cap,
                          uint64_t* rp, uint64_t* nseq);
/* Diagnostics (read-only, after a run with key-range passes): the staging's exact starts of `pass`,
 * a pass of the run's last emission group: (pf_nwg + 1) rows of 64, row w column d = where staging
 * workgroup w begins in level-0 slice d, row pf_nwg = the slices' ends (at most cap written);
 * returns the value count.  SKM_E_ARG for a pass of an earlier group, SKM_E_STATE after one pass. */
int skm_build_debug_stage_starts(skm_build* b, uint32_t pass, uint64_t* out, int cap);
/* Diagnostics (read-only, after a run): this rank's window count of every key-range pass of the
 * last run, after any heavy-key routing (at most cap written); returns the pass count.  With one
 * pass: the single valid window count. */
int skm_build_debug_pass_windows(skm_build* b, uint64_t* out, int cap);
/* Diagnostics: device time of the chain kernel on njobs synthetic jobs of length n
 * (mode 0: the build's choice by length, 1: one lane per chain, 2: one wave pair per chain;
 *  3 / 5: the P^2 wave alone, previous / current walk; 4: the variance wave alone). */
int skm_debug_chain_bench(uint32_t n, uint32_t njobs, int mode, float* ms);
/* Diagnostics: the P^2 median and the variance (raw doubles) of one chain of n samples in visit
 * order, by the per-lane (mode 1) or the wave-pair (mode 2) chain code. */
int skm_debug_chain_eval(const uint32_t* samples, uint32_t n, int mode, double* median, double* var);
/* Diagnostics: device exact-division helpers (reciprocal + corrected quotient used by the
 * statistics recurrences) against IEEE division: m = 1..nm, then nm*per random pairs. */
int skm_debug_div_check(uint64_t nm, uint32_t per, uint64_t* mismatches);
/* Run (if not yet run since the last prepare) and download the result, keys ascending (sorted
 * on the device in key-range chunks and streamed to the host arrays; the reference's KeptKmers is
 * a hash map, kmers-build-signatures.cc:206-221, so any order is valid).  At most 2^32 - 1 kept
 * k-mers per call (use skm_build_finish_slice beyond).  With world_size > 1 this is collective:
 * rank 0 receives every rank's kept k-mers, the other ranks the k-mers they own; the statistics
 * are global on every rank. */
int skm_build_finish(skm_build* b, skm_kept* out);
/* The kept k-mers of one output slice: those whose slice hash -- MurmurHash3's fmix64 of the
 * little-endian key, top slice_bits bits -- equals `slice` (0 <= slice < 2^slice_bits, slice_bits
 * <= 16; slice_bits 0 = every kept k-mer), keys sorted, with the build's global statistics.  The
 * 2^slice_bits slices partition the kept set, so a caller streams an output too large for one
 * host copy slice by slice (the 50M-protein build keeps ~2.9G k-mers).  The reference writes
 * final.kmers / the .dat from one in-memory KeptKmers map (kmers-build-signatures.cc:198-264);
 * its order is hash order, so slices written one after another are a valid final.kmers.
 * n_seqs_with_signature counts sequences (not distinct seq ids).  With world_size > 1: this
 * rank's own k-mers of the slice (not collective for the keys; distinct_signatures is global). */
int skm_build_finish_slice(skm_build* b, int slice_bits, uint32_t slice, skm_kept* out);
/* The last run's per-sequence signature flags (KmerStatistics::seqs_with_a_signature, signature_
 * build.tcc:275, as a bitmap over the sequences with a kept function in add order; world_size > 1:
 * every rank's sequences in rank order): min(cap, sequences) bytes of 0/1. */
int skm_build_signature_flags(skm_build* b, uint8_t* out, uint64_t cap);
void skm_kept_free(skm_kept* k);
void skm_build_destroy(skm_build* b);

/* ------------------------------------------------------------------------------------------
 * Multi-GPU (one process per GPU; opts.rank / opts.world_size, a power of two).  Rank r adds
 * the r-th contiguous range of files (emission order is rank order).  Rank 0 calls
 * skm_comm_unique_id, the caller broadcasts the 128 bytes (e.g. torch.distributed over gloo),
 * every rank passes them to skm_build_set_comm (collective) before prepare/run.  Owner of a
 * k-mer = top bits of its hashed key; occurrence elements are exchanged with one RCCL
 * all-to-all over xGMI, then per-function counts (sum) and signature flags (max) are
 * all-reduced.  prepare / run / finish are collective.
 * ------------------------------------------------------------------------------------------ */
int skm_comm_unique_id(uint8_t id[128]);
int skm_build_set_comm(skm_build* b, const uint8_t id[128]);
/* Test/diagnostic transport: run n handles of ranks 0..n-1 (world_size n) in this process,
 * exchanging through device copies instead of RCCL; skm_build_finish on any member afterwards. */
int skm_build_group_run(skm_build* const* bs, int n);

/* ------------------------------------------------------------------------------------------
 * Signature DB (CmphKmerDb<StoredKmerData,8>, cmph_kmer.h:28-164).  Reads a cmph BDZ dump
 * (<dir>/kmer_data.mph) + the dense record file (<dir>/kmer_data.dat) and lays g, the rank table
 * and the records out contiguously in HBM.
 * ------------------------------------------------------------------------------------------ */
typedef struct skm_db skm_db;

int skm_db_open(skm_db** out, const char* mph_path, const char* dat_path, int device);
int skm_db_open_mem(skm_db** out, const uint8_t* mph, size_t mph_len, const uint8_t* dat,
                    size_t dat_len, int device);
/* Exact-key DB over the kept k-mers of a build: KeptKmerDB<K> (kept_kmer_db.h:9-31), used by the
 * recall pass of kmers-build-signatures (kmers-build-signatures.cc:238-349).  A window hits only
 * if its k-mer is one of keys (record data[i]); keys must be distinct and non-zero.  Laid out in
 * HBM as an open-addressing table (load <= 1/2) + the 10-byte records.  skm_db_lookup returns
 * the record index, or n for a miss.                                                          */
int skm_db_open_kept(skm_db** out, const uint64_t* keys, const skm_stored_kmer_data* data, size_t n, int device);

/* The same exact-key DB made on the device from a finished build, without a host copy of the kept
 * set.  Its table is range-reduced: any number of 16-byte slots (key, record index, function_index
 * << 16 | mean), not a power of two and possibly more than 2^32; a key's home slot is the high 64
 * bits of fmix64(key) * slots, and probing is linear with a wrap at the table's end. */
typedef struct skm_kept_db_opts {
    uint32_t load_pct;      /* 0 = 40; else 10..95: slots = max(16, ceil(100 n / load_pct)).  The
                               recall lookup at load 0.6 measured 31-41 % slower than on the host
                               path's table, at 0.5 5-16 % slower, at 0.4 8-13 % faster
                                                                           */
    int32_t  release_work;  /* 1: free the build handle's per-pass work buffers first (below);
                               2: the same, but keep the resident sequences (skm_build_recall)  */
    uint64_t slots;         /* 0 = from load_pct; else exactly this many slots (> n); tests and
                               callers that size the table themselves                           */
} skm_kept_db_opts;

/* Exact-key DB (KeptKmerDB, kept_kmer_db.h:20-27) over the kept k-mers of b's last run, built on
 * b's device from the resident arena: no host copy of keys or records. opts NULL = defaults.
 * Runs the build first if it has not run since prepare (as skm_build_finish does).  world_size > 1
 * returns SKM_E_STATE (the kept set is sharded over the ranks).  At most 2^32 - 2 kept k-mers.
 * The DB is independent of b: it holds the table only -- not the 10-byte records, so
 * skm_matrix_create / skm_matrix_batch_create over it return SKM_E_ARG -- and skm_db_lookup returns
 * a k-mer's index in b's arena (a permutation of 0..n-1 over the members; n for a miss).  When the
 * table cannot be allocated the call returns SKM_E_OOM with the bytes asked for and the bytes free
 * in skm_last_error(), and b stays usable.
 * release_work = 1 frees every device buffer of b except the kept arena, the statistics and the
 * signature flags before the table is allocated (and whether or not that allocation succeeds):
 * skm_build_finish, _finish_slice, _signature_flags and _counters return what they returned before,
 * and every call that would need the freed buffers -- skm_build_add_batch, _reserve, _prepare,
 * _run, _group_run, and a finish after skm_build_set_option -- returns SKM_E_STATE.  Such a handle
 * is only read out and destroyed.  release_work = 2 frees the same buffers except the residues and
 * the sequence table, which skm_build_recall reads; the same calls return SKM_E_STATE afterwards.  A
 * later release_work = 1 frees those two as well.  Other non-zero values return SKM_E_ARG. */
int skm_build_kept_db(skm_build* b, const skm_kept_db_opts* opts, skm_db** out);

/* host only: the table skm_build_kept_db would allocate for n keys */
int skm_kept_db_plan(uint64_t n, const skm_kept_db_opts* opts, uint64_t* slots, uint64_t* bytes);
/* host only (test hook): the home slot of key in a table of `slots` slots -- the same function the
 * device uses */
int skm_debug_kept_slot(uint64_t key, uint64_t slots, uint64_t* slot);
/* batched record word of a key as the call path reads it: function_index << 16 | mean, or
 * 0xFFFFFFFF for a miss (BDZ DBs: whatever record the search lands on, as fetch does). Any DB. */
int skm_db_lookup_fm(skm_db* db, const uint64_t* keys, size_t n, uint32_t* fm_out);
/* out[0]=slots [1]=table bytes [2]=keys [3]=longest probe sequence seen at insert (slots examined
 * by one key, 1 = every key sits in its home slot; 0 for a table made by skm_db_open_kept, which
 * does not record it) [4]=1 if range-reduced (made by skm_build_kept_db); 0s for a BDZ DB;
 * returns entries written */
int skm_db_table_info(skm_db* db, uint64_t* out, int cap);
/* cmph_size() (cmph_kmer.h:102); for an exact DB the number of kept k-mers */
int skm_db_size(skm_db* db, uint32_t* m);
/* Batched cmph_search(hash, key, 8) (cmph_kmer.h:90-92); idx >= size is a miss. */
int skm_db_lookup(skm_db* db, const uint64_t* keys, size_t n, uint32_t* idx_out);
/* test hook: the same search through the generic bdz_search walk (any b), bypassing the b == 7
 * (g word, rank) pair lines that skm_db_lookup / the annotate kernels use when present */
int skm_debug_db_lookup_generic(skm_db* db, const uint64_t* keys, size_t n, uint32_t* idx_out);
void skm_db_close(skm_db* db);

/* Build a BDZ minimal perfect hash over keys (build_perfect_hash, perfect_hash.h:11-69):
 * writes a cmph-compatible .mph image and the .dat records (data[i] goes to slot search(key i)).
 * seed: initial PRNG seed for the hash seed draws (cmph uses rand() % 15).                     */
int skm_mph_build(const uint64_t* keys, const skm_stored_kmer_data* data, size_t n, uint32_t seed,
                  const char* mph_path, const char* dat_path);

/* skm_mph_build with the construction on a GPU: same parameters and image format, the
 * 3-hypergraph peeled in parallel rounds and g assigned round by round on `device`, the rank
 * table and records placed from the device lookup.  Deterministic for a given (keys, seed).
 * device < 0 (or fewer than 1024 keys) runs the host builder.                                */
int skm_mph_build_device(const uint64_t* keys, const skm_stored_kmer_data* data, size_t n, uint32_t seed,
                         const char* mph_path, const char* dat_path, int device);

/* skm_mph_build_device with phase times and an optional on-device check, for builds up to the
 * headline kept set (cmph's 32-bit m, n = 3r: n < 2^32, i.e. about 3.4 G keys).  mph_path /
 * dat_path may be NULL (that image is not written).  verify != 0: every key's slot is < n and
 * distinct (a slot bitmap), the annotate kernels' b == 7 pair-line search equals the generic
 * bdz_search for every key, and .dat[slot] equals the key's record; a failure returns
 * SKM_E_STATE.  Replaces build_perfect_hash (perfect_hash.h:11-69) as kmers-build-signatures
 * runs it over the whole kept set (kmers-build-signatures.cc:253-264). */
typedef struct skm_mph_stats {
    double upload_s, peel_s, assign_s, rank_s, place_s, verify_s, write_s, total_s;
    uint64_t n_keys, n_vertices;
    uint32_t attempts, peel_rounds;
    int32_t verified;      /* 1: the check above ran and passed */
    int32_t pad;
} skm_mph_stats;
int skm_mph_build_device_ex(const uint64_t* keys, const skm_stored_kmer_data* data, size_t n, uint32_t seed,
                            const char* mph_path, const char* dat_path, int device, int verify,
                            skm_mph_stats* stats);

/* The BDZ signature DB -- what build_perfect_hash writes (perfect_hash.h:11-69) and
 * CmphKmerDb::load_hash / load_data read back (cmph_kmer.h:95-104) -- made and opened on the
 * device from a finished build, without the host copy of the kept set, the second upload and the
 * file round trip of skm_build_finish + skm_mph_build_device + skm_db_open. */
typedef struct skm_mph_db_opts {
    uint32_t seed;          /* as skm_mph_build_device's seed                                   */
    int32_t  release_work;  /* as skm_kept_db_opts.release_work, the same contract (0, 1, 2)    */
    int32_t  verify;        /* as skm_mph_build_device_ex's verify                              */
    int32_t  pad;
    const char* mph_path;   /* NULL = not written                                               */
    const char* dat_path;   /* NULL = not written                                               */
} skm_mph_db_opts;

/* A full BDZ DB over the kept k-mers of b's last run, on b's device, independent of b: every call
 * that takes a DB opened by skm_db_open works on it (skm_db_lookup, _lookup_fm, skm_annotate,
 * skm_query_*, skm_matrix_*, skm_matrix_batch_*), and skm_db_table_info returns zeros as for any
 * BDZ DB.  opts NULL = seed 1, nothing released, checked or written.  Runs the build first if it
 * has not run since prepare.  world_size > 1 returns SKM_E_STATE; more kept k-mers than one BDZ
 * holds (n = 3r < 2^32, about 3.4 G keys) SKM_E_ARG; a failed device allocation SKM_E_OOM with the
 * bytes asked for and the bytes free in skm_last_error(), and b stays usable.  release_work = 1
 * is skm_build_kept_db's: the same buffers go, before anything is allocated, and the same calls
 * return SKM_E_STATE afterwards.
 * From 1024 kept k-mers on, everything stays on the device: the peel, assign and place kernels of
 * skm_mph_build_device read the keys and records in place from the arena (its keys are distinct by
 * construction, so there is no duplicate check), the rank table is counted and scanned on the
 * device from g, and the records, record words and b = 7 pair lines are written straight into the
 * DB's buffers.  The peel does not depend on the order of the keys, so the image and the .dat are
 * byte for byte those of skm_mph_build_device over the sorted kept set with the same seed.  g and
 * the rank table come to the host only when mph_path is given (the cmph dump); dat_path is written
 * from the DB's record array.  Below 1024 kept k-mers the sorted kept set is downloaded and the
 * host builder runs, as in skm_mph_build_device.  stats (may be NULL): upload_s stays 0, write_s
 * covers the files. */
int skm_build_mph_db(skm_build* b, const skm_mph_db_opts* opts, skm_db** out, skm_mph_stats* stats);
/* host only: for n kept k-mers, out[0] = r of the first attempt (ceil(1.23 n / 3) made odd),
 * [1] = vertices (3r), [2] = device bytes of the open DB, [3] = the most device bytes live at one
 * time during skm_build_mph_db, the arena not counted (the peel state: 16 bytes per vertex and 5
 * per key).  n above the BDZ limit returns SKM_E_ARG.  Callers decide on release_work with it. */
int skm_mph_db_plan(uint64_t n, uint64_t out[4]);

/* final.kmers written from the resident arena, formatted on the device -- the third product of
 * the kept set (with skm_build_kept_db and skm_build_mph_db) that needs no host copy of it.
 * Replaces the dump loop of kmers-build-signatures.cc:198-221: one line per kept k-mer,
 *   KMER '\t' avg_from_end '\t' function_index '\t' '\n'
 * KMER = the 8 key bytes as they are, the two numbers as decimals without leading zeros; lines in
 * ascending key order (the order of skm_build_finish; the reference's is hash order). */
typedef struct skm_final_kmers_stats {
    uint64_t n_kmers, bytes, chunks, pieces; /* lines, file bytes, key-range chunks, pinned pieces  */
    double total_s, wait_s, write_s;         /* host seconds: the call, of them waiting for the
                                                device / PCIe, and in pwrite                      */
    float select_ms, sort_ms, gather_ms, format_ms, d2h_ms; /* device ms summed over the chunks and
                                                pieces; gather_ms is 0: the format kernels read
                                                keys and records through the sorted index       */
    uint32_t wide_index;                     /* 1: 64-bit arena indices ("handoff_index_limit")   */
} skm_final_kmers_stats;
/* kmers-build-signatures.cc:198-221.  Runs the build first if it has not run since prepare (as
 * skm_build_finish does), then sorts the arena's keys chunk by chunk as the finish hand-off does,
 * formats each chunk's lines on the device and streams the text through two pinned pieces into
 * `path` (pwrite at each piece's file offset).  The file is created and truncated before anything
 * else runs; no kept k-mer gives an empty file.  world_size > 1 returns SKM_E_STATE before that
 * (no file is made).  An open, write or close error returns SKM_E_IO with the path in
 * skm_last_error(); the file may then be partial, and b stays usable.  Works on a handle whose
 * work buffers were released (skm_build_kept_db / skm_build_mph_db release_work).  stats may be
 * NULL.  Options: "handoff_index_limit" / "handoff_max_chunk" as for the finish hand-off, and
 * "final_kmers_piece_kb" (tests: the pinned piece size in KB, 1 .. 2^20; 0 = 64 MB). */
int skm_build_write_final_kmers(skm_build* b, const char* path, skm_final_kmers_stats* stats);
/* kmers-build-signatures.cc:198-221 (the stdout lines and distinct_functions around the dump):
 * everything skm_build_finish returns except the arrays -- keys and data are NULL; n,
 * distinct_functions, seqs_with_func, n_functions, n_seqs_with_signature (distinct seq ids where
 * they collide, as skm_build_finish counts them), distinct_signatures, n_windows and n_records are
 * filled.  Runs the build first if needed; works after a release; world_size > 1 returns
 * SKM_E_STATE.  Free with skm_kept_free. */
int skm_build_stats(skm_build* b, skm_kept* out);
/* kmers-build-signatures.cc:198-221 has no geometry (it is a loop over a map); the device
 * formatter's: lines per emit tile (one workgroup), threads per workgroup, the longest line in
 * bytes (22), reserved (0).  Host only. */
int skm_final_kmers_info(uint32_t out[4]);
/* kmers-build-signatures.cc:198-221 on the host (test hook, no device): the lines of n kept k-mers
 * through the formatter the device kernels run (csrc/skm_finalkmers.h).  *len = the total length,
 * also when cap is too small; then only the whole lines that fit in cap bytes are written. */
int skm_debug_final_kmers_host(const uint64_t* keys, const skm_stored_kmer_data* data, size_t n, uint8_t* out,
                               size_t cap, uint64_t* len);

/* ------------------------------------------------------------------------------------------
 * Function calling.  Replaces FunctionCaller<CmphKmerDb>::process_aa_seq for a batch of query
 * sequences (call_functions.tcc:259-338 + HitSet :6-108, window iterator kmer_data.h:76-102).
 * find_best_call (call_functions.tcc:347-659): skm_find_best_call for one sequence on the host;
 * for a batch, on the host or on the resident calls, the "Best call per sequence" section below.
 * ------------------------------------------------------------------------------------------ */
typedef struct skm_annot_opts {
    int32_t min_hits;      /* 5   (call_functions.h:66)                                   */
    int32_t max_gap;       /* 200                                                          */
    int32_t ignore_hypo;   /* --ignore-hypo                                                */
    int32_t hypo_index;    /* index of "hypothetical protein" in function.index           */
    int32_t mean_mode;     /* Boost.Math mean: 0 = >=1.76 four-lane (default), 1 = <=1.75  */
    int32_t mad_mode;      /* MAD: 0 = |x(mid)-median| (>=1.76), 1 = |x(mid)| (older Boost,  */
                           /* libstdc++ nth_element order)                      */
} skm_annot_opts;

typedef struct skm_calls {
    uint64_t* call_off;    /* [n_seqs+1] CSR offsets                                       */
    skm_kmer_call* calls;  /* [n_calls]                                                    */
    uint64_t n_seqs;
    uint64_t n_calls;
    uint64_t n_windows;    /* query windows examined                                       */
} skm_calls;

typedef struct skm_query skm_query;
/* Upload a batch of query sequences (residues/seq_off/seq_len as in skm_build_add_batch). */
int skm_query_create(skm_query** out, skm_db* db, const uint8_t* residues, const uint64_t* seq_off,
                     const uint32_t* seq_len, size_t n_seqs);
/* Device pipeline (window lookup + HitSet) on resident queries; calls stay on the device. */
int skm_query_run(skm_query* q, const skm_annot_opts* opts);
int skm_query_last_timings(skm_query* q, float* ms, int cap);
/* Download the calls of the last run. */
int skm_query_calls(skm_query* q, skm_calls* out);
/* The last run's per-window hits as the device lookup produced them (diagnostics and parity tests
 * of the device window iterator, kmer_data.h:76-102, and fetch, cmph_kmer.h:139-147; the CLI's
 * --debug-hits prints them as the reference's hit_cb does, kmers-call-functions.cc:109-118):
 * hit_off [n_seqs+1] CSR offsets; for the first `cap` hits pos = the window's offset in its
 * sequence and fm = function_index << 16 | mean of its record (either array may be NULL).
 * *n_out = the total number of hits. */
int skm_query_window_hits(skm_query* q, uint64_t* hit_off, uint32_t* pos, uint32_t* fm, uint64_t cap, uint64_t* n_out);
void skm_query_destroy(skm_query* q);
/* Convenience: create + run + calls, through one query object the DB keeps for these calls (its
 * device buffers, stream and host threads reused from batch to batch; released by
 * skm_db_close).  A batch laid out packed -- seq_off[s] = sum over t < s of (seq_len[t] + 1),
 * i.e. one byte after every sequence -- is uploaded as it is (the bytes between sequences are not
 * read as residues); any other layout is packed on the host first.  Like every call on a handle,
 * from one host thread at a time per DB. */
int skm_annotate(skm_db* db, const uint8_t* residues, const uint64_t* seq_off, const uint32_t* seq_len,
                 size_t n_seqs, const skm_annot_opts* opts, skm_calls* out);
void skm_calls_free(skm_calls* c);

/* ------------------------------------------------------------------------------------------
 * FASTA parsed on the device: raw file bytes in, a resident query out.  Replaces FastaParser
 * (fasta_parser.h:38-144, fasta_parser.cc:17-36) for the sequence bodies, and the per-record
 * copies of FunctionCaller::process_fasta_stream (call_functions.tcc:217-255): the packed
 * residues, the per-sequence table and the window offsets are built in HBM.  Ids and definition
 * lines stay host string work (the headers-only host parse).
 *
 * bytes[0, file_off[n_files]) = the files back to back, file f at [file_off[f], file_off[f+1])
 * (file_off ascends from 0; empty files allowed).  Every file is parsed as the reference parses
 * it: '\r' dropped in every state, bytes before the first '>' and every byte the reference reports
 * as an error dropped, a record ended by a '>' at a line start or by the end of its file
 * (parse_complete()), a record with an empty id dropped with its residues -- as every caller of
 * the reference skips it (signature_build.tcc:124).  Error reports are not made here.
 * ------------------------------------------------------------------------------------------ */
typedef struct skm_fasta_table {
    uint64_t n_files, n_recs, n_residues, n_windows;
    uint64_t* file_rec;   /* [n_files+1] first kept record of each file; [n_files] = n_recs  */
    uint32_t* seq_len;    /* [n_recs]                                                       */
    uint64_t* hdr_pos;    /* [n_recs] position in bytes[] of the record's '>'               */
    uint8_t*  residues;   /* packed (record s at sum over t < s of (seq_len[t] + 1), a 0    */
                          /* after each), only when asked for (tests, diagnostics); else NULL */
    float parse_ms;       /* device time of the parse                                       */
} skm_fasta_table;

/* The device parser's chunk geometry (fasta_parser.h:38-144 has none: it is a byte loop): bytes
 * per thread per step, bytes per wave per step, bytes per workgroup tile, reserved (0). */
int skm_fasta_parse_info(uint32_t out[4]);
/* FastaParser::parse + parse_complete (fasta_parser.h:38-144, fasta_parser.cc:17-36) over every
 * file, on `device`: the table of the kept records (*out is overwritten; release it with
 * skm_fasta_table_free).  SKM_E_ARG: a null array, a file_off that does not ascend from 0,
 * >= 2^32 - 1 kept records, a record longer than 2^32 - 2 residues. */
int skm_fasta_parse_device(const uint8_t* bytes, const uint64_t* file_off, size_t n_files, int device,
                           int want_residues, skm_fasta_table* out);
/* skm_query_create from file bytes (FastaParser, fasta_parser.h:38-144, feeding process_aa_seq as
 * process_fasta_stream does, call_functions.tcc:217-255): parses straight into the query's own
 * device buffers (no second device copy of the residues; the raw bytes live in a buffer of the
 * query that only grows).  The result is an ordinary skm_query: query s is kept record s.  tab
 * (optional, overwritten) gets the table, without residues. */
int skm_query_create_fasta(skm_query** out, skm_db* db, const uint8_t* bytes, const uint64_t* file_off,
                           size_t n_files, skm_fasta_table* tab);
/* skm_annotate from file bytes (process_fasta_stream, call_functions.tcc:217-255, with FastaParser,
 * fasta_parser.h:38-144, on the device): parse + run + calls through the query object the DB keeps
 * for skm_annotate; a later skm_annotate on the same DB is unaffected. */
int skm_annotate_fasta(skm_db* db, const uint8_t* bytes, const uint64_t* file_off, size_t n_files,
                       const skm_annot_opts* opts, skm_calls* calls, skm_fasta_table* tab);
/* Releases the arrays of a table filled by the three calls above (fasta_parser.h:38-144 has no
 * counterpart: its records are std::strings). */
void skm_fasta_table_free(skm_fasta_table* t);

/* ------------------------------------------------------------------------------------------
 * All-vs-all shared-signature-k-mer counts.  Replaces MatrixDistance::compute
 * (matrix_distance.h:45-170) as run by kmers-matrix-distance (kmers-matrix-distance.cc:94-212):
 * process_aa_seq with ignore_hypothetical(true) feeds hit_cb (:123-152: hits whose seqlen lies
 * outside mean +/- 2 sd of the record are dropped; sd = sqrt(var), or 0.1 seqlen when var == 0),
 * kmer_hit_map[kmer] = set of SeqIdMap indices (seq_id_map.h:12-27), seq_dist[id1][id2]++ for
 * every id1 < id2 of a k-mer's set (:176-196).
 * ------------------------------------------------------------------------------------------ */
typedef struct skm_matrix skm_matrix;

typedef struct skm_matrix_opts {
    int32_t hypo_index;       /* function index of "hypothetical protein" (dropped); -1: none    */
    uint32_t row_begin;       /* count only pairs with id1 in [row_begin, row_end): this GPU's    */
    uint32_t row_end;         /* tile of the triangle (skm_matrix_tile_rows); 0, 0 = every row    */
    uint32_t pad;
    uint64_t max_tile_bytes;  /* reserved (0): the counts live in per-row LDS histograms, no dense
                                 tile is allocated in HBM                                        */
} skm_matrix_opts;

typedef struct skm_pairs {
    uint32_t* pairs;          /* [n][3] = (id1, id2, count), id1 < id2, sorted by (id1, id2)      */
    uint64_t n;
    uint64_t n_hits;          /* (kmer, sequence) hit records that passed the filters            */
} skm_pairs;

/* seq_idx[s]: SeqIdMap index of sequence s (index of the first sequence with its id, in input
 * order; < n_idx).  residues / seq_off / seq_len as in skm_build_add_batch. */
int skm_matrix_create(skm_matrix** out, skm_db* db, const uint8_t* residues, const uint64_t* seq_off,
                      const uint32_t* seq_len, const uint32_t* seq_idx, size_t n_seqs, uint32_t n_idx);
/* Device pipeline on the resident queries; the pairs stay on the device. */
int skm_matrix_run(skm_matrix* m, const skm_matrix_opts* opts);
/* Multi-GPU matrix distance: rank `rank` of `world` created its handle over its
 * own contiguous range of the query sequences, with the global SeqIdMap indices and n_idx (every
 * rank's the same).  After joining the ranks -- a host transport (copied) or an RCCL communicator
 * (rank 0's skm_comm_unique_id, collective) -- skm_matrix_run is collective: each rank looks up
 * only its own queries (kmers-matrix-distance.cc:123-152 hit_cb), every (k-mer, index) hit goes
 * to the k-mer's owner GPU (all-to-all), the owner builds its k-mers' kmer_hit_map entries and
 * sends each one's index set to the GPUs whose row band (skm_matrix_tile_rows) it has pairs in
 * (all-to-all), and each GPU counts the pairs of its band (:176-196); opts row_begin / row_end are
 * ignored, and skm_matrix_pairs returns the band's pairs (concatenate the ranks' in rank order). */
int skm_matrix_set_transport(skm_matrix* m, int rank, int world, const skm_transport* tp);
int skm_matrix_set_comm(skm_matrix* m, int rank, int world, const uint8_t id[128]);
/* [0]=hits [1]=group (hash + sort) [2]=pair increments [3]=compaction [4]=total (ms) */
int skm_matrix_last_timings(skm_matrix* m, float* ms, int cap);
/* [0]=windows [1]=hit records [2]=pair increments [3]=nonzero pairs [4]=distinct hit k-mers
 * (kmer_hit_map.size(), kmers-matrix-distance.cc:169; with ranks: the k-mers this rank owns)
 * [5]=hits of this handle's queries [6]=with ranks: index entries routed to this rank's band */
int skm_matrix_counters(skm_matrix* m, uint64_t* out, int cap);
int skm_matrix_pairs(skm_matrix* m, skm_pairs* out);
void skm_pairs_free(skm_pairs* p);
void skm_matrix_destroy(skm_matrix* m);
/* Row band of rank `rank` of `world` GPUs with (nearly) equal triangle area. */
int skm_matrix_tile_rows(uint32_t n_idx, int rank, int world, uint32_t* row_begin, uint32_t* row_end);

/* Batched matrix distance: P independent problems (one family's sequences each) in one device
 * pass.  Problem p owns the sequences [prob_seq[p], prob_seq[p+1]) and its own SeqIdMap index
 * space [0, prob_nidx[p]); seq_idx[s] is local to the problem of s.  A k-mer that occurs in
 * several problems pairs sequences only within each of them: every problem's pairs equal those
 * of skm_matrix_* run on that problem alone.  The number of host synchronisations of a run does
 * not depend on P. */
typedef struct skm_matrix_batch skm_matrix_batch;
typedef struct skm_matrix_batch_opts {
    int32_t hypo_index;       /* as skm_matrix_opts                                               */
    uint32_t small_cols;      /* 0 = built-in limit (1024); else min(small_cols, 1024): rows of
                                 problems with more indices take the large-row kernel            */
} skm_matrix_batch_opts;
int skm_matrix_batch_create(skm_matrix_batch** out, skm_db* db, const uint8_t* residues, const uint64_t* seq_off,
                            const uint32_t* seq_len, const uint32_t* seq_idx, const uint64_t* prob_seq,
                            const uint32_t* prob_nidx, size_t n_prob);
/* Reusable: a second run gives the same pairs. */
int skm_matrix_batch_run(skm_matrix_batch* b, const skm_matrix_batch_opts* opts);
/* Triples with problem-local indices, sorted by (problem, id1, id2); problem p's are
 * [prob_off[p], prob_off[p+1]).  prob_off has P+1 entries.  Free with skm_pairs_free. */
int skm_matrix_batch_pairs(skm_matrix_batch* b, skm_pairs* out, uint64_t* prob_off);
/* [0]=windows [1]=hit records [2]=pair increments [3]=nonzero pairs [4]=groups (distinct
 * (problem, k-mer)) [5]=rows (indices) on the small path [6]=rows on the large path */
int skm_matrix_batch_counters(skm_matrix_batch* b, uint64_t* out, int cap);
/* out[P]: groups of each problem of the last run -- its kmer_hit_map size (matrix_distance.h:110) */
int skm_matrix_batch_group_counts(skm_matrix_batch* b, uint64_t* out);
/* as skm_matrix_last_timings */
int skm_matrix_batch_last_timings(skm_matrix_batch* b, float* ms, int cap);
void skm_matrix_batch_destroy(skm_matrix_batch* b);

/* find_best_call (call_functions.tcc:347-659) on the host.  function_index: nfunc C strings
 * (function.index column 1).  out_func receives the called function (NUL-terminated).      */
int skm_find_best_call(const skm_kmer_call* calls, size_t ncalls, const char* const* function_index,
                       size_t nfunc, uint16_t* out_fi, float* out_score, float* out_offset,
                       char* out_func, size_t out_func_cap);

/* ------------------------------------------------------------------------------------------
 * Best call per sequence for a whole batch, on the host or on the device.  The same decision as
 * skm_find_best_call (call_functions.tcc:347-659) made on ids: the strings of function.index are
 * reduced once to tables (skm_fidx: the rank of every name under std::string order, and string-pool
 * ids of the name and of its split(" / ") parts), and one core (csrc/skm_bestcall.h) runs per
 * sequence in a device kernel and in the host batch function alike.
 *
 * The core declines ("defers") a sequence only when it has more than SKM_BEST_MAX_CALLS calls or
 * one of its calls names a function of more than SKM_BEST_MAX_PARTS parts; the library resolves
 * those with skm_find_best_call from that sequence's calls and reports how many there were.
 * ------------------------------------------------------------------------------------------ */
#define SKM_BEST_MAX_PARTS 8
#define SKM_BEST_MAX_CALLS 64
#define SKM_BEST_PAIR 1

typedef struct skm_fidx skm_fidx;
/* device >= 0: the tables are uploaded there too; device < 0: host only (no HIP call is made).
 * A NULL entry of function_index is the name "". */
int skm_fidx_create(skm_fidx** out, const char* const* function_index, size_t nfunc, int device);
void skm_fidx_destroy(skm_fidx* fx);

typedef struct skm_best_call {       /* 16 bytes */
    uint16_t fi;        /* out_fi of skm_find_best_call                                          */
    uint16_t fi_a, fi_b;/* SKM_BEST_PAIR: the "f1 ?? f2" functions, f1 = fi_a (the greater name); */
                        /* else SKM_UNDEFINED_FUNCTION                                           */
    uint16_t flags;     /* SKM_BEST_PAIR = 1                                                     */
    float score, offset;
} skm_best_call;
typedef struct skm_best_calls {      /* library-owned; skm_best_calls_free */
    skm_best_call* best;  /* [n_seqs] */
    uint64_t n_seqs, n_calls, n_windows, n_deferred;
    float kernel_ms;      /* device time of the best-call kernel (0 on the host)                 */
} skm_best_calls;
/* The function string find_best_call returns: name(fi), "f1 ?? f2", or "".  Returns the length
 * of the whole string (truncated to cap - 1 bytes in out), or < 0 on error. */
int skm_best_call_name(const skm_fidx* fx, const skm_best_call* c, char* out, size_t cap);

/* host batch (no device): the same core on n_threads host threads; works on a CPU-only machine.
 * Only call_off, calls and the counts of `calls` are read. */
int skm_best_calls_host(const skm_calls* calls, const skm_fidx* fx, int n_threads, skm_best_calls* out);
/* On the resident calls of q's last run: kernel on q's stream, 16 B per sequence downloaded; the
 * calls themselves are not downloaded unless a sequence was deferred.  SKM_E_ARG: fx without
 * device tables or made for another device than q's; SKM_E_STATE: q has not run. */
int skm_query_best_calls(skm_query* q, const skm_fidx* fx, skm_best_calls* out);
/* skm_annotate / skm_annotate_fasta + the above, through the DB's kept query */
int skm_annotate_best(skm_db* db, const uint8_t* residues, const uint64_t* seq_off, const uint32_t* seq_len,
                      size_t n_seqs, const skm_annot_opts* opts, const skm_fidx* fx, skm_best_calls* out);
int skm_annotate_fasta_best(skm_db* db, const uint8_t* bytes, const uint64_t* file_off, size_t n_files,
                            const skm_annot_opts* opts, const skm_fidx* fx, skm_best_calls* out,
                            skm_fasta_table* tab);
/* Test vehicle: a caller-made CSR of calls through the kernel on `device`, no DB and no fallback;
 * deferred[s] = 1 where the kernel declined (their best[] entries are then unspecified). */
int skm_debug_best_calls(const skm_kmer_call* calls, const uint64_t* call_off, size_t n_seqs,
                         const skm_fidx* fx, int device, skm_best_call* best, uint8_t* deferred, float* ms);
void skm_best_calls_free(skm_best_calls* c);

/* ------------------------------------------------------------------------------------------
 * Recall pass over a build's resident sequences.  Replaces the recall loop of
 * kmers-build-signatures.cc:266-349 (every training protein through process_aa_seq +
 * find_best_call against the DB just built) without the second host pack and upload of the
 * proteins: the build already holds them in HBM in the layout a query uses (raw letters, one 0
 * byte after each sequence, 64 zero bytes at the end), so a batch is a view into that buffer and
 * the annotate pipeline runs on it in place.  A DB goes in; 16 bytes per sequence (or the calls)
 * come out.  Nothing is copied device to device and no residue crosses PCIe.  With
 * skm_build_kept_db, skm_build_mph_db and skm_build_write_final_kmers this is the fourth user of
 * the build's resident data, and the only one that reads its input side.
 *
 * Resident sequences: those added with seq_func != 0xFFFF, in add order over all
 * skm_build_add_batch calls (the others are dropped on the host by add_batch).
 * ------------------------------------------------------------------------------------------ */
typedef struct skm_recall_opts {
    uint64_t batch_residues; /* 0 = default (2^29: about 7 B of query scratch per residue, so under 4 GB
                                a batch -- a plan, not a measured optimum).  A batch is a run of whole
                                resident sequences whose packed bytes (len + 1 each) do not exceed it; a
                                sequence that alone exceeds it is a batch of its own.  Values above 2^31
                                are taken as 2^31 */
    uint64_t first_seq, n_seqs; /* range of resident sequences; n_seqs 0 = to the end */
} skm_recall_opts;
typedef struct skm_recall_stats {
    uint64_t n_seqs, n_windows, n_calls, n_deferred, n_batches, resident_bytes;
    float view_ms, lookup_ms, calls_ms, best_ms;   /* device time summed over the batches */
    double wall_s;
} skm_recall_stats;
/* kmers-build-signatures.cc:266-349 reads its proteins from the FASTA files again; here: how many
 * sequences the handle holds and their packed bytes (len + 1 each).  Zeros once they were released
 * (release_work = 1).  Host only. */
int skm_build_resident_seqs(skm_build* b, uint64_t* n_seqs, uint64_t* n_residue_bytes);
/* kmers-build-signatures.cc:266-349 over the resident sequences [first_seq, first_seq + n_seqs) of b
 * against db, batch by batch through the query object db keeps for skm_annotate (its buffers only
 * grow; per batch the host waits where skm_query_run waits, plus once for the batch's results).
 * best and calls may each be NULL, not both: best[s] is what skm_annotate_best gives for sequence
 * first_seq + s (sequences the best-call kernel declines are resolved as skm_query_best_calls
 * resolves them; needs fx with device tables on b's device, else SKM_E_ARG), calls is what
 * skm_annotate gives (CSR, call_off global over the range).  Release them with skm_best_calls_free /
 * skm_calls_free.  db: any skm_db on b's device -- BDZ, host-built exact, or skm_build_kept_db's
 * table; another device is SKM_E_ARG.  ropts NULL = defaults; a range outside the resident
 * sequences is SKM_E_ARG.  stats may be NULL.
 * SKM_E_STATE: b is not prepared (sequences added since the last prepare included); world_size > 1
 * (a rank holds its shard's sequences only); the sequences were released (release_work = 1; the
 * message names release_work -- release_work = 2 keeps them: every buffer 1 frees except the
 * residues and the sequence table, and the same calls return SKM_E_STATE afterwards.  At the 50 M
 * proteins of the headline build that keeps about 17.3 GB; by DESIGN.md section 4's figures it fits
 * beside the 115.6 GB table, which nobody has run).  A build with no resident sequences gives zero
 * results and launches nothing.
 * The call first waits for everything the build's streams still have in flight.  It reads the
 * residues, the sequence table and the host copy of the table, and writes only db's query object;
 * but like every call on a handle it is made from the one host thread that drives b, so it does not
 * run beside skm_build_write_final_kmers on b: a caller runs the two one after the other.
 * write_final_kmers sizes its chunk from 3/4 of the memory free at its call and frees it before it
 * returns, so the recall's batch buffers are allocated either before it (and are counted out of
 * that free memory) or after it (and have the chunk's memory back); either order fits. */
int skm_build_recall(skm_build* b, skm_db* db, const skm_annot_opts* aopts, const skm_recall_opts* ropts,
                     const skm_fidx* fx, skm_best_calls* best, skm_calls* calls, skm_recall_stats* stats);
/* host only (the cut rule of skm_build_recall, csrc/skm_recallplan.h; kmers-build-signatures.cc:
 * 266-349 has no batches): the batches of the range over n_total sequences of these lengths, packed
 * as the build packs them.  *n_batches = how many; for the first cap of them out[6 i ..] = first
 * sequence, sequences, base (the view's start: the first sequence's packed start & ~15), that packed
 * start, the packed end (after the last separator), windows. */
int skm_recall_plan(const uint32_t* seq_len, uint64_t n_total, uint64_t batch_residues, uint64_t first_seq,
                    uint64_t n_seqs, uint64_t* out, uint64_t cap, uint64_t* n_batches);

#ifdef __cplusplus
}
#endif

#endif /* SKM_H */
