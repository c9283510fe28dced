// skm_fasta.h -- the device FASTA parser (skm_fasta.hip) as the query code uses it: raw file bytes
// in, the packed residues, QMeta and window offsets of a resident query out (FastaParser,
// fasta_parser.h:38-144, as parse_fasta_impl in front/skm_front.cpp restates it).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "skm_lookup.h"
#include "skm_util.h"

namespace skm {

// chunk geometry (skm_fasta_parse_info): bytes per thread per step (one 16-byte load), per wave
// step, and per workgroup tile (the unit of the cross-workgroup scans)
constexpr uint32_t FA_BYTES = 16, FA_THREADS = 256, FA_WAVE_BYTES = 64 * FA_BYTES, FA_TILE = FA_THREADS * FA_BYTES;

// device work buffers of the parser; they only grow, so a reused query allocates nothing once it
// has seen its largest batch
struct FastaWork {
    DevBuf d_raw;     // the file bytes, padded with '\r' to a whole tile
    DevBuf d_foff;    // file_off [n_files + 1]
    DevBuf d_tmap;    // per tile: its transition map, then (k_fasta_map_scan) its entry state
    DevBuf d_tcnt;    // per tile: (kept residues, kept records), then their exclusive sums; + totals
    DevBuf d_pstart;  // per kept record: its packed start
    DevBuf d_nwin;    // per kept record: max(len - 7, 0)
    DevBuf d_tab;     // the download: error flag, file_rec, hdr_pos, seq_len
    Scanner scan;
    hipEvent_t ev[4] = {};
    ~FastaWork();
};

struct FastaTotals {
    uint64_t n_recs = 0, n_residues = 0, rp = 0, n_windows = 0;
    float ms = 0;
};

// SKM_E_ARG unless file_off ascends from 0 and bytes is there when file_off[n_files] > 0
void fasta_check_args(const uint8_t* bytes, const uint64_t* file_off, size_t n_files);

// Parses bytes[0, file_off[n_files]) on the current device, on stream st.  d_res gets the packed
// residues (record s at pstart[s] = sum over t < s of (len[t] + 1), a 0 after each, the tail zeroed
// and padded as query_setup leaves it), d_meta the QMeta and d_scr_off the n_recs + 1 window
// offsets.  tab (optional) gets the host table; its residues only with want_residues.  Returns with
// the stream idle.
FastaTotals fasta_parse(FastaWork& w, const uint8_t* bytes, const uint64_t* file_off, size_t n_files, hipStream_t st,
                        DevBuf& d_res, DevBuf& d_meta, DevBuf& d_scr_off, int want_residues, skm_fasta_table* tab);

}  // namespace skm
