// skm_fasta.h -- the device FASTA parser (skm_fasta.hip) as the query code uses it: raw file bytes
// in, the packed residues, QMeta and window offsets of a resident query out (FastaParser,
// fasta_parser.h:38-144, as parse_fasta_impl in front/skm_front.cpp restates it).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <functional>
#include <vector>

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
    DevBuf d_rfunc;   // fasta_parse_select: rec_func [n_recs]
    DevBuf d_tsel;    //   per tile: (selected residues, selected records), then their exclusive sums; + totals
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

struct FastaSelect {
    uint64_t n_recs = 0, n_residues = 0;               // every parser record (non-empty id)
    uint64_t n_sel = 0, sel_residues = 0, sel_bytes = 0;  // the selected ones; sel_bytes = residues + one 0 each
    float ms = 0;
};

// The selecting parse (the build's input: FastaParser feeding the selection of
// signature_build.tcc:93-158).  rec_func[r] describes parser record r (a record with a non-empty id,
// in file order); 0xFFFF = not selected.  SKM_E_ARG when the bytes hold another number of parser
// records than n_recs (nothing is written then).  reserve(sel_bytes) is called once the selected
// size is known (not when it is 0) and returns where the selected records go: their residues and a 0
// after each, back to back, at any byte address; at most sel_bytes - 1 bytes are written -- the 0 after
// the last selected record is the caller's.  sel_pstart[r] = the packed start of record r relative
// to that address (~0 when r is not selected); *tab = fasta_parse's table over every parser record,
// without residues (the caller frees it).  Returns with the stream idle.
FastaSelect fasta_parse_select(FastaWork& w, const uint8_t* bytes, const uint64_t* file_off, size_t n_files,
                               const uint16_t* rec_func, uint64_t n_recs, hipStream_t st,
                               const std::function<uint8_t*(uint64_t)>& reserve, std::vector<uint64_t>& sel_pstart,
                               skm_fasta_table* tab);

}  // namespace skm
