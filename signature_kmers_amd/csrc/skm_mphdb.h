// skm_mphdb.h -- the BDZ signature DB made on the device from a build's kept arena
// (skm_build_mph_db): what the build side (skm_build.hip) calls in the DB side (skm_annotate.hip).
#pragma once
#include <cstdint>

#include "../../include/skm.h"

namespace skm {
// A full BDZ DB (g, rank table, records, record words, b = 7 pair lines) over n >= 1024 distinct
// keys and their records resident on `device`, both read in place: the peel, assign and place
// kernels take d_keys / d_data as they are, and the DB keeps neither array.  Nothing that touches
// the two arrays may be in flight.  o->mph_path / o->dat_path, each if given, are written from the
// device buffers.
skm_db* db_from_device_mph(const uint64_t* d_keys, const skm_stored_kmer_data* d_data, uint64_t n,
                           const skm_mph_db_opts* o, int device, skm_mph_stats* st);
// The same DB for fewer than 1024 keys: the host builder over the downloaded keys (ascending),
// opened from memory.
skm_db* db_from_host_mph(const uint64_t* keys, const skm_stored_kmer_data* data, uint64_t n, const skm_mph_db_opts* o,
                         int device, skm_mph_stats* st);
// skm_mph_db_plan's four numbers for n keys (validates n)
void mph_db_plan(uint64_t n, uint64_t out[4]);
}  // namespace skm
