// skm_keptdb.h -- the exact-key DB made on the device from a build's kept arena
// (skm_build_kept_db): what the build side (skm_build.hip) calls in the DB side (skm_annotate.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/skm.h"

namespace skm {
// An exact DB with a range-reduced table of `slots` (> n) slots over n distinct non-zero keys and
// their records resident on `device`, read in place and inserted on st; the DB keeps neither array.
skm_db* db_from_device_kept(const uint64_t* d_keys, const skm_stored_kmer_data* d_data, uint64_t n, uint64_t slots,
                            int device, hipStream_t st);
// the table size of skm_build_kept_db for n keys (validates opts)
uint64_t kept_db_slots(uint64_t n, const skm_kept_db_opts* opts);
}  // namespace skm
