// skm_recall.h -- the recall pass over a build's resident sequences (skm_build_recall): what the
// build side (skm_build.hip) calls in the query side (skm_annotate.hip).
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/skm.h"
#include "skm_recallplan.h"

namespace skm {
// The annotate pipeline over the batches of `plan` (skm_recallplan.h), read in place from d_res (the
// packed residues of the whole build, a 0 after each sequence, 64 zero bytes after the last) and
// d_meta (one 16-byte record per resident sequence: u64 pstart, u32 len, 4 bytes not read here --
// the build's SeqMeta, laid out as QMeta), through the query object the DB keeps for skm_annotate.
// Nothing running on the device may still write either buffer.  best / calls: either may be NULL;
// both are filled over the plan's whole range (call_off global).  stats is filled except wall_s
// and resident_bytes.
void recall_resident(skm_db* db, const uint8_t* d_res, const void* d_meta, const std::vector<RecallBatch>& plan,
                     const skm_annot_opts* aopts, const skm_fidx* fx, skm_best_calls* best, skm_calls* calls,
                     skm_recall_stats* stats);
// the device a DB lives on
int db_device(const skm_db* db);
}  // namespace skm
