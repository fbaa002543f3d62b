// txh_stages.h -- the stage launchers that the units of the tree / flat-hasher search define for txh.hip's
// orchestration.  Internal: txh.h stays the interface the api*.hip units and the other sources see.
#pragma once
#include "txh.h"

namespace scann {

// Shape of the scan's work items, which the work lists are cut to: points per tile chunk, query quads per tile,
// chunks per tile.
struct WorkTiling {
    uint32_t tp, qpt, cpt;
};

// ---- txh_partition.hip: K1, K3, K4 ----
int launch_ah_tokens(const TxhIndexDev &ix, const TxhWork &w, hipStream_t st);
int launch_centroid_scores(const TxhIndexDev &ix, const TxhWork &w, hipStream_t st);
// flat hasher (one implicit leaf, P = 1): partition and work lists in one launch
int launch_ah_setup(const TxhIndexDev &ix, const TxhWork &w, const WorkTiling &t, hipStream_t st);
int launch_work_init(const TxhIndexDev &ix, const TxhWork &w, hipStream_t st);
int launch_work_lists(const TxhIndexDev &ix, const TxhWork &w, const WorkTiling &t, hipStream_t st);
int launch_lut_build(const TxhIndexDev &ix, const TxhWork &w, hipStream_t st);

// ---- txh_prefilter.hip: K6d / K6e, the integer-MFMA prefilters and the refine ----
int launch_lut8_build(const TxhWork &w, uint32_t S, int fold, hipStream_t st);
int launch_prefilter_refine(const TxhIndexDev &ix, const TxhWork &w, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1);

// ---- txh_rows.hip: the 8-bit row stores of the re-rank filter (K8b) ----
int launch_rerank_i8(const TxhIndexDev &ix, const TxhWork &w, hipStream_t st);
// ... and the re-rank of a handle whose rows are stored quantized (ix.qrows): cand_exact of every candidate
int launch_rerank_quant(const TxhIndexDev &ix, const TxhWork &w, hipStream_t st);

}  // namespace scann
