// mmr.h -- MMR stage (restricts/crowding.rs:203-268): MmrDiversifier::apply over the rows of a search at k = depth,
// similarity of two datapoints = minus the handle's distance between their stored f32 rows.
#pragma once
#include "common.h"

namespace scann {

constexpr uint32_t kMmrMaxDepth = 2048;   // == the largest brute-force k

// rows_* : [nq][depth] result rows of a search with k = depth (+ rows_cnt [nq]); out_* : [nq][k] / [nq], written in
// selection order.  data: [n][stride] f32 rows by datapoint index; every rows_idx below its row's count is < n (an
// index that is not takes part in no similarity).  lambda in [0, 1].  Enqueue only.
int mmr_launch(const uint32_t *rows_idx, const float *rows_dist, const uint32_t *rows_cnt, uint32_t nq, uint32_t depth,
               const float *data, uint64_t n, uint32_t dim, uint32_t stride, int measure, uint32_t k, float lambda,
               uint32_t *out_idx, float *out_dist, uint32_t *out_cnt, hipStream_t st);

}  // namespace scann
