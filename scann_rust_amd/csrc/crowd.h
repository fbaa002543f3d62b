// crowd.h -- crowding stage (restricts/crowding.rs:81-104): at most per_crowd_limit results per attribute.
#pragma once
#include "common.h"

namespace scann {

constexpr uint32_t kCrowdMaxDepth = 8192;    // == kMaxPreReorderK: the longest row any handle's final select leaves
constexpr uint32_t kCrowdMinSlots = 128;
constexpr uint32_t kCrowdMaxSlots = 12288;   // 12 bytes per slot: 144 KB of the workgroup's 160 KB
constexpr uint32_t kCrowdMaxDims = 8;        // attribute dimensions of the multi-attribute stage
constexpr uint32_t kCrowdMdMaxKeys = kCrowdMaxSlots / 2;   // n_dims * min(k, depth): table keys of that stage

// Slots of the LDS attribute table for rows of `depth` entries (scann_hip_crowd_table_slots).
uint32_t crowd_table_slots(uint32_t depth);

// rows_* : [nq][depth] result rows of a search with k = depth (+ rows_cnt [nq]); out_* : [nq][k] / [nq].
// attrs: [n_attrs] device array, may be null when n_attrs == 0 (every attribute is then 0).  Enqueue only.
int crowd_launch(const uint32_t *rows_idx, const float *rows_dist, const uint32_t *rows_cnt, uint32_t nq,
                 uint32_t depth, const uint64_t *attrs, uint64_t n_attrs, uint32_t k, uint32_t limit,
                 uint32_t *out_idx, float *out_dist, uint32_t *out_cnt, hipStream_t st);

// CrowdingMultidimensional::apply (restricts/crowding.rs:166-200).  attrs: [n_dims][n_attrs] device array, dimension-
// major; limits: [n_dims] HOST array.  n_dims * min(k, depth) > kCrowdMdMaxKeys -> Unimplemented.  Enqueue only.
int crowd_md_launch(const uint32_t *rows_idx, const float *rows_dist, const uint32_t *rows_cnt, uint32_t nq,
                    uint32_t depth, const uint64_t *attrs, uint32_t n_dims, uint64_t n_attrs, uint32_t k,
                    const uint32_t *limits, uint32_t *out_idx, float *out_dist, uint32_t *out_cnt, hipStream_t st);

}  // namespace scann
