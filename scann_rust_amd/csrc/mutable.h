// mutable.h -- what the mutable-index layer (mutable.hip) asks of a base handle (api.hip).
#pragma once
#include "common.h"

namespace scann {

struct BaseView {
    scann_hip_ctx *ctx = nullptr;
    bool brute_force = false;
    const float *rows = nullptr;   // device, [n][stride]; by datapoint index unless rows_csr
    uint64_t n = 0;
    uint32_t dim = 0, stride = 0;
    int measure = 0;               // measure of the handle's final distances (brute force: its own; tree / AH: the re-rank's)
    bool quantized = false, rows_csr = false, partitioned = false, sharded = false;
};
int index_base_view(const scann_hip_index *ix, BaseView *v);

constexpr uint32_t kMutMaxCapacity = SCANN_HIP_MUTABLE_MAX_CAPACITY;
constexpr uint32_t kMutMaxK = SCANN_HIP_MUTABLE_MAX_K;
constexpr uint32_t kMutTile = SCANN_HIP_MUTABLE_DELTA_TILE;   // delta rows sorted per workgroup of delta_scan_kernel

}  // namespace scann
