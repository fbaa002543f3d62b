// mutable.h -- what the mutable-index layer (mutable.hip) asks of a base handle (handle.h; the views are in api.hip).
#pragma once
#include <vector>

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
    bool projected = false;        // scann_hip_txh_create_projected: the rows are not in the index's space
};
int index_base_view(const scann_hip_index *ix, BaseView *v);

// The arrays of an unsharded tree / hasher base that scann_hip_fold_mutable reads (device pointers, owned by the base).
// A flat hasher has L = 1, leaf_off = {0, n}, leaf_ids = centers = nullptr: CSR position == datapoint index.
struct FoldView {
    uint32_t L = 0, S = 0, K = 0, dsub = 0, nw = 0;
    int ah = 0, use_residuals = 0;
    uint64_t n_local = 0, n_rows = 0;
    const uint32_t *leaf_off = nullptr, *leaf_ids = nullptr, *codes = nullptr;
    const float *centers = nullptr, *codebook = nullptr;
};
int index_fold_view(const scann_hip_index *ix, FoldView *v);
// New handles over arrays the fold wrote on the device.  The buffers are TAKEN (left empty) on success and on failure
// alike; model (centres, codebook, measure, search defaults) is copied from `old` device to device; everything derived is
// built by the finish half of scann_hip_bf_create / scann_hip_txh_create (api_create.hip).  off: host copy of leaf_off.
int index_fold_bf(const scann_hip_index *old, DevBuf &rows, uint64_t n, uint32_t stride, scann_hip_index **out);
int index_fold_txh(const scann_hip_index *old, DevBuf &rows, DevBuf &codes, DevBuf &leaf_off, DevBuf &leaf_ids,
                   const std::vector<uint32_t> &off, uint64_t n, uint32_t stride, scann_hip_index **out);

constexpr uint32_t kMutFoldChunk = SCANN_HIP_FOLD_CHUNK;   // CSR positions per workgroup of the fold's count / scatter passes
constexpr uint32_t kMutMaxCapacity = SCANN_HIP_MUTABLE_MAX_CAPACITY;
constexpr uint32_t kMutMaxK = SCANN_HIP_MUTABLE_MAX_K;
constexpr uint32_t kMutTile = SCANN_HIP_MUTABLE_DELTA_TILE;   // delta rows sorted per workgroup of delta_scan_kernel

}  // namespace scann
