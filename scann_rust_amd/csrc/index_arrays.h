// index_arrays.h -- a handle's arrays read back to the host (api.hip), for scann_hip_index_write_file (index_file.hip).
#pragma once
#include <vector>

#include "common.h"

namespace scann {

// Host copies of a handle's arrays, as scann_hip_index_write_file stores them (index_file.hip).
struct IndexHostArrays {
    bool brute_force = false;
    scann_hip_txh_desc d{};   // scalar fields; the pointers address the vectors below
    std::vector<float> data, centers, codebook;
    std::vector<uint32_t> leaf_offsets, leaf_ids, codes;   // codes: the device's packed words
    std::vector<uint8_t> rows_q;                           // quantized re-rank rows as stored (d.data is then null) ...
    int rows_q_fmt = 0;                                    // ... their SCANN_HIP_ROWS_* format, 0 = none ...
    float rows_q_inv = 1.0f;                               // ... and the int8 inv_multiplier
    // a projected handle (scann_hip_txh_create_projected): d describes the index space and d.data stays null; `data`
    // holds the original rows, proj_meta[4] floats apart
    uint32_t proj_meta[5] = {0, 0, 0, 0, 0};               // kind (0 = none), in_dim, out_dim, start, row_stride
    std::vector<float> proj_matrix, proj_mean;
};
// with_rows = false: everything but the f32 / quantized rows (d.data stays null; d.n_rows is still the handle's)
int index_download(const scann_hip_index *ix, IndexHostArrays *out, bool with_rows = true);

}  // namespace scann
