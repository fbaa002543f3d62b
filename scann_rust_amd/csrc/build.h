// build.h -- scann_hip_txh_build (scann_hip.h "device build"): a tree or flat-hasher index trained, encoded and laid
// out on the device from the resident rows of an f32 brute-force handle (build.hip).  The handle itself is put
// together in api_create.hip (index_build_txh), which owns scann_hip_index.
#pragma once
#include <vector>

#include "bf.h"
#include "common.h"

namespace scann {

// What build_txh_device leaves on the device for the new handle.
struct BuildParts {
    DevBuf codes;       // [n][nw] packed code words, CSR row order
    DevBuf leaf_off;    // [L + 1]
    DevBuf leaf_ids;    // [n] (tree only)
    DevBuf centers;     // [L][dim] (tree only)
    DevBuf codebook;    // [S][K][dsub]
    std::vector<uint32_t> off;   // host copy of leaf_off (the planner's, as in the fold)
    uint32_t L = 0;     // leaves: min(num_partitions, n); the tree's leaves (hierarchical); 1 for a flat hasher
};

// Every refusal of scann_hip_txh_build that depends on the rows' shape and the configuration; launches nothing.
int build_check(const BfIndexDev &src, const scann_hip_build_config &cfg);
// Runs stages 0..5 of scann_hip_build_report.stage_ms on `stream` (complete on return); `rep` may be null.
int build_txh_device(const BfIndexDev &src, const scann_hip_build_config &cfg, hipStream_t stream, BuildParts *out,
                     scann_hip_build_report *rep);

// scann_hip_txh_build_hierarchical: step 1 by the level-order k-means tree of ktree.hip (flattened to its leaves), then the
// same stages 2..5 on its centres and leaf assignment.  cfg.num_partitions only says "a tree" (non-zero); out->L is the
// number of leaves found.  More than 16384 leaves: Unimplemented.  `trep` may be null.
int build_txh_hierarchical_device(const BfIndexDev &src, const scann_hip_tree_config &tree,
                                  const scann_hip_build_config &cfg, hipStream_t stream, BuildParts *out,
                                  scann_hip_build_report *rep, scann_hip_tree_report *trep);

// api_create.hip: the new handle around `parts` (taken) and a device copy of src's rows when cfg.store_rows; stage_ms[6].
// proj != nullptr (scann_hip_txh_build_projected): `parts` index the projected rows, [n][out_dim]; the handle copies
// the projection and keeps src's rows as re-rank rows in their own space.
int index_build_txh(const scann_hip_index *src, const scann_hip_build_config &cfg, BuildParts &parts,
                    scann_hip_index **out, scann_hip_build_report *rep, const scann_hip_projection *proj = nullptr);

}  // namespace scann
