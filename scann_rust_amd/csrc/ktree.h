// ktree.h -- the hierarchical partitioner of scann_hip_txh_build_hierarchical (scann_hip.h "hierarchical device
// build"): KMeansTree::build_node (trees/kmeans_tree.rs:212-267) level by level on the device, flattened to its leaves
// as TreePartitioner::build_hierarchical does (partitioning/tree_partitioner.rs:101-140).  ktree.hip.
#pragma once
#include "bf.h"
#include "build.h"
#include "common.h"

namespace scann {

constexpr uint32_t kTreeMaxDepth = 4;   // levels 0..4 of scann_hip_tree_report

// Every refusal that depends on the tree configuration alone; launches nothing.
int ktree_check(const scann_hip_tree_config &tree);

// Step 1 of the rule on `stream` (complete on return): out->centers [L][dim] (the ordered f64 mean of every leaf),
// out->leaf_ids [n] (leaf by leaf in depth-first order, ascending datapoint index inside a leaf), out->leaf_off [L + 1]
// with its host copy out->off, out->L, and d_leaf [n] = the leaf of every datapoint.  rep (may be null): the root's
// k-means in the partition_* slots, the seeding and Lloyd time of all levels in stage_ms[0] and [1].  trep may be null.
// More than kMaxLeavesSelect leaves: Unimplemented, `out` is to be dropped by the caller.
int ktree_build_device(const BfIndexDev &src, const scann_hip_tree_config &tree, uint32_t simd_threshold,
                       hipStream_t stream, BuildParts *out, DevBuf *d_leaf, scann_hip_build_report *rep,
                       scann_hip_tree_report *trep);

}  // namespace scann
