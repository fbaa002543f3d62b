// fold.h -- the CSR / code half of scann_hip_fold_mutable (fold.hip): arguments and launchers.  The row half
// (live-prefix, gather, delta scatter) and the orchestration live in mutable.hip.
#pragma once
#include "common.h"

namespace scann {

// Everything is a device pointer.  "sorted index" i: the delta rows taken in ascending external id.
struct FoldArgs {
    // old base (a flat hasher: L = 1, leaf_off = {0, n}, leaf_ids = nullptr -- CSR position == datapoint index)
    const uint32_t *leaf_off = nullptr;   // [L + 1]
    const uint32_t *leaf_ids = nullptr;   // [n]
    const uint32_t *codes = nullptr;      // [n][nw]
    uint32_t L = 0, nw = 0, S = 0, bits = 4;
    uint64_t n = 0;
    // live state of the mutable handle
    const uint64_t *live = nullptr;          // [ceil(n / 64)], bits past n clear
    const uint32_t *live_prefix = nullptr;   // exclusive popcount prefix per word (live_prefix_kernel)
    const uint32_t *base_ids = nullptr;      // external id of base row j; nullptr: identity
    // delta
    uint32_t nd = 0;
    const uint32_t *sorted_ids = nullptr;   // [nd] external ids, ascending
    const uint32_t *order = nullptr;        // [nd] delta slot of sorted index i
    const uint32_t *dj = nullptr;           // [nd] new datapoint index of sorted index i (ascending)
    const uint32_t *tok_slot = nullptr;     // [nd] leaf of the row in delta SLOT s; nullptr: every row in leaf 0
    const uint8_t *code8 = nullptr;         // [nd][S] code of the row in delta SLOT s, one byte per subspace
    // scratch (fold_scratch_bytes)
    uint64_t *sbits = nullptr;     // [chunks * kMutFoldChunk / 64] survivor bitmap over CSR positions
    uint32_t *cpref = nullptr;     // [chunks + 1] survivors per chunk, then their exclusive prefix (last = total)
    uint32_t *sbase = nullptr;     // [L + 1] survivors in CSR positions below leaf_off[l]
    uint32_t *doff = nullptr;      // [L + 1] delta rows per leaf, then their exclusive prefix
    uint32_t *dtok = nullptr;      // [nd] leaf of sorted index i
    uint32_t *drank = nullptr;     // [nd] rank of sorted index i among its leaf's delta rows
    uint32_t *dlist = nullptr;     // [nd] sorted indices grouped by leaf, ascending inside a leaf
    uint32_t *flag = nullptr;      // [1] bit 0: a leaf is not strictly ascending; bit 1: a leaf id >= n
    // results
    uint32_t *new_off = nullptr;   // [L + 2]: the new offsets, then a copy of *flag
    uint32_t *new_ids = nullptr;   // [n_new] (unused for a flat hasher)
    uint32_t *new_codes = nullptr; // [n_new][nw]
    uint64_t n_new = 0;
};

// clears what pass 1 accumulates into (doff, flag): two memsets on the stream, kept apart so that a timed span over
// fold_count holds kernels only
int fold_clear(const FoldArgs &a, hipStream_t st);
// pass 1 (after fold_clear): survivor bitmap + per-chunk counts + the ascending check, the delta's per-leaf histogram and ranks, both scans
// and the new offsets (a.new_off complete on return of the stream).  Needs neither new_ids nor new_codes.
int fold_count(const FoldArgs &a, hipStream_t st);
// pass 2: the stable scatter of code words and remapped ids (base survivors and delta rows)
int fold_scatter(const FoldArgs &a, hipStream_t st);

}  // namespace scann
