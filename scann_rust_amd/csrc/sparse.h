// sparse.h -- the host side of the sparse brute-force scan (sparse.hip): constants of the LDS panel,
// the checks made on a batch of sparse queries, the greedy packing of queries into tiles and the row-chunk rule, and
// the constants, LDS size and block-chunk rule of the posting-list scan (sparse_inv.hip).
// Plain C++ with no device code and no HIP types, so that it can be compiled into a stand-alone host program.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#include "../../include/scann_hip.h"

namespace scann {

constexpr uint32_t kSparseQT = SCANN_HIP_SPARSE_TILE_QUERIES;   // queries of a tile: the panel's row width
constexpr uint32_t kSparseSlots = SCANN_HIP_SPARSE_TILE_SLOTS;  // panel rows: distinct dimensions of a tile
constexpr uint32_t kSparseMap = SCANN_HIP_SPARSE_MAP_SIZE;      // open-addressing map entries
constexpr uint32_t kSparseMaxK = SCANN_HIP_SPARSE_MAX_K;
constexpr uint32_t kSparseEmpty = 0xFFFFFFFFu;                  // no dimension: dimensionality <= 2^32 - 1
constexpr uint32_t kSparseThreads = 1024;                       // one workgroup of the scan: 16 waves
constexpr uint32_t kSparseWaves = kSparseThreads / 64;
constexpr uint32_t kSparseRowsInFlight = 64 / kSparseQT;        // rows a wave accumulates side by side
constexpr uint32_t kSparseGroups = 2;                           // row groups a wave scans between two barriers
constexpr uint32_t kSparseRoundRows = kSparseWaves * kSparseRowsInFlight * kSparseGroups;   // rows of a workgroup's round
constexpr uint32_t kSparseChunkRows = 2048;                     // least rows of a chunk
constexpr uint32_t kSparseMergeKeys = 8192;                     // keys the merge kernel sorts in LDS (64 KB)
static_assert(kSparseQT * kSparseRowsInFlight == 64, "a wave is rows-in-flight x tile queries");
static_assert((kSparseMap & (kSparseMap - 1)) == 0 && kSparseMap >= 2 * kSparseSlots, "map: a power of two, at most half full");
static_assert(kSparseSlots >= 1024 && kSparseSlots <= 65536, "slots are u16");
static_assert(kSparseChunkRows % kSparseRoundRows == 0, "chunks are whole rounds");

// Append-buffer entries per query of the selection: room for the k kept keys and for every key one round can add,
// a power of two (it is sorted bitonically).
static inline uint32_t sparse_select_cap(uint32_t k) {
    uint32_t c = 1;
    while (c < k + kSparseRoundRows) c <<= 1;
    return c;
}

// Dynamic LDS of the scan: panel, map keys, map slots, and with a selection the append buffers.
static inline size_t sparse_scan_lds(uint32_t k, bool select) {
    size_t b = (size_t)kSparseSlots * kSparseQT * 4 + (size_t)kSparseMap * 4 + (size_t)kSparseMap * 2;
    if (select) b += (size_t)kSparseQT * sparse_select_cap(k) * 8;
    return b;
}

// Rows per chunk and chunks of a scan over n rows.  A search keeps chunks * k within the merge kernel's LDS sort
// (max_chunks = kSparseMergeKeys / k); the distances entry is bounded by the grid alone (65535).
static inline void sparse_chunks(uint64_t n, uint32_t max_chunks, uint32_t *chunk_rows, uint32_t *chunks) {
    if (max_chunks < 1) max_chunks = 1;
    uint64_t rows = (n + max_chunks - 1) / max_chunks;
    if (rows < kSparseChunkRows) rows = kSparseChunkRows;
    rows = (rows + kSparseRoundRows - 1) / kSparseRoundRows * kSparseRoundRows;
    *chunk_rows = (uint32_t)rows;
    *chunks = n ? (uint32_t)((n + rows - 1) / rows) : 0u;
}

// ---- the posting-list scan (sparse_inv.hip) --------------------------------------------------------------------------
constexpr uint32_t kSparseBlockRows = SCANN_HIP_SPARSE_BLOCK_ROWS;        // rows of a block: one LDS accumulator each
constexpr uint32_t kSparseWaveRows = kSparseBlockRows / kSparseWaves;     // the rows of a block one wave owns
static_assert((kSparseBlockRows & (kSparseBlockRows - 1)) == 0 && kSparseBlockRows <= 65536, "a row inside its block is a u16");
static_assert(kSparseWaveRows >= 64 && kSparseWaveRows % 64 == 0, "a wave's epilogue takes its rows 64 at a time");

// Append-buffer entries of the posting-list scan's one query: the k kept keys and the keys of one epilogue round (one
// row per thread), a power of two.
static inline uint32_t sparse_inv_select_cap(uint32_t k) {
    uint32_t c = 1;
    while (c < k + kSparseThreads) c <<= 1;
    return c;
}

// Dynamic LDS of the posting-list scan: the block's accumulators; per query term its posting range in the block and
// the query's value; with a selection the append buffer.
static inline size_t sparse_inv_lds(uint32_t k, bool select) {
    size_t b = (size_t)kSparseBlockRows * 4 + (size_t)kSparseSlots * 12;
    if (select) b += (size_t)sparse_inv_select_cap(k) * 8;
    return b;
}

// Blocks per chunk and chunks of a posting-list scan over `blocks` blocks: chunks are whole blocks, and a search keeps
// chunks * k within the merge kernel's LDS sort exactly as sparse_chunks does.
static inline void sparse_inv_chunks(uint32_t blocks, uint32_t max_chunks, uint32_t *chunk_blocks, uint32_t *chunks) {
    if (max_chunks < 1) max_chunks = 1;
    uint32_t per = (blocks + max_chunks - 1) / max_chunks;
    if (per < 1) per = 1;
    *chunk_blocks = per;
    *chunks = (blocks + per - 1) / per;
}

// The checks of a batch of sparse queries (ascending offsets; per query strictly ascending dims below dimensionality and
// finite values) and, per query, its sequential f32 squared norm.  SCANN_HIP_OK or InvalidArgument; *why names the check.
static inline int sparse_check_queries(const uint64_t *q_offsets, const uint32_t *q_dims, const float *q_vals, uint32_t nq,
                                       uint32_t dimensionality, std::vector<float> *norms, const char **why) {
    norms->assign(nq, 0.0f);
    const uint64_t o0 = q_offsets[0];
    for (uint32_t q = 0; q < nq; ++q) {
        if (q_offsets[q + 1] < q_offsets[q]) {
            *why = "query offsets are not ascending";
            return SCANN_HIP_INVALID_ARGUMENT;
        }
        float s = 0.0f;
        for (uint64_t e = q_offsets[q] - o0; e < q_offsets[q + 1] - o0; ++e) {
            const uint32_t d = q_dims[e];
            if (d >= dimensionality || (e > q_offsets[q] - o0 && d <= q_dims[e - 1])) {
                *why = "query dims must be strictly ascending and below the dimensionality";
                return SCANN_HIP_INVALID_ARGUMENT;
            }
            if (!isfinite(q_vals[e])) {
                *why = "query values must be finite";
                return SCANN_HIP_INVALID_ARGUMENT;
            }
            s += q_vals[e] * q_vals[e];
        }
        (*norms)[q] = s;
    }
    return SCANN_HIP_OK;
}

// Greedy packing of consecutive queries into tiles: at most kSparseQT queries, and a sum of lengths (an upper bound of
// the tile's union of dimensions) of at most kSparseSlots.  starts gets tiles + 1 query indices.  Unimplemented if one
// query alone is longer than the slot capacity.
static inline int sparse_plan_tiles(const uint64_t *q_offsets, uint32_t nq, std::vector<uint32_t> *starts) {
    starts->clear();
    starts->push_back(0);
    uint32_t in_tile = 0;
    uint64_t slots = 0;
    for (uint32_t q = 0; q < nq; ++q) {
        const uint64_t len = q_offsets[q + 1] - q_offsets[q];
        if (len > kSparseSlots) return SCANN_HIP_UNIMPLEMENTED;
        if (in_tile == kSparseQT || slots + len > kSparseSlots) {
            starts->push_back(q);
            in_tile = 0;
            slots = 0;
        }
        ++in_tile;
        slots += len;
    }
    if (nq) starts->push_back(nq);
    return SCANN_HIP_OK;
}

}  // namespace scann
