// stacked.h -- the host side of stacked / additive quantizer handles (stacked.hip): the shape of a
// handle (levels, code positions, table entries), the tile and centroid-slab rules of the fused encode, and the table
// slabs, row chunks and LDS sizes of the ADC scan.
// Plain C++ with no device code and no HIP types, so that it can be compiled into a stand-alone host program.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/scann_hip.h"

namespace scann {

constexpr uint32_t kStackedMaxLevels = SCANN_HIP_STACKED_MAX_LEVELS;
constexpr uint32_t kStackedMaxCodes = SCANN_HIP_STACKED_MAX_CODES;   // T: code bytes of a row
constexpr uint32_t kStackedMaxK = SCANN_HIP_STACKED_MAX_K;           // results of a search
constexpr uint32_t kStackedMaxDim = SCANN_HIP_STACKED_MAX_DIM;
// encode: one workgroup owns a tile of rows whose residuals stay in LDS through every level
constexpr uint32_t kStackedEncThreads = 512;
constexpr uint32_t kStackedEncTileBytes = 64 * 1024;    // residuals, f32 [R][dim | 1]
constexpr uint32_t kStackedEncStageBytes = 32 * 1024;   // one slab of centroids
constexpr uint32_t kStackedEncCodeBytes = 16 * 1024;    // the tile's codes, u8 [R][T]
constexpr uint32_t kStackedEncMaxRows = 256;
constexpr uint32_t kStackedEncMinRows = 4;
// scan: 8 waves, every lane keeps kStackedRowsPerLane rows x (4 queries x quads) accumulators in registers
constexpr uint32_t kStackedScanThreads = 512;
constexpr uint32_t kStackedRowsPerLane = 4;
constexpr uint32_t kStackedRoundRows = kStackedScanThreads * kStackedRowsPerLane;   // rows whose sums are in flight
constexpr uint32_t kStackedSlabBytes = 32 * 1024;       // one of the two table buffers
constexpr uint32_t kStackedMaxQuads = 2;                // query quads of a workgroup
constexpr uint32_t kStackedChunkRows = 4 * kStackedRoundRows;   // least rows of a chunk
constexpr uint32_t kStackedMergeKeys = 8192;            // keys the merge kernel sorts in LDS (64 KB)
static_assert(4 * 256 * 16 * kStackedMaxQuads <= kStackedSlabBytes, "one code dword's tables always fit a slab");
static_assert(kStackedChunkRows % kStackedRoundRows == 0, "chunks are whole rounds");
static_assert(kStackedSlabBytes / 16 <= 4 * kStackedScanThreads, "a thread prefetches at most four entries of a slab");

struct StackedShape {
    uint32_t dim, levels;
    uint32_t T;         // code bytes of a row: the sum of the levels' subspaces
    uint32_t dwords;    // ceil(T / 4): code dwords of a row in the scan layout
    uint32_t entries;   // float4 entries of one query quad's tables, the one-entry tables of the pad positions included
    uint32_t S[kStackedMaxLevels], K[kStackedMaxLevels], dsub[kStackedMaxLevels];
    uint32_t toff[kStackedMaxLevels];    // the level's first code position
    uint32_t eoff[kStackedMaxLevels];    // the level's first table entry
    uint32_t cboff[kStackedMaxLevels];   // the level's first float of the codebooks
    uint32_t cb_floats;
};

// The checks of scann_hip_stacked_create on the shape alone.  SCANN_HIP_OK, InvalidArgument or Unimplemented; *why says which.
static inline int stacked_shape(uint32_t dim, uint32_t levels, const uint32_t *subspaces, const uint32_t *num_codes, StackedShape *out,
                                const char **why) {
    StackedShape sh{};
    if (levels < 1 || levels > kStackedMaxLevels) {
        *why = "num_levels must be in 1..SCANN_HIP_STACKED_MAX_LEVELS";
        return SCANN_HIP_INVALID_ARGUMENT;
    }
    if (dim == 0) {
        *why = "dim must be at least 1";
        return SCANN_HIP_INVALID_ARGUMENT;
    }
    sh.dim = dim;
    sh.levels = levels;
    uint64_t T = 0, e = 0, f = 0;
    for (uint32_t l = 0; l < levels; ++l) {
        const uint32_t S = subspaces[l], K = num_codes[l];
        if (S == 0 || dim % S != 0) {
            *why = "dim must be a multiple of every level's subspaces";
            return SCANN_HIP_INVALID_ARGUMENT;
        }
        if (K < 2 || K > 256) {
            *why = "every level's num_codes must be in 2..256";
            return SCANN_HIP_INVALID_ARGUMENT;
        }
        sh.S[l] = S;
        sh.K[l] = K;
        sh.dsub[l] = dim / S;
        sh.toff[l] = (uint32_t)T;
        sh.eoff[l] = (uint32_t)e;
        sh.cboff[l] = (uint32_t)f;
        T += S;
        e += (uint64_t)S * K;
        f += (uint64_t)K * dim;
        if (T > kStackedMaxCodes) {
            *why = "more than SCANN_HIP_STACKED_MAX_CODES code bytes per row";
            return SCANN_HIP_INVALID_ARGUMENT;
        }
    }
    if (dim > kStackedMaxDim) {
        *why = "dim above SCANN_HIP_STACKED_MAX_DIM (4095): the encode tile of 64 KB cannot hold 4 rows";
        return SCANN_HIP_UNIMPLEMENTED;
    }
    sh.T = (uint32_t)T;
    sh.dwords = (sh.T + 3) / 4;
    sh.entries = (uint32_t)e + (sh.dwords * 4 - sh.T);
    sh.cb_floats = (uint32_t)f;
    *out = sh;
    return SCANN_HIP_OK;
}

// Floats between two rows of the encode tile: odd, so that lanes walking one column each hit 64 different banks.
static inline uint32_t stacked_row_stride(uint32_t dim) { return dim | 1u; }

// Rows of an encode tile: as many as 64 KB of residuals and 16 KB of codes hold, at most 256; below 4 the dim is refused.
static inline uint32_t stacked_tile_rows(uint32_t dim, uint32_t T) {
    uint32_t r = kStackedEncTileBytes / (stacked_row_stride(dim) * 4);
    if (r > kStackedEncCodeBytes / T) r = kStackedEncCodeBytes / T;
    return r > kStackedEncMaxRows ? kStackedEncMaxRows : r;
}

// Centroid slabs of one level of the encode: whole subspaces, `group` at a time, when one fits the stage; else runs of
// `run` codes of one subspace (the additive form).  run >= 2 for every dim the handle accepts.
static inline void stacked_enc_slab(uint32_t K, uint32_t dsub, uint32_t *group, uint32_t *run) {
    const uint32_t stage = kStackedEncStageBytes / 4;
    if (K * dsub <= stage) {
        *group = stage / (K * dsub);
        *run = K;
    } else {
        *group = 1;
        *run = stage / dsub;
    }
}

static inline size_t stacked_enc_lds(uint32_t dim, uint32_t T, uint32_t rows) {
    return (size_t)rows * stacked_row_stride(dim) * 4 + kStackedEncStageBytes + (((size_t)rows * T + 15) & ~(size_t)15);
}

// First table entry of every code position, the pad positions (one +0.0f entry each) included: dwords * 4 + 1 values.
static inline void stacked_entry_offsets(const StackedShape &sh, std::vector<uint32_t> *eoff) {
    eoff->clear();
    uint32_t e = 0;
    for (uint32_t l = 0; l < sh.levels; ++l)
        for (uint32_t s = 0; s < sh.S[l]; ++s, e += sh.K[l]) eoff->push_back(e);
    for (uint32_t t = sh.T; t < sh.dwords * 4; ++t, ++e) eoff->push_back(e);
    eoff->push_back(e);
}

// Table slabs of a scan whose workgroups take `quads` query quads: runs of whole code dwords, ascending, each as long as
// kStackedSlabBytes allows.  slab_dw gets slabs + 1 dword indices.
static inline void stacked_plan_slabs(const StackedShape &sh, const std::vector<uint32_t> &eoff, uint32_t quads,
                                      std::vector<uint32_t> *slab_dw) {
    slab_dw->assign(1, 0u);
    const uint32_t cap = kStackedSlabBytes / (16 * quads);
    uint32_t g0 = 0;
    for (uint32_t g = 1; g <= sh.dwords; ++g) {
        if (eoff[4 * g] - eoff[4 * g0] > cap) {   // (g - 1 > g0: one dword alone always fits)
            slab_dw->push_back(g - 1);
            g0 = g - 1;
        }
    }
    slab_dw->push_back(sh.dwords);
}

// Append-buffer entries per query of the scan's selection: the k kept keys and one key per thread, a power of two.
static inline uint32_t stacked_select_cap(uint32_t k) {
    uint32_t c = 1;
    while (c < k + kStackedScanThreads) c <<= 1;
    return c;
}

// Dynamic LDS of the scan: the two table buffers (one when a single slab holds everything) and the append buffers.
static inline size_t stacked_scan_lds(uint32_t quads, uint32_t k, bool select, uint32_t slabs) {
    size_t b = (size_t)kStackedSlabBytes * (slabs > 1 ? 2 : 1);
    if (select) b += (size_t)quads * 4 * stacked_select_cap(k) * 8;
    return b;
}

// Rows per chunk and chunks of a scan over n rows, as sparse_chunks: a search keeps chunks * k within the merge kernel's
// LDS sort (max_chunks = kStackedMergeKeys / k); the distances entry is bounded by the grid alone (65535).
static inline void stacked_chunks(uint64_t n, uint32_t max_chunks, uint32_t *chunk_rows, uint32_t *chunks) {
    if (max_chunks < 1) max_chunks = 1;
    uint64_t rows = (n + max_chunks - 1) / max_chunks;
    if (rows < kStackedChunkRows) rows = kStackedChunkRows;
    rows = (rows + kStackedRoundRows - 1) / kStackedRoundRows * kStackedRoundRows;
    *chunk_rows = (uint32_t)rows;
    *chunks = n ? (uint32_t)((n + rows - 1) / rows) : 0u;
}

}  // namespace scann
