// ranges.h -- range filters: typed attribute columns resident on the device that write per-query allow-bitmaps.
// RangeFilter (restricts/mod.rs:73-95) is the row-index case; the general form is a conjunction of inclusive ranges
// over int64 / float columns, one range per (query, clause).
#pragma once
#include "common.h"

namespace scann {

// rows a lane of range_bitmap_kernel holds per clause, 64-bit words of one tile, queries whose words a wave stores at once
constexpr uint32_t kRangeRowsPerLane = 4;
constexpr uint32_t kRangeTileWords = SCANN_HIP_RANGE_TILE_BITS / 64;
constexpr uint32_t kRangeQueryGroup = 64 / kRangeRowsPerLane;
static_assert((SCANN_HIP_RANGE_TILE_BITS & (SCANN_HIP_RANGE_TILE_BITS - 1)) == 0 && SCANN_HIP_RANGE_TILE_BITS >= 128,
              "the tile is a power of two of at least one 16-byte store");

// the clauses of one call, by value in the kernel's arguments: the column of clause c (null for the row index) and its
// SCANN_HIP_ATTR_* type (0: the row index)
struct RangeClauses {
    const void *col[SCANN_HIP_ATTR_MAX_CLAUSES];
    int32_t type[SCANN_HIP_ATTR_MAX_CLAUSES];
};

// one clause at one row: lo <= v <= hi, the signed 64-bit compare or the IEEE f32 compare on the low four bytes (a NaN
// on either side is false; '&', not '&&': no branch per row).  type 0 (the row index) compares as i64.  Host model and kernel share it.
__host__ __device__ static inline bool range_clause_holds(int32_t type, uint64_t v, uint64_t lo, uint64_t hi) {
    if (type == SCANN_HIP_ATTR_F32) {
        const float f = __builtin_bit_cast(float, (uint32_t)v);
        return (__builtin_bit_cast(float, (uint32_t)lo) <= f) & (f <= __builtin_bit_cast(float, (uint32_t)hi));
    }
    return ((int64_t)lo <= (int64_t)v) & ((int64_t)v <= (int64_t)hi);
}

// d_out row q, words [0, ceil(bits / 64)): op 0 writes the conjunction of the n_cols clauses under d_bounds[(q * n_cols
// + c) * 2 + {0, 1}] and zeroes the gap words up to `stride`; SCANN_HIP_ALLOW_AND / _OR / _ANDNOT combine it into the
// words that are there and leave the gap.  Arguments checked by the caller.  Enqueue only: one kernel, no clear, no
// global atomic.
int range_bitmaps_launch(const RangeClauses &cl, uint32_t n_cols, const uint64_t *d_bounds, uint32_t nq, int op, uint64_t bits,
                         uint64_t stride, uint64_t *d_out, hipStream_t st);

}  // namespace scann
