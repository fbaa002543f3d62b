// ranges.hip -- range filters: typed attribute columns resident on the device that write per-query allow-bitmaps.
// Callers of a filtered batch hold numeric predicates (timestamp >= t0, price <= p) that no small token set expresses.
// RangeFilter (restricts/mod.rs:73-95) allows start <= index < end on the datapoint index; here that is the row-index
// pseudo-column, and the general form is a conjunction of up to SCANN_HIP_ATTR_MAX_CLAUSES inclusive ranges over int64
// and float columns uploaded once.  A batch sends two 8-byte bounds per (query, clause).
//
// range_bitmap_kernel<NC>: workgroup (t, y) owns tile t (SCANN_HIP_RANGE_TILE_BITS rows) of the bitmaps of the query
// groups y, y + gridDim.y, ... (kRangeQueryGroup queries a group).  Each lane loads its kRangeRowsPerLane rows of
// every clause's column once per tile -- wave w, slot r, lane l holds row tile + (w * R + r) * 64 + l: one coalesced
// load per slot -- and keeps them in registers across the whole query loop (8 bytes a value, an f32 in the low four;
// the row index is computed).  Per query: the bounds are read through wave-uniform loads, each clause compares its R
// rows under a wave-uniform type switch, and one __ballot per slot gives a finished 64-bit word; lanes past the
// capacity vote 0, the only mask the last word needs.  The word of query g, slot r is kept by lane g * R + r (two
// selects, no LDS): after a group every lane holds one word, and the wave stores -- or, for an in-place op, loads,
// combines and stores -- its 64 words with one instruction, the R words of a query contiguous.  A wave's words are
// its own, so the kernel has no barrier and no shared memory: the first form staged a group's words in LDS and stored
// them through store_words, 16 bytes a lane, and spent its time at the barriers, which wait for the stores before
// them (DESIGN 3.3c-r has both measurements).  Under op 0 the last tile of a query also writes the zero gap words up
// to the stride, through store_words.  No clear, no global atomic.
#include <algorithm>
#include <memory>
#include <mutex>
#include <vector>

#include "allow.h"
#include "comm.h"   // ctx_device
#include "handle.h"
#include "launch.h"
#include "ranges.h"
#include "tokens.h"   // store_words, allow_combine_word

namespace scann {

namespace {

constexpr uint32_t kR = kRangeRowsPerLane;
static_assert(kBitmapThreads / 64 * kR == kRangeTileWords, "one ballot word per wave and row slot");
static_assert(kRangeQueryGroup * kR == 64, "after a group every lane of a wave holds one word");

template <int NC>
__global__ __launch_bounds__(kBitmapThreads) void range_bitmap_kernel(RangeClauses cl, const uint64_t *__restrict__ bounds,
                                                                      uint32_t nq, int op, uint64_t bits, uint64_t words,
                                                                      uint64_t stride, uint64_t tiles, uint64_t *out) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t my_g = lane / kR, my_r = lane % kR, my_slot = wave * kR + my_r;   // the query of a group and the tile word this lane stores
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t w0 = min(t * kRangeTileWords, words);
        const uint32_t tile_words = (uint32_t)min((uint64_t)kRangeTileWords, words - w0);
        const bool last_tile = t + 1 == tiles;
        // the tile's values: read once, held across the query loop
        uint64_t v[NC > 0 ? NC : 1][kR];
        uint64_t valid[kR];   // the lanes of slot r that hold a row below the capacity: a wave-uniform mask
        (void)v;              // (NC = 0 holds no value)
#pragma unroll
        for (uint32_t r = 0; r < kR; ++r) {
            const uint64_t row = t * SCANN_HIP_RANGE_TILE_BITS + (uint64_t)(wave * kR + r) * 64u + lane;
            valid[r] = __ballot(row < bits);
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                uint64_t x = row;   // (the row index: computed, not loaded)
                if (row < bits) {
                    if (cl.type[c] == SCANN_HIP_ATTR_I64) x = static_cast<const uint64_t *>(cl.col[c])[row];
                    else if (cl.type[c] == SCANN_HIP_ATTR_F32) x = static_cast<const uint32_t *>(cl.col[c])[row];
                }
                v[c][r] = x;
            }
        }
        for (uint64_t q0 = (uint64_t)blockIdx.y * kRangeQueryGroup; q0 < nq; q0 += (uint64_t)gridDim.y * kRangeQueryGroup) {
            uint64_t mine = 0;
#pragma unroll 4   // (four queries' bounds in flight; sixteen spill the scalar registers)
            for (uint32_t g = 0; g < kRangeQueryGroup; ++g) {
                const uint64_t q = min(q0 + g, (uint64_t)nq - 1);   // (past the batch: the last query again, never stored)
                bool ok[kR];
#pragma unroll
                for (uint32_t r = 0; r < kR; ++r) ok[r] = true;
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    const uint64_t lo = bounds[(q * NC + c) * 2], hi = bounds[(q * NC + c) * 2 + 1];   // (wave-uniform)
                    if (cl.type[c] == SCANN_HIP_ATTR_F32) {
#pragma unroll
                        for (uint32_t r = 0; r < kR; ++r) ok[r] = ok[r] & range_clause_holds(SCANN_HIP_ATTR_F32, v[c][r], lo, hi);
                    } else {
#pragma unroll
                        for (uint32_t r = 0; r < kR; ++r) ok[r] = ok[r] & range_clause_holds(SCANN_HIP_ATTR_I64, v[c][r], lo, hi);
                    }
                }
                // the lane of (g, slot r) keeps ballot r: a select by slot under loop-invariant masks, one by query
                uint64_t word = __ballot(ok[0]) & valid[0];
#pragma unroll
                for (uint32_t r = 1; r < kR; ++r) {
                    const uint64_t b = __ballot(ok[r]) & valid[r];
                    word = my_r == r ? b : word;
                }
                mine = my_g == g ? word : mine;
            }
            const uint64_t q = q0 + my_g;
            if (q < nq && my_slot < tile_words) {
                uint64_t *dst = out + q * stride + w0 + my_slot;
                *dst = op == 0 ? mine : allow_combine_word(op, *dst, mine);
            }
            if (op == 0 && last_tile && stride > words)
                for (uint32_t g = 0; g < kRangeQueryGroup && q0 + g < nq; ++g)
                    store_words(out + (q0 + g) * stride + words, nullptr, stride - words);
        }
    }
}

// ---- argument checks (host-readable arguments only) -------------------------------------------------------------
int check_table_args(uint64_t n, uint32_t n_columns, const int32_t *types, const void *const *columns) {
    if (n >= 0xFFFFFFFFull) return fail(SCANN_HIP_OUT_OF_RANGE, "num_datapoints must be below 2^32 - 1");
    if (n_columns && !types) return fail(SCANN_HIP_INVALID_ARGUMENT, "null types with n_columns > 0");
    for (uint32_t c = 0; c < n_columns; ++c)
        if (types[c] != SCANN_HIP_ATTR_I64 && types[c] != SCANN_HIP_ATTR_F32)
            return fail(SCANN_HIP_INVALID_ARGUMENT, "column " + std::to_string(c) + ": unknown attribute type");
    if (n && n_columns && !columns) return fail(SCANN_HIP_INVALID_ARGUMENT, "null columns with num_datapoints > 0");
    for (uint32_t c = 0; n && c < n_columns; ++c)
        if (!columns[c]) return fail(SCANN_HIP_INVALID_ARGUMENT, "column " + std::to_string(c) + " is null");
    return SCANN_HIP_OK;
}

// everything a call checks but its bounds / output pointers; fills type[c] (0: the row index) of every clause
int check_call_args(uint64_t n, uint32_t n_columns, const int32_t *types, const uint32_t *cols, uint32_t n_cols, int op,
                    uint64_t stride_words, int32_t *clause_type) {
    if (op != 0 && op != SCANN_HIP_ALLOW_AND && op != SCANN_HIP_ALLOW_OR && op != SCANN_HIP_ALLOW_ANDNOT)
        return fail(SCANN_HIP_INVALID_ARGUMENT, "op must be 0 (write), SCANN_HIP_ALLOW_AND, _OR or _ANDNOT");
    if (n_cols > SCANN_HIP_ATTR_MAX_CLAUSES)
        return fail(SCANN_HIP_UNIMPLEMENTED, "more than SCANN_HIP_ATTR_MAX_CLAUSES clauses in one call");
    if (n_cols && !cols) return fail(SCANN_HIP_INVALID_ARGUMENT, "null cols with n_cols > 0");
    for (uint32_t c = 0; c < n_cols; ++c) {
        if (cols[c] != SCANN_HIP_ATTR_ROW_INDEX && cols[c] >= n_columns)
            return fail(SCANN_HIP_INVALID_ARGUMENT, "clause " + std::to_string(c) + ": no such column");
        clause_type[c] = cols[c] == SCANN_HIP_ATTR_ROW_INDEX ? 0 : types[cols[c]];
    }
    return check_block_args(n, stride_words);
}

// words this call reads or writes per row: none of them means the pointers are not needed
bool call_touches_words(uint64_t n, uint32_t nq, int op, uint64_t stride_words) {
    return nq != 0 && (op == 0 ? stride_words : allow_words(n)) != 0;
}

}  // namespace

int range_bitmaps_launch(const RangeClauses &cl, uint32_t n_cols, const uint64_t *d_bounds, uint32_t nq, int op, uint64_t bits,
                         uint64_t stride, uint64_t *d_out, hipStream_t st) {
    const uint64_t words = allow_words(bits);
    if (nq == 0 || (op == 0 ? stride : words) == 0) return SCANN_HIP_OK;
    // (bits = 0: one tile of no words, which owns the gap)
    const uint64_t tiles = std::max<uint64_t>(1, ceil_div_u64(bits, SCANN_HIP_RANGE_TILE_BITS));
    const uint64_t groups = ceil_div_u64(nq, kRangeQueryGroup);
    // a workgroup reads its tile's columns once and walks many query groups with them: as few rows of workgroups as
    // fill the device; tiles and groups beyond the grid are looped over
    const uint32_t gx = (uint32_t)std::min<uint64_t>(tiles, 1u << 20);
    const uint64_t fill = (uint64_t)num_cus() * 16;
    const uint32_t gy = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(groups, 65535), ceil_div_u64(fill, gx)));
    return with_value<0, 1, 2, 3, 4, 5, 6, 7, 8>((int)n_cols, [&](auto nc) {
        return launch(range_bitmap_kernel<decltype(nc)::value>, dim3(gx, gy), dim3(kBitmapThreads), 0, st, cl, d_bounds, nq, op,
                      bits, words, stride, tiles, d_out);
    });
}

}  // namespace scann

using namespace scann;

struct scann_hip_attr_table {
    int device = 0;
    uint64_t n = 0;
    std::vector<int32_t> types;
    std::vector<std::unique_ptr<DevBuf>> cols;
    // the host-pointer forms: one stream and grow-only staging buffers, one call at a time
    std::mutex mu;
    hipStream_t stream = nullptr;
    DevBuf s_bounds;
    FilterSearchBufs fs;   // fs.block: the block of the host-pointer forms
    ~scann_hip_attr_table() {
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace {

int table_clauses(const scann_hip_attr_table *t, const uint32_t *cols, uint32_t n_cols, int op, uint64_t stride_words,
                  RangeClauses *cl) {
    *cl = RangeClauses{};
    SCANN_TRY(check_call_args(t->n, (uint32_t)t->types.size(), t->types.data(), cols, n_cols, op, stride_words, cl->type));
    for (uint32_t c = 0; c < n_cols; ++c) cl->col[c] = cl->type[c] ? t->cols[cols[c]]->p : nullptr;
    return SCANN_HIP_OK;
}

// the host-pointer form under t->mu: bounds up (and the block, for an in-place op), one kernel, the block left in
// t->fs.block (no copy back, no synchronise beyond the uploads')
int stage_block(scann_hip_attr_table *t, const RangeClauses &cl, uint32_t n_cols, const scann_hip_range_bound *bounds,
                uint32_t nq, int op, uint64_t stride, const uint64_t *block_in) {
    const size_t bb = (size_t)nq * n_cols * 16, ob = (size_t)nq * stride * 8;
    SCANN_TRY(t->s_bounds.ensure(bb));
    SCANN_TRY(t->fs.block.ensure(ob));
    if (bb) SCANN_HIP_CHECK(hipMemcpyAsync(t->s_bounds.p, bounds, bb, hipMemcpyHostToDevice, t->stream));
    if (op != 0 && ob) SCANN_HIP_CHECK(hipMemcpyAsync(t->fs.block.p, block_in, ob, hipMemcpyHostToDevice, t->stream));
    return range_bitmaps_launch(cl, n_cols, t->s_bounds.as<uint64_t>(), nq, op, t->n, stride, t->fs.block.as<uint64_t>(),
                                t->stream);
}

}  // namespace

extern "C" {

int scann_hip_attr_table_create(scann_hip_ctx *ctx, uint64_t num_datapoints, uint32_t n_columns, const int32_t *types,
                                const void *const *columns, scann_hip_attr_table **out) {
    if (!out) return fail(SCANN_HIP_INVALID_ARGUMENT, "out is null");
    *out = nullptr;
    if (!ctx) return fail(SCANN_HIP_INVALID_ARGUMENT, "context is null");
    SCANN_TRY(check_table_args(num_datapoints, n_columns, types, columns));
    std::unique_ptr<scann_hip_attr_table> t(new scann_hip_attr_table());
    t->device = ctx_device(ctx);
    t->n = num_datapoints;
    t->types.assign(types, types + n_columns);
    SCANN_HIP_CHECK(hipSetDevice(t->device));
    for (uint32_t c = 0; c < n_columns; ++c) {
        t->cols.emplace_back(new DevBuf());
        const size_t width = types[c] == SCANN_HIP_ATTR_I64 ? 8 : 4;
        SCANN_TRY(upload(*t->cols.back(), num_datapoints ? columns[c] : nullptr, (size_t)num_datapoints * width));
    }
    SCANN_HIP_CHECK(hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking));
    *out = t.release();
    return SCANN_HIP_OK;
}

void scann_hip_attr_table_destroy(scann_hip_attr_table *t) {
    if (!t) return;
    (void)hipSetDevice(t->device);
    delete t;
}

uint64_t scann_hip_attr_table_num_datapoints(const scann_hip_attr_table *t) { return t ? t->n : 0; }

uint32_t scann_hip_attr_table_num_columns(const scann_hip_attr_table *t) { return t ? (uint32_t)t->types.size() : 0; }

int scann_hip_attr_table_column_type(const scann_hip_attr_table *t, uint32_t column) {
    return t && column < t->types.size() ? t->types[column] : 0;
}

int scann_hip_attr_table_allow_bitmaps_device(const scann_hip_attr_table *t, const uint32_t *cols, uint32_t n_cols,
                                              const scann_hip_range_bound *d_bounds, uint32_t nq, int op, uint64_t stride_words,
                                              uint64_t *d_out_words, void *hip_stream) {
    if (!t) return fail(SCANN_HIP_INVALID_ARGUMENT, "attribute table is null");
    RangeClauses cl;
    SCANN_TRY(table_clauses(t, cols, n_cols, op, stride_words, &cl));
    if (!call_touches_words(t->n, nq, op, stride_words)) return SCANN_HIP_OK;
    if ((n_cols && !d_bounds) || !d_out_words) return fail(SCANN_HIP_INVALID_ARGUMENT, "null bounds/output pointer");
    SCANN_HIP_CHECK(hipSetDevice(t->device));
    return range_bitmaps_launch(cl, n_cols, reinterpret_cast<const uint64_t *>(d_bounds), nq, op, t->n, stride_words, d_out_words,
                                static_cast<hipStream_t>(hip_stream));
}

int scann_hip_attr_table_allow_bitmaps(scann_hip_attr_table *t, const uint32_t *cols, uint32_t n_cols,
                                       const scann_hip_range_bound *bounds, uint32_t nq, int op, uint64_t stride_words,
                                       uint64_t *out_words) {
    if (!t) return fail(SCANN_HIP_INVALID_ARGUMENT, "attribute table is null");
    RangeClauses cl;
    SCANN_TRY(table_clauses(t, cols, n_cols, op, stride_words, &cl));
    if (!call_touches_words(t->n, nq, op, stride_words)) return SCANN_HIP_OK;
    if ((n_cols && !bounds) || !out_words) return fail(SCANN_HIP_INVALID_ARGUMENT, "null bounds/output pointer");
    std::lock_guard<std::mutex> lock(t->mu);
    SCANN_HIP_CHECK(hipSetDevice(t->device));
    SCANN_TRY(stage_block(t, cl, n_cols, bounds, nq, op, stride_words, out_words));
    SCANN_HIP_CHECK(hipMemcpyAsync(out_words, t->fs.block.p, (size_t)nq * stride_words * 8, hipMemcpyDeviceToHost, t->stream));
    SCANN_HIP_CHECK(hipStreamSynchronize(t->stream));
    return SCANN_HIP_OK;
}

int scann_hip_allow_bitmaps_from_ranges(uint64_t num_datapoints, uint32_t n_columns, const int32_t *types,
                                        const void *const *columns, const uint32_t *cols, uint32_t n_cols,
                                        const scann_hip_range_bound *bounds, uint32_t nq, int op, uint64_t stride_words,
                                        uint64_t *out_words) {
    SCANN_TRY(check_table_args(num_datapoints, n_columns, types, columns));
    int32_t type[SCANN_HIP_ATTR_MAX_CLAUSES] = {};
    SCANN_TRY(check_call_args(num_datapoints, n_columns, types, cols, n_cols, op, stride_words, type));
    if (!call_touches_words(num_datapoints, nq, op, stride_words)) return SCANN_HIP_OK;
    if ((n_cols && !bounds) || !out_words) return fail(SCANN_HIP_INVALID_ARGUMENT, "null bounds/output pointer");
    const uint64_t words = allow_words(num_datapoints);
    std::vector<uint64_t> range(words);
    for (uint32_t q = 0; q < nq; ++q) {
        std::fill(range.begin(), range.end(), 0ull);
        for (uint64_t j = 0; j < num_datapoints; ++j) {
            bool ok = true;
            for (uint32_t c = 0; c < n_cols && ok; ++c) {
                uint64_t v = j;
                if (type[c] == SCANN_HIP_ATTR_I64) v = static_cast<const uint64_t *>(columns[cols[c]])[j];
                else if (type[c] == SCANN_HIP_ATTR_F32) v = static_cast<const uint32_t *>(columns[cols[c]])[j];
                const scann_hip_range_bound *b = bounds + ((size_t)q * n_cols + c) * 2;
                ok = range_clause_holds(type[c], v, b[0].bits, b[1].bits);
            }
            if (ok) range[j >> 6] |= 1ull << (j & 63u);
        }
        uint64_t *row = out_words + (size_t)q * stride_words;
        for (uint64_t w = 0; w < words; ++w) row[w] = op == 0 ? range[w] : allow_combine_word(op, row[w], range[w]);
        for (uint64_t w = words; op == 0 && w < stride_words; ++w) row[w] = 0;
    }
    return SCANN_HIP_OK;
}

int scann_hip_search_batched_ranges(scann_hip_index *index, scann_hip_attr_table *t, const float *queries, uint32_t nq,
                                    uint32_t q_stride, uint32_t q_dim, uint32_t k, const scann_hip_search_opts *opts,
                                    const uint32_t *cols, uint32_t n_cols, const scann_hip_range_bound *bounds,
                                    uint32_t *out_idx, float *out_dist, uint32_t *out_count) {
    if (!index || !t) return fail(SCANN_HIP_INVALID_ARGUMENT, "null index/attribute table");
    if (nq == 0) return SCANN_HIP_OK;
    SCANN_TRY(filter_search_check(index, queries, q_stride, q_dim, k, opts, out_idx, out_dist, out_count, "the ranges"));
    if (t->n != scann_hip_index_size(index))
        return fail(SCANN_HIP_INVALID_ARGUMENT, "the attribute table's num_datapoints differs from the index's row count");
    if (index->ctx && ctx_device(index->ctx) != t->device)
        return fail(SCANN_HIP_INVALID_ARGUMENT, "the index and the attribute table live on different devices");
    const uint64_t stride = std::max<uint64_t>(allow_words(t->n), 1);   // (a stride of 0 would mean one shared bitmap)
    RangeClauses cl;
    SCANN_TRY(table_clauses(t, cols, n_cols, 0, stride, &cl));
    if (n_cols && !bounds) return fail(SCANN_HIP_INVALID_ARGUMENT, "null bounds pointer");
    scann_hip_search_opts o;
    if (opts) o = *opts;
    else scann_hip_search_opts_default(&o);
    std::lock_guard<std::mutex> lock(t->mu);
    SCANN_HIP_CHECK(hipSetDevice(t->device));
    SCANN_TRY(filter_search_begin(t->fs, t->stream, queries, nq, q_stride, k));
    // the block is built and read on one stream, with nothing between the two enqueues
    SCANN_TRY(stage_block(t, cl, n_cols, bounds, nq, 0, stride, nullptr));
    return filter_search_finish(index, t->fs, t->stream, queries, nq, q_stride, q_dim, k, o, t->n, stride, out_idx, out_dist,
                                out_count);
}

}  // extern "C"
